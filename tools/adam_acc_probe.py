"""A gradient-accumulating optimizer step with everything offloaded: the fused Adam reading its
gradient from the remote fp32 accumulators and zeroing them in the same pass
(OffloadedAdam.step(accumulator=acc), ocm_x_adam_multi_acc) against the sequence it replaces,
acc.read(), the copy into .grad, opt.step(), acc.zero().

    python tools/adam_acc_probe.py --out out/adam_acc_probe.json [--mi 64] [--tensors 8]

One process. Per case `--rounds` alternating runs of each sequence, a run being warm-up calls and
then the mean of `--reps` timed calls (issue to torch.cuda.synchronize plus ocm_wait on both
allocations); the row reports the median run and every run. The accumulators hold zeros
throughout, which changes no timing: both sequences move every byte whatever it holds. Over the
link both read 12 bytes per parameter (moments and accumulators; 16 with bf16 masters) and write
12 (16); the earlier sequence does it in three passes and adds a local copy.

Cases: fp32 parameters with the moments and the accumulators both in the pinned host tier; the
same with both in another daemon's HBM on the same GPU (a stand-in for a peer GPU: no xGMI hop is
measured); bf16 parameters on the host tier.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oncilla_amd import api  # noqa: E402
from oncilla_amd.models import OffloadedAdam, OffloadedGradAccumulator  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402


def run(fn, allocs, warmup, reps):
    def settle():
        torch.cuda.synchronize()
        for a in allocs:
            a.wait()

    for _ in range(warmup):
        fn()
    settle()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        settle()
    return (time.perf_counter() - t0) / reps


def case(label, n_daemons, flags, dtype, elems, tensors, warmup, reps, rounds):
    with Mesh(n_daemons, gpus=[0] * n_daemons) as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            params = [torch.nn.Parameter(torch.randn(elems // tensors, device="cuda:0").to(dtype)) for _ in range(tensors)]
            opt = OffloadedAdam(params, c, lr=1e-3, flags=flags)
            in_place = OffloadedGradAccumulator(params, c, flags=flags, readback=False)
            staged = OffloadedGradAccumulator(params, c, flags=flags)  # built last: .grad are views of its local half

            def earlier():
                sums = staged.read()
                with torch.no_grad():
                    for p, g in zip(params, sums):
                        p.grad.copy_(g)
                opt.step()
                staged.zero()

            def fused():
                opt.step(accumulator=in_place)

            allocs = [opt.allocs[0], staged.alloc, in_place.alloc]
            new, old = [], []
            for _ in range(rounds):  # alternating
                new.append(run(fused, allocs, warmup, reps))
                old.append(run(earlier, allocs, warmup, reps))
            tiers = {"state": sorted({e["tier"] for e in opt.allocs[0].remote_info()["extents"]}),
                     "accumulators": sorted({e["tier"] for e in in_place.alloc.remote_info()["extents"]})}
            local = {"staged": staged.local_bytes, "in_place": in_place.local_bytes}
            for o in (staged, in_place, opt):
                o.close()
    mn, mo = statistics.median(new), statistics.median(old)
    row = {"case": label, "pool_tiers": tiers, "params": elems, "tensors": tensors,
           "dtype": str(dtype).replace("torch.", ""),
           "read_copy_step_zero_ms": round(mo * 1e3, 3), "read_copy_step_zero_ms_runs": [round(t * 1e3, 3) for t in old],
           "step_accumulator_ms": round(mn * 1e3, 3), "step_accumulator_ms_runs": [round(t * 1e3, 3) for t in new],
           "speedup": round(mo / mn, 3), "accumulator_local_bytes": local, "warmup": warmup, "reps": reps, "rounds": rounds}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mi", type=int, default=64, help="Mi parameters")
    ap.add_argument("--tensors", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_acc_probe measures on a GPU; none is visible")
    elems = args.mi << 20
    cases = [("fp32_host_tier", 1, api.OCM_ALLOC_HOST_TIER, torch.float32),
             ("fp32_same_gpu_hbm_stand_in", 2, 0, torch.float32),
             ("bf16_host_tier", 1, api.OCM_ALLOC_HOST_TIER, torch.bfloat16)]
    rows = [case(label, n, flags, dt, elems, args.tensors, args.warmup, args.reps, args.rounds)
            for label, n, flags, dt in cases]
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
