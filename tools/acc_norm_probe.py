"""The global gradient norm over remote fp32 accumulators, computed where they live
(OffloadedGradAccumulator.sumsq, ocm_x_acc_sumsq: one read-only pass and a finishing kernel)
against the only alternative before it, acc.read() + torch.linalg.vector_norm on the read-back
region; and the clipped optimizer step, OffloadedAdam.step(accumulator=acc, max_norm=...), against
the unclipped one.

    python tools/acc_norm_probe.py --out out/acc_norm_probe.json [--mi 64] [--tensors 8]

One process. Per case `--rounds` alternating runs of each sequence, a run being warm-up calls and
then the mean of `--reps` timed calls (issue to torch.cuda.synchronize plus ocm_wait on the
allocations); the row reports the median run and every run. The accumulators hold zeros
throughout, which changes no timing: every sequence moves every byte whatever it holds. The
clipped step adds the norm pass (4 bytes per parameter read over the link) and one host
synchronise to the unclipped step's single pass.

Cases: accumulators (and, for the steps, moments) in the pinned host tier; the same in another
daemon's HBM on the same GPU (a stand-in for a peer GPU: no xGMI hop is measured).
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


def case(label, n_daemons, flags, elems, tensors, warmup, reps, rounds):
    with Mesh(n_daemons, gpus=[0] * n_daemons) as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            params = [torch.nn.Parameter(torch.randn(elems // tensors, device="cuda:0")) for _ in range(tensors)]
            opt = OffloadedAdam(params, c, lr=1e-3, flags=flags)
            in_place = OffloadedGradAccumulator(params, c, flags=flags, readback=False)
            staged = OffloadedGradAccumulator(params, c, flags=flags)

            def in_place_norm():
                in_place.sumsq()

            def read_back_norm():
                torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in staged.read()]))

            def unclipped():
                opt.step(accumulator=in_place)

            def clipped():
                opt.step(accumulator=in_place, max_norm=1.0, skip_nonfinite=True)

            allocs = [opt.allocs[0], staged.alloc, in_place.alloc]
            t = {"sumsq": [], "read_norm": [], "step": [], "step_clipped": []}
            for _ in range(rounds):  # alternating
                t["sumsq"].append(run(in_place_norm, allocs, warmup, reps))
                t["read_norm"].append(run(read_back_norm, allocs, warmup, reps))
                t["step_clipped"].append(run(clipped, allocs, warmup, reps))
                t["step"].append(run(unclipped, allocs, warmup, reps))
            tiers = sorted({e["tier"] for e in in_place.alloc.remote_info()["extents"]})
            for o in (staged, in_place, opt):
                o.close()
    med = {k: statistics.median(v) for k, v in t.items()}
    row = {"case": label, "pool_tiers": tiers, "params": elems, "tensors": tensors, "dtype": "float32",
           "sumsq_ms": round(med["sumsq"] * 1e3, 3), "sumsq_ms_runs": [round(x * 1e3, 3) for x in t["sumsq"]],
           "sumsq_gb_per_s": round(4 * elems / med["sumsq"] / 1e9, 1),
           "read_vector_norm_ms": round(med["read_norm"] * 1e3, 3),
           "read_vector_norm_ms_runs": [round(x * 1e3, 3) for x in t["read_norm"]],
           "sumsq_speedup": round(med["read_norm"] / med["sumsq"], 3),
           "step_ms": round(med["step"] * 1e3, 3), "step_ms_runs": [round(x * 1e3, 3) for x in t["step"]],
           "step_clipped_ms": round(med["step_clipped"] * 1e3, 3),
           "step_clipped_ms_runs": [round(x * 1e3, 3) for x in t["step_clipped"]],
           "clipped_over_unclipped": round(med["step_clipped"] / med["step"], 3),
           "warmup": warmup, "reps": reps, "rounds": rounds}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mi", type=int, default=64, help="Mi accumulators")
    ap.add_argument("--tensors", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("acc_norm_probe measures on a GPU; none is visible")
    elems = args.mi << 20
    cases = [("host_tier", 1, api.OCM_ALLOC_HOST_TIER), ("same_gpu_hbm_stand_in", 2, 0)]
    rows = [case(label, n, flags, elems, args.tensors, args.warmup, args.reps, args.rounds) for label, n, flags in cases]
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
