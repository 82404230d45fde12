"""fp32 gradient accumulators in disaggregated memory: one one-sided accumulate
(Allocation.accumulate_batch) against what the library could do without it, a get into an
fp32 staging buffer in HBM, torch's add_(g, alpha=s) and a put back, stream-ordered.

    python tools/acc_probe.py --out out/acc_probe.json [--hbm] [--mib 64 1024]

Per case (pool placement x accumulator size x gradient dtype): `--rounds` alternating runs of
each variant, a run being warm-up calls and then the mean of `--reps` timed calls (issue to
torch.cuda.synchronize plus ocm_wait); the row reports the median run and the spread.
Pools: the pinned host tier (1 daemon) and, labelled as a stand-in, HBM of the same GPU
striped over three daemons (--hbm). Both variants move the same 8 bytes per element over
the link; GiB/s counts accumulator bytes once.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oncilla_amd import api  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402

SCALE = 0.25


def run(fn, a, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a.wait()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        a.wait()
    return (time.perf_counter() - t0) / reps


def case(label, n_daemons, mib, dtype, warmup, reps, rounds):
    elems = (mib << 20) // 4
    esize = torch.empty((), dtype=dtype).element_size()
    gbytes, abytes = elems * esize, elems * 4
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            # local half: [gradients | fp32 staging (the baseline's only)]
            a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=gbytes + abytes, remote_bytes=abytes, flags=api.OCM_ALLOC_STRIPE)
            local = a.local_tensor(torch.uint8)
            g = local[:gbytes].view(dtype)
            stage = local[gbytes:].view(torch.float32)
            g.normal_()
            stage.zero_()
            a.put(gbytes, 0, abytes)
            ops = api.acc_ops(np.array([[0, 0, elems]]), dtype, SCALE)

            def candidate():
                a.stream_wait()
                a.accumulate_batch(ops, async_=True)
                a.stream_signal()

            def baseline():
                a.stream_wait()
                a.get(gbytes, 0, abytes, async_=True)
                a.stream_signal()
                stage.add_(g, alpha=SCALE)
                a.stream_wait()
                a.put(gbytes, 0, abytes, async_=True)
                a.stream_signal()

            cand, base = [], []
            for _ in range(rounds):  # alternating
                cand.append(run(candidate, a, warmup, reps))
                base.append(run(baseline, a, warmup, reps))
            tiers = sorted({e["tier"] for e in a.remote_info()["extents"]})
            a.free()
    mc, mb = statistics.median(cand), statistics.median(base)
    row = {"case": label, "pool_tiers": tiers, "accumulator_MiB": mib, "grad_dtype": str(dtype).replace("torch.", ""),
           "elems": elems, "accumulate_us": round(mc * 1e6, 1),
           "accumulate_us_runs": [round(t * 1e6, 1) for t in cand],
           "get_add_put_us": round(mb * 1e6, 1), "get_add_put_us_runs": [round(t * 1e6, 1) for t in base],
           "speedup": round(mb / mc, 3), "accumulate_GiBps": round(abytes / mc / 2**30, 1),
           "get_add_put_GiBps": round(abytes / mb / 2**30, 1), "warmup": warmup, "reps": reps, "rounds": rounds}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, nargs="+", default=[64, 1024], help="MiB of fp32 accumulators")
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (4 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("acc_probe measures on a GPU; none is visible")
    places = [("host_tier_pool", 1)] + ([("same_gpu_hbm_stand_in_striped3", 4)] if args.hbm else [])
    rows = [case(label, n, mib, dt, args.warmup, args.reps, args.rounds)
            for label, n in places for mib in args.mib for dt in (torch.bfloat16, torch.float32)]
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
