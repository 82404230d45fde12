"""Gather of random table rows by ids that live on the GPU: one indexed op
(Allocation.indexed_batch, the ids read by the kernel) against what a caller does without
it (the baseline: existing code): the ids copied to the host, one ocm_params per row, one
Allocation.batch.

    python tools/indexed_probe.py --out out/indexed_probe.json

Per case the two ways alternate, `--reps` timed runs each after warm-up. A run starts
with the ids in device memory and ends when Allocation.wait() returns: `host_us` is the
time before the launch returns (indexed: validation, planning and the launch; baseline:
the device-to-host copy of the ids with its sync, building the descriptors, validation,
planning, their upload and the launch), `total_us` the whole call, `copy_us` their
difference (what is left to wait for once the launch has returned).
Tables: the pinned host tier (1 daemon) and, labelled as a stand-in, HBM of the same GPU
striped over three daemons (--hbm; an xGMI figure would be a bound, not a measurement).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oncilla_amd import api  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402

TABLE_ROWS = 1 << 17


def one(run, alloc):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    t1 = time.perf_counter()
    alloc.wait()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t0) * 1e6


def stats(samples):
    out = {}
    for name, vals in (("host_us", [s[0] for s in samples]), ("total_us", [s[1] for s in samples]),
                       ("copy_us", [s[1] - s[0] for s in samples])):
        v = sorted(vals)
        out[name] = round(v[len(v) // 2], 1)
        out[name + "_min_max"] = [round(v[0], 1), round(v[-1], 1)]
    return out


def case(label, n_daemons, n_ids, row_bytes, warmup, reps):
    out_bytes = n_ids * row_bytes
    ids_off = (out_bytes + 15) // 16 * 16
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=ids_off + 8 * n_ids, remote_bytes=TABLE_ROWS * row_bytes,
                        flags=api.OCM_ALLOC_STRIPE)
            tiers = sorted({e["tier"] for e in a.remote_info()["extents"]})
            raw = a.local_tensor(torch.uint8)
            ids_dev = raw[ids_off: ids_off + 8 * n_ids].view(torch.int64)
            ids_dev.copy_(torch.randint(0, TABLE_ROWS, (n_ids,), generator=torch.Generator().manual_seed(n_ids)))
            torch.cuda.synchronize()
            indexed = api.indexed_ops([[0, 0, 0, row_bytes, n_ids, row_bytes, row_bytes, api.OCM_INDEX_NONE, ids_off,
                                        n_ids, TABLE_ROWS]], api.OCM_INDEX_I64)
            lo = np.arange(n_ids, dtype=np.int64) * row_bytes

            def baseline():
                ids = ids_dev.cpu().numpy()  # the sync a caller pays today
                ops = np.stack([np.zeros_like(ids), lo, ids * row_bytes, np.full_like(ids, row_bytes)], axis=1)
                a.batch(api.batch_ops(ops), async_=True)

            ways = {"indexed": lambda: a.indexed_batch(indexed, async_=True), "ids_to_host_batch": baseline}
            # both ways bring the same rows
            got = []
            for fn in ways.values():
                raw[:out_bytes].zero_()
                torch.cuda.synchronize()
                fn()
                a.wait()
                got.append(raw[:out_bytes].clone())
            assert torch.equal(got[0], got[1]), "the indexed op and the batch of rows disagree"
            samples = {k: [] for k in ways}
            for i in range(warmup + reps):  # the two alternate
                for k, fn in ways.items():
                    s = one(fn, a)
                    if i >= warmup:
                        samples[k].append(s)
            row = {"case": label, "ids": n_ids, "row_bytes": row_bytes, "table_rows": TABLE_ROWS, "pool_tiers": tiers,
                   "bytes": out_bytes, "warmup": warmup, "reps": reps,
                   "indexed": {"descriptors": 1, **stats(samples["indexed"])},
                   "ids_to_host_batch": {"descriptors": n_ids, **stats(samples["ids_to_host_batch"])}}
            lo_b, hi_b = row["ids_to_host_batch"]["copy_us_min_max"]
            cu = row["indexed"]["copy_us"]
            row["indexed_copy_vs_baseline_span"] = "below" if cu < lo_b else "inside" if cu <= hi_b else "above"
            row["indexed_GiBps"] = round(out_bytes / row["indexed"]["total_us"] * 1e6 / 2**30, 2)
            row["ids_to_host_batch_GiBps"] = round(out_bytes / row["ids_to_host_batch"]["total_us"] * 1e6 / 2**30, 2)
            print(json.dumps(row), flush=True)
            a.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--row-bytes", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (4 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for label, n_daemons in [("host_tier_table", 1)] + ([("same_gpu_hbm_stand_in_striped3", 4)] if args.hbm else []):
        for rb in args.row_bytes:
            for n in args.ids:
                rows.append(case(label, n_daemons, n, rb, args.warmup, args.reps))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
