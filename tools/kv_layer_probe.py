"""Layer-major KV-cache block swap (PagedKVOffload layers=32, 2 KiB rows, 64 KiB per
block): one strided op per block (Allocation.strided_batch) against the same transfer
expanded into one plain op per row (Allocation.batch, the baseline: existing code).

    python tools/kv_layer_probe.py --out out/kv_layer_probe.json

Per case and direction the two ways alternate, `--reps` timed runs each after warm-up.
A run is one async call on prepared descriptor lists followed by Allocation.wait():
`host_us` is the call itself (validation, planning, the descriptor upload and the
launch: the host time before the launch returns), `total_us` ends when the wait does.
Pools: the pinned host tier (1 daemon) and, labelled as a stand-in, HBM of the same GPU
striped over three daemons (--hbm; an xGMI figure would be a bound, not a measurement).
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oncilla_amd import api  # noqa: E402
from oncilla_amd.models import PagedKVOffload  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402

BLOCK = (2, 8, 64)  # K+V, 8 kv heads x 64 (one token slice), fp16 = 2 KiB per layer
LAYERS = 32         # 64 KiB per logical block


def expand(kv, pairs, put):
    """One plain op per row of each block: [op_flag, local_offset, remote_offset, bytes]."""
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    g, p = (a[:, 0], a[:, 1]) if put else (a[:, 1], a[:, 0])
    layer = np.arange(kv.layers, dtype=np.int64)
    bb = kv.block_bytes
    lo = (g[:, None] * bb + layer[None, :] * kv.num_gpu_blocks * bb).reshape(-1)
    ro = (p[:, None] * kv.pool_block_bytes + layer[None, :] * bb).reshape(-1)
    return np.stack([np.full_like(lo, 1 if put else 0), lo, ro, np.full_like(lo, bb)], axis=1)


def one(run, alloc):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    t1 = time.perf_counter()
    alloc.wait()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t0) * 1e6


def stats(samples):
    host = sorted(s[0] for s in samples)
    total = sorted(s[1] for s in samples)
    return {"total_us": round(total[len(total) // 2], 1), "total_us_min_max": [round(total[0], 1), round(total[-1], 1)],
            "host_us": round(host[len(host) // 2], 1), "host_us_min_max": [round(host[0], 1), round(host[-1], 1)]}


def case(label, n_daemons, n_swap, warmup, reps):
    rng = random.Random(0)
    n_gpu_blocks, n_pool_blocks = n_swap, 2 * n_swap
    rows = []
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            kv = PagedKVOffload(c, n_gpu_blocks, n_pool_blocks, BLOCK, layers=LAYERS)
            kv.gpu_cache.normal_()
            torch.cuda.synchronize()
            pairs = np.array(list(zip(rng.sample(range(n_gpu_blocks), n_swap), rng.sample(range(n_pool_blocks), n_swap))),
                             dtype=np.int64)
            tiers = sorted({e["tier"] for e in kv.alloc.remote_info()["extents"]})
            # both ways move the same bytes: out strided, back expanded, and the cache is as it was
            want = kv.gpu_cache.clone()
            kv.alloc.strided_batch(kv._ops(pairs, put=True))
            kv.gpu_cache.zero_()
            torch.cuda.synchronize()
            kv.alloc.batch(api.batch_ops(expand(kv, pairs[:, ::-1].copy(), False)))
            assert torch.equal(kv.gpu_cache, want), "strided out + expanded in did not restore the cache"
            del want
            for direction, put, pr in (("swap_out", True, pairs), ("swap_in", False, pairs[:, ::-1].copy())):
                t0 = time.perf_counter()
                strided = kv._ops(pr, put=put)
                t1 = time.perf_counter()
                expanded = api.batch_ops(expand(kv, pr, put))
                t2 = time.perf_counter()
                ways = {"strided": lambda: kv.alloc.strided_batch(strided, async_=True),
                        "expanded_batch": lambda: kv.alloc.batch(expanded, async_=True)}
                samples = {k: [] for k in ways}
                for i in range(warmup + reps):  # the two alternate
                    for k, fn in ways.items():
                        s = one(fn, kv.alloc)
                        if i >= warmup:
                            samples[k].append(s)
                row = {"case": label, "direction": direction, "blocks": n_swap, "layers": LAYERS,
                       "row_bytes": kv.block_bytes, "block_KiB": kv.pool_block_bytes >> 10, "pool_tiers": tiers,
                       "bytes": n_swap * kv.pool_block_bytes, "warmup": warmup, "reps": reps,
                       "strided": {"descriptors": strided.n, "build_list_us": round((t1 - t0) * 1e6, 1), **stats(samples["strided"])},
                       "expanded_batch": {"descriptors": expanded.n, "build_list_us": round((t2 - t1) * 1e6, 1),
                                          **stats(samples["expanded_batch"])}}
                lo, hi = row["expanded_batch"]["total_us_min_max"]
                row["strided_median_vs_baseline_span"] = ("below" if row["strided"]["total_us"] < lo else
                                                          "inside" if row["strided"]["total_us"] <= hi else "above")
                row["strided_GiBps"] = round(row["bytes"] / row["strided"]["total_us"] * 1e6 / 2**30, 1)
                row["expanded_batch_GiBps"] = round(row["bytes"] / row["expanded_batch"]["total_us"] * 1e6 / 2**30, 1)
                print(json.dumps(row), flush=True)
                rows.append(row)
            kv.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (4 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for n in args.blocks:
        rows += case("host_tier_pool", 1, n, args.warmup, args.reps)
    if args.hbm:
        rows += case("same_gpu_hbm_stand_in_striped3", 4, args.blocks[0], args.warmup, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
