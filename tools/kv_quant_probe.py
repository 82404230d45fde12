"""KV-cache block swap, plain against MXFP8-compressed (PagedKVOffload compress=None /
"mxfp8"): random 64 KiB fp16 blocks out to the pool and back in.

    python tools/kv_quant_probe.py --compress none  --out out/kv_quant_none.json
    python tools/kv_quant_probe.py --compress mxfp8 --out out/kv_quant_mxfp8.json

One process per mode (a fresh daemon, a fresh library state). compress=None is the
unchanged batch path. Per case: warm-up swaps, then the median and the spread of
`--reps` timed swaps (launch to torch.cuda.synchronize), the bytes the swap puts on
the wire, and GiB/s of *source* bytes (16-bit elements), whatever the wire carried.
Pools: the pinned host tier (1 daemon) and, labelled as a stand-in, HBM of the same
GPU striped over three daemons (--hbm).

    python tools/kv_quant_probe.py --format mxfp4 --reps 5 --out out/kv_mx4_probe.json

With --format the three pools (plain, MXFP8 and the given format) live in one process and
their swaps alternate, `--reps` timed runs each after warm-up: one row per case with the
medians side by side and the ratios next to the byte ratios. Without it nothing changes.
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

BLOCK = (2, 16, 8, 128)  # K+V, 16 tokens, 8 kv heads, head dim 128, fp16 = 64 KiB


def timeit(fn, warmup, reps):
    for _ in range(warmup):
        fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def case(label, n_daemons, n_swap, compress, warmup, reps):
    rng = random.Random(0)
    n_gpu_blocks, n_pool_blocks = n_swap, 2 * n_swap
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            kv = PagedKVOffload(c, n_gpu_blocks, n_pool_blocks, BLOCK, compress=compress)
            kv.gpu_cache.normal_()
            pairs = list(zip(rng.sample(range(n_gpu_blocks), n_swap), rng.sample(range(n_pool_blocks), n_swap)))
            out_np = np.array(pairs, dtype=np.int64)
            in_np = out_np[:, ::-1].copy()
            n_ops = kv.swap_out(out_np, async_=False)
            out = timeit(lambda: kv.swap_out(out_np, async_=True), warmup, reps)
            inn = timeit(lambda: kv.swap_in(in_np, async_=True), warmup, reps)
            tiers = sorted({e["tier"] for e in kv.alloc.remote_info()["extents"]})
            src = n_swap * kv.block_bytes
            wire = n_swap * (api.quant_bytes(kv.block_elems) if compress else kv.block_bytes)
            kv.close()
    row = {"case": label, "compress": compress or "none", "blocks": n_swap, "block_KiB": kv.block_bytes >> 10,
           "ops_per_swap": n_ops, "pool_tiers": tiers, "source_bytes": src, "wire_bytes": wire,
           "swap_out_us": round(out[0] * 1e6, 1), "swap_out_us_min_max": [round(out[1] * 1e6, 1), round(out[2] * 1e6, 1)],
           "swap_in_us": round(inn[0] * 1e6, 1), "swap_in_us_min_max": [round(inn[1] * 1e6, 1), round(inn[2] * 1e6, 1)],
           "swap_out_source_GiBps": round(src / out[0] / 2**30, 1), "swap_in_source_GiBps": round(src / inn[0] / 2**30, 1),
           "warmup": warmup, "reps": reps}
    print(json.dumps(row), flush=True)
    return row


def compare(label, n_daemons, n_swap, fmt, warmup, reps):
    """plain, MXFP8 and `fmt` pools in one process, their swaps alternating."""
    rng = random.Random(0)
    modes = {"none": None, "mxfp8": "mxfp8", fmt: fmt}
    pairs = list(zip(rng.sample(range(n_swap), n_swap), rng.sample(range(2 * n_swap), n_swap)))
    out_np = np.array(pairs, dtype=np.int64)
    in_np = out_np[:, ::-1].copy()
    row = {"case": label, "blocks": n_swap, "warmup": warmup, "reps": reps, "alternating": list(modes)}
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            kvs = {k: PagedKVOffload(c, n_swap, 2 * n_swap, BLOCK, compress=v) for k, v in modes.items()}
            for kv in kvs.values():
                kv.gpu_cache.normal_()
                kv.swap_out(out_np, async_=False)
            row["block_KiB"] = kvs["none"].block_bytes >> 10
            row["pool_tiers"] = sorted({e["tier"] for kv in kvs.values() for e in kv.alloc.remote_info()["extents"]})
            for direction, fn_of in (("swap_out", lambda kv: (lambda: kv.swap_out(out_np, async_=True))),
                                     ("swap_in", lambda kv: (lambda: kv.swap_in(in_np, async_=True)))):
                fns = {k: fn_of(kv) for k, kv in kvs.items()}
                samples = {k: [] for k in fns}
                for i in range(warmup + reps):  # the modes alternate
                    for k, fn in fns.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        if i >= warmup:
                            samples[k].append(time.perf_counter() - t0)
                for k, ts in samples.items():
                    ts.sort()
                    row[f"{direction}_us_{k}"] = round(ts[len(ts) // 2] * 1e6, 1)
                    row[f"{direction}_us_min_max_{k}"] = [round(ts[0] * 1e6, 1), round(ts[-1] * 1e6, 1)]
                row[f"{direction}_{fmt}_over_none"] = round(row[f"{direction}_us_{fmt}"] / row[f"{direction}_us_none"], 3)
                row[f"{direction}_{fmt}_over_mxfp8"] = round(row[f"{direction}_us_{fmt}"] / row[f"{direction}_us_mxfp8"], 3)
                row[f"{direction}_mxfp8_over_none"] = round(row[f"{direction}_us_mxfp8"] / row[f"{direction}_us_none"], 3)
            src = n_swap * kvs["none"].block_bytes
            row["source_bytes"] = src
            for k, v in modes.items():
                row[f"wire_bytes_{k}"] = n_swap * api.quant_bytes(kvs[k].block_elems, v) if v else src
            row["bytes_ratio_over_none"] = round(row[f"wire_bytes_{fmt}"] / src, 3)
            row["bytes_ratio_over_mxfp8"] = round(row[f"wire_bytes_{fmt}"] / row["wire_bytes_mxfp8"], 3)
            for kv in kvs.values():
                kv.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--compress", choices=["none", "mxfp8"], default="none")
    ap.add_argument("--format", choices=["mxfp4"], default=None,
                    help="compare this record format with the plain and the MXFP8 swap in one process (--compress is then unused)")
    ap.add_argument("--blocks", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (4 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    compress = None if args.compress == "none" else args.compress
    if args.format:
        rows = [compare("host_tier_pool", 1, n, args.format, args.warmup, args.reps) for n in args.blocks]
        if args.hbm:
            rows += [compare("same_gpu_hbm_stand_in_striped3", 4, n, args.format, args.warmup, args.reps) for n in args.blocks[:1]]
    else:
        rows = [case("host_tier_pool", 1, n, compress, args.warmup, args.reps) for n in args.blocks]
        if args.hbm:
            rows += [case("same_gpu_hbm_stand_in_striped3", 4, n, compress, args.warmup, args.reps) for n in args.blocks[:1]]
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
