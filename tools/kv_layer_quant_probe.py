"""Layer-major KV-cache block swap with MXFP8 records (PagedKVOffload layers=32,
compress="mxfp8-rows", 2 KiB fp16 rows of 1024 elements, 64 KiB per block), three forms
of the same swap:

  quant_strided     one strided converting op per block (Allocation.quant_strided_batch)
  expanded_quant    the same transfer as one plain converting op per row
                    (Allocation.quant_batch, existing code: the reference for the kernel)
  strided_copy      the uncompressed layers=32 swap (Allocation.strided_batch: the
                    reference for what compression buys)

and, for the open question of rows that fill one of a tile's two rounds, the same bytes
as converting ops of 2048 elements (whole tiles) on dense offsets: full_tiles.
--format mxfp4 runs the converting forms with MXFP4 records (compress="mxfp4-rows").

    python tools/kv_layer_quant_probe.py --hbm --out out/kv_layer_quant_probe.json

Per case and direction the forms alternate, `--reps` timed runs each after warm-up. A run
is one async call on a prepared descriptor list followed by Allocation.wait(): `host_us`
is the call itself (validation, planning, the descriptor upload and the launch: the host
time before the launch returns), `total_us` ends when the wait does. Pools: the pinned
host tier (1 daemon) and, labelled as a stand-in, HBM of the same GPU striped over three
daemons (--hbm; an xGMI figure would be a bound, not a measurement).
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

BLOCK = (2, 8, 64)  # K+V, 8 kv heads x 64 (one token slice), fp16 = 2 KiB = 1024 elements per layer
LAYERS = 32         # 64 KiB per logical block


def expand(kv, pairs, put):
    """One plain converting op per layer of each block: [op_flag, local_offset, remote_offset, elems]."""
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    g, p = (a[:, 0], a[:, 1]) if put else (a[:, 1], a[:, 0])
    layer = np.arange(kv.layers, dtype=np.int64)
    lo = (g[:, None] * kv.block_bytes + layer[None, :] * kv.num_gpu_blocks * kv.block_bytes).reshape(-1)
    ro = (p[:, None] * kv.pool_block_bytes + layer[None, :] * kv.record_bytes).reshape(-1)
    return np.stack([np.full_like(lo, 1 if put else 0), lo, ro, np.full_like(lo, kv.block_elems)], axis=1)


def full_tiles(kv, n_swap, put):
    """As many elements in converting ops of 2048 (two rows' worth, a whole tile each) on dense offsets."""
    i = np.arange(n_swap * kv.layers // 2, dtype=np.int64)
    return np.stack([np.full_like(i, 1 if put else 0), i * 4096, i * 2 * kv.record_bytes, np.full_like(i, 2048)], axis=1)


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


def case(label, n_daemons, n_swap, warmup, reps, fmt="mxfp8"):
    rng = random.Random(0)
    rows = []
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            kv = PagedKVOffload(c, n_swap, n_swap, BLOCK, layers=LAYERS, compress=fmt + "-rows")
            plain = PagedKVOffload(c, n_swap, n_swap, BLOCK, layers=LAYERS)
            kv.gpu_cache.normal_()
            plain.gpu_cache.normal_()
            torch.cuda.synchronize()
            pairs = np.array(list(zip(rng.sample(range(n_swap), n_swap), rng.sample(range(n_swap), n_swap))), dtype=np.int64)
            back = pairs[:, ::-1].copy()
            tiers = sorted({e["tier"] for e in kv.alloc.remote_info()["extents"]})
            # both converting forms compute the same bytes: out strided and back expanded gives what
            # out expanded and back strided gives
            kv.alloc.quant_strided_batch(kv._ops(pairs, put=True))
            kv.alloc.quant_batch(api.quant_ops(expand(kv, back, False), kv.dtype, fmt))
            once = kv.gpu_cache.clone()
            kv.alloc.quant_batch(api.quant_ops(expand(kv, pairs, True), kv.dtype, fmt))
            kv.alloc.quant_strided_batch(kv._ops(back, put=False))
            assert torch.equal(kv.gpu_cache.view(torch.int16), once.view(torch.int16)), "the two converting forms differ"
            del once
            for direction, put, pr in (("swap_out", True, pairs), ("swap_in", False, back)):
                lists = {"quant_strided": kv._ops(pr, put=put),
                         "expanded_quant": api.quant_ops(expand(kv, pr, put), kv.dtype, fmt),
                         "strided_copy": plain._ops(pr, put=put),
                         "full_tiles": api.quant_ops(full_tiles(kv, n_swap, put), kv.dtype, fmt)}
                ways = {"quant_strided": (kv.alloc, lambda: kv.alloc.quant_strided_batch(lists["quant_strided"], async_=True)),
                        "expanded_quant": (kv.alloc, lambda: kv.alloc.quant_batch(lists["expanded_quant"], async_=True)),
                        "strided_copy": (plain.alloc, lambda: plain.alloc.strided_batch(lists["strided_copy"], async_=True)),
                        "full_tiles": (kv.alloc, lambda: kv.alloc.quant_batch(lists["full_tiles"], async_=True))}
                samples = {k: [] for k in ways}
                for i in range(warmup + reps):  # the forms alternate
                    for k, (alloc, fn) in ways.items():
                        s = one(fn, alloc)
                        if i >= warmup:
                            samples[k].append(s)
                row = {"case": label, "direction": direction, "blocks": n_swap, "layers": LAYERS, "row_elems": kv.block_elems,
                       "pool_tiers": tiers, "source_bytes": n_swap * LAYERS * kv.block_bytes,
                       "record_bytes": n_swap * LAYERS * api.quant_bytes(kv.block_elems, fmt), "warmup": warmup, "reps": reps}
                for k in ways:
                    row[k] = {"descriptors": lists[k].n, **stats(samples[k])}
                lo, hi = row["expanded_quant"]["total_us_min_max"]
                a, b, cc = (row[k]["total_us"] for k in ("quant_strided", "expanded_quant", "strided_copy"))
                # the condition: (a) is not slower than (b) by more than the spread of (b)'s own runs
                row["expanded_quant_spread_us"] = round(hi - lo, 1)
                row["quant_strided_minus_expanded_us"] = round(a - b, 1)
                row["condition_holds"] = bool(a - b <= hi - lo)
                row["quant_strided_over_strided_copy"] = round(a / cc, 3)
                row["bytes_ratio"] = round(33 / 64, 3)
                if fmt != "mxfp8":
                    row["format"], row["bytes_ratio"] = fmt, round(17 / 64, 3)
                row["half_tiles_over_full_tiles"] = round(b / row["full_tiles"]["total_us"], 3)
                print(json.dumps(row), flush=True)
                rows.append(row)
            kv.close()
            plain.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--format", choices=["mxfp8", "mxfp4"], default="mxfp8", help="the record format of the converting forms")
    ap.add_argument("--blocks", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (4 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    cases = [("host_tier_pool", 1, n) for n in args.blocks]
    if args.hbm:
        cases += [("same_gpu_hbm_stand_in_striped3", 4, n) for n in args.blocks]
    for label, n_daemons, n in cases:
        rows += case(label, n_daemons, n, args.warmup, args.reps, args.format)
        if args.out:  # after every case: a later one that fails keeps the earlier results
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
