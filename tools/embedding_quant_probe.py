"""Lookup of random rows of an embedding table kept as MX records in remote memory, the ids on
the GPU:

  (a) one indexed converting get (Allocation.quant_indexed_batch), for MXFP8 and for MXFP4;
  (b) the plain indexed get (Allocation.indexed_batch) of the same rows from an uncompressed table
      of the same shape: existing code, and the baseline for the byte saving;
  (c) what a caller does for compressed rows without (a): the ids copied to the host, one
      ocm_quant_params per row, one Allocation.quant_batch.

    python tools/embedding_quant_probe.py --hbm --out out/embedding_quant_probe.json

One process. Per shape the ways alternate, `--reps` timed runs each after `--warmup` runs. A run
starts with the ids in device memory and ends when Allocation.wait() returns: `host_us` is the time
before the launch returns, `total_us` the whole call, `copy_us` their difference. Reported per
shape and format: (a) / (b) of the whole call next to the byte ratio of the padded records (record
stride over 2 * dim), and whether (a) lies below the whole min-max range of (c).
Tables: the pinned host tier (1 daemon) and, labelled as a stand-in, HBM of the same GPU striped
over three daemons (--hbm; an xGMI figure would be a bound, not a measurement).
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
FORMATS = ("mxfp8", "mxfp4")
DTYPE = torch.float16


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


class Table:
    """A pair whose remote half holds TABLE_ROWS rows at `stride` bytes (records of `fmt`, or 16-bit rows
    for fmt None) and whose local half holds n_ids output rows and the ids; filled with random rows."""

    def __init__(self, c, n_ids, dim, fmt, ids):
        self.fmt, self.dim, self.n_ids = fmt, dim, n_ids
        self.row_bytes = 2 * dim
        self.stride = self.row_bytes if fmt is None else (api.quant_bytes(dim, fmt) + 31) // 32 * 32
        self.out_bytes = n_ids * self.row_bytes
        self.ids_off = (self.out_bytes + 15) // 16 * 16
        self.a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=self.ids_off + 8 * n_ids, remote_bytes=TABLE_ROWS * self.stride,
                         flags=api.OCM_ALLOC_STRIPE)
        self.tiers = sorted({e["tier"] for e in self.a.remote_info()["extents"]})
        self.raw = self.a.local_tensor(torch.uint8)
        self.ids_dev = self.raw[self.ids_off: self.ids_off + 8 * n_ids].view(torch.int64)
        out = self.raw[:self.out_bytes].view(DTYPE).view(n_ids, dim)
        out.copy_(torch.randn((n_ids, dim), generator=torch.Generator().manual_seed(dim)).to(DTYPE))
        torch.cuda.synchronize()
        for r in range(0, TABLE_ROWS, n_ids):  # the same chunk of random rows all over the table
            n = min(n_ids, TABLE_ROWS - r)
            if fmt is None:
                self.a.put(0, r * self.stride, n * self.row_bytes)
            else:
                self.a.quant_strided_batch([[1, 0, r * self.stride, dim, n, self.row_bytes, self.stride]], DTYPE, format=fmt)
        self.ids_dev.copy_(ids)
        torch.cuda.synchronize()

    def rows(self):
        return self.raw[:self.out_bytes].clone()


def case(label, n_daemons, n_ids, dim, warmup, reps):
    ids = torch.randint(0, TABLE_ROWS, (n_ids,), generator=torch.Generator().manual_seed(n_ids))
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            plain = Table(c, n_ids, dim, None, ids)
            quant = {fmt: Table(c, n_ids, dim, fmt, ids) for fmt in FORMATS}
            rb = plain.row_bytes
            plain_ops = api.indexed_ops([[0, 0, 0, rb, n_ids, rb, rb, api.OCM_INDEX_NONE, plain.ids_off, n_ids, TABLE_ROWS]],
                                        api.OCM_INDEX_I64)
            lo = np.arange(n_ids, dtype=np.int64) * rb
            ways = {"b_indexed_plain": (plain, lambda: plain.a.indexed_batch(plain_ops, async_=True))}
            for fmt, t in quant.items():
                qops = api.quant_indexed_ops([[0, 0, 0, dim, n_ids, rb, t.stride, api.OCM_INDEX_NONE, t.ids_off, n_ids, TABLE_ROWS]],
                                             DTYPE, api.OCM_INDEX_I64, fmt)

                def a_way(t=t, qops=qops):
                    t.a.quant_indexed_batch(qops, async_=True)

                def c_way(t=t, fmt=fmt):
                    got = t.ids_dev.cpu().numpy()  # the sync a caller pays today
                    ops = np.stack([np.zeros_like(got), lo, got * t.stride, np.full_like(got, dim)], axis=1)
                    t.a.quant_batch(api.quant_ops(ops, DTYPE, fmt), async_=True)

                ways[f"a_quant_indexed_{fmt}"] = (t, a_way)
                ways[f"c_ids_to_host_quant_{fmt}"] = (t, c_way)
            # (a) and (c) bring the same rows
            for fmt, t in quant.items():
                got = []
                for name in (f"a_quant_indexed_{fmt}", f"c_ids_to_host_quant_{fmt}"):
                    t.raw[:t.out_bytes].zero_()
                    torch.cuda.synchronize()
                    ways[name][1]()
                    t.a.wait()
                    got.append(t.rows())
                assert torch.equal(got[0], got[1]), f"{fmt}: the indexed converting get and the list of rows disagree"
            samples = {k: [] for k in ways}
            for i in range(warmup + reps):  # the ways alternate
                for k, (t, fn) in ways.items():
                    s = one(fn, t.a)
                    if i >= warmup:
                        samples[k].append(s)
            row = {"case": label, "ids": n_ids, "dim": dim, "dtype": "float16", "table_rows": TABLE_ROWS, "pool_tiers": plain.tiers,
                   "warmup": warmup, "reps": reps, "row_bytes": rb,
                   "b_indexed_plain": {"descriptors": 1, "remote_stride": rb, **stats(samples["b_indexed_plain"])}}
            b_total = row["b_indexed_plain"]["total_us"]
            row["b_GiBps_of_rows"] = round(n_ids * rb / b_total * 1e6 / 2**30, 2)
            for fmt, t in quant.items():
                a_s, c_s = stats(samples[f"a_quant_indexed_{fmt}"]), stats(samples[f"c_ids_to_host_quant_{fmt}"])
                row[f"a_quant_indexed_{fmt}"] = {"descriptors": 1, "record_stride": t.stride, **a_s}
                row[f"c_ids_to_host_quant_{fmt}"] = {"descriptors": n_ids, **c_s}
                lo_c, hi_c = c_s["total_us_min_max"]
                row[f"{fmt}_a_over_b"] = round(a_s["total_us"] / b_total, 3)
                row[f"{fmt}_byte_ratio_padded"] = round(t.stride / rb, 3)
                row[f"{fmt}_a_vs_c_total_span"] = "below" if a_s["total_us_min_max"][1] < lo_c else \
                    "median below" if a_s["total_us"] < lo_c else "inside" if a_s["total_us"] <= hi_c else "above"
            print(json.dumps(row), flush=True)
            for t in (plain, *quant.values()):
                t.a.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--dim", type=int, nargs="+", default=[64, 2048])
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (4 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for label, n_daemons in [("host_tier_table", 1)] + ([("same_gpu_hbm_stand_in_striped3", 4)] if args.hbm else []):
        for dim in args.dim:
            for n in args.ids:
                rows.append(case(label, n_daemons, n, dim, args.warmup, args.reps))
                if args.out:  # after every case: a run that is cut short keeps what it measured
                    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
                    with open(args.out, "w") as f:
                        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
