"""Pooled lookup of an embedding table in remote memory, ids and offsets on the GPU, three ways:

  (a) RemoteEmbedding.lookup_bags: ONE pooled lookup (ocm_copy_onesided_bag), the bags' rows summed
      in registers on the way in;
  (b) what a caller did before it: RemoteEmbedding.lookup(ids), which writes len(ids) rows into the
      local half, then ONE torch launch on the same stream that sums them per bag:
      torch.nn.functional.embedding_bag over the looked-up rows with the ids 0 .. len(ids) - 1
      (made once outside the timed region), which accumulates in fp32 and writes the table's dtype;
  (c) the same lookup followed by the segment sum spelled out in torch ops: zeros, a float() copy of
      the rows, index_add_ by a bag index made outside the timed region, the cast back (four
      launches and an fp32 copy of the rows). Whichever of (b) and (c) is faster is the one to beat.

    python tools/bag_lookup_probe.py --hbm --out out/bag_lookup_probe.json

One process. Per case the ways alternate, `--reps` timed runs each after `--warmup` runs. A run
starts with ids and offsets in device memory and ends when torch's stream, which every way makes
wait for the copy, has drained: `total_us` is that whole time, `host_us` the time before the calls
return. Every row crosses the link either way; what (a) saves is the write and re-read of
len(ids) x dim elements of local HBM, the second launch, and an output region mean-bag-length times
larger. Tables: the pinned host tier (1 daemon) and, labelled as a stand-in, HBM of the same GPU
striped over three daemons (--hbm): a 1-GPU box measures PCIe or local HBM, not xGMI.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oncilla_amd import api  # noqa: E402
from oncilla_amd.models import RemoteEmbedding  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402


def one(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e6, (t2 - t0) * 1e6, out


def stats(samples):
    out = {}
    for name, vals in (("host_us", [s[0] for s in samples]), ("total_us", [s[1] for s in samples])):
        v = sorted(vals)
        out[name] = round(v[len(v) // 2], 1)
        out[name + "_min_max"] = [round(v[0], 1), round(v[-1], 1)]
    return out


def case(label, n_daemons, rows, dim, bags, mean_len, dtype, warmup, reps):
    g = torch.Generator().manual_seed(bags)
    lens = torch.randint(1, 2 * mean_len, (bags,), generator=g)  # mean mean_len
    offsets = (torch.cumsum(lens, 0) - lens).cuda()
    k = int(lens.sum())
    ids = torch.randint(0, rows, (k,), generator=g).cuda()
    bag_of_id = torch.repeat_interleave(torch.arange(bags), lens).cuda()
    with Mesh(n_daemons, gpus=[0] * n_daemons, policy="stripe") as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            emb = RemoteEmbedding(c, rows, dim, dtype, max_ids=k, max_bags=bags)
            tiers = sorted({e["tier"] for e in emb.alloc.remote_info()["extents"]})
            chunk = (torch.randint(-127, 128, (k, dim), generator=g).float() / 16).to(dtype).cuda()
            for r in range(0, rows, k):  # the same chunk of rows all over the table
                n = min(k, rows - r)
                emb.out[:n].copy_(chunk[:n])
                emb.alloc.stream_wait()
                emb.alloc.put(0, r * emb.row_bytes, n * emb.row_bytes)

            def fused():
                return emb.lookup_bags(ids, offsets)

            every = torch.arange(k, device="cuda")

            def composed():
                return torch.nn.functional.embedding_bag(every, emb.lookup(ids), offsets, mode="sum")

            def spelled_out():
                got = emb.lookup(ids)
                return torch.zeros((bags, dim), dtype=torch.float32, device="cuda").index_add_(0, bag_of_id, got.float()).to(dtype)

            ways = {"a_lookup_bags": fused, "b_lookup_then_segment_sum": composed, "c_lookup_then_index_add": spelled_out}
            a = one(fused)[2].float().clone()
            for other in (composed, spelled_out):
                b = one(other)[2].float()
                # torch adds in another order: the two agree to the rounding of a sum of mean_len terms
                assert torch.allclose(a, b, rtol=2.0 ** -6, atol=2.0 ** -4), float((a - b).abs().max())
            samples = {name: [] for name in ways}
            for i in range(warmup + reps):  # the ways alternate
                for name, fn in ways.items():
                    s = one(fn)
                    if i >= warmup:
                        samples[name].append(s[:2])
            row = {"case": label, "table_rows": rows, "dim": dim, "dtype": str(dtype).replace("torch.", ""), "bags": bags, "ids": k,
                   "mean_bag_len": round(k / bags, 2), "pool_tiers": tiers, "warmup": warmup, "reps": reps,
                   "row_bytes": emb.row_bytes, "bytes_over_the_link": k * emb.row_bytes}
            for name in ways:
                row[name] = stats(samples[name])
            a_t, b_t = row["a_lookup_bags"]["total_us"], row["b_lookup_then_segment_sum"]["total_us"]
            row["a_over_b_total"] = round(a_t / b_t, 3)
            row["a_over_c_total"] = round(a_t / row["c_lookup_then_index_add"]["total_us"], 3)
            row["a_GiBps_of_rows"] = round(k * emb.row_bytes / a_t * 1e6 / 2 ** 30, 2)
            row["b_GiBps_of_rows"] = round(k * emb.row_bytes / b_t * 1e6 / 2 ** 30, 2)
            lo_b = row["b_lookup_then_segment_sum"]["total_us_min_max"][0]
            hi_a = row["a_lookup_bags"]["total_us_min_max"][1]
            row["a_vs_b_total_span"] = "below" if hi_a < lo_b else "median below" if a_t < b_t else "not below"
            print(json.dumps(row), flush=True)
            emb.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--bags", type=int, default=4096)
    ap.add_argument("--mean-len", type=int, default=32)
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float16", "float32"])
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (4 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = []
    for label, n_daemons in [("host_tier_table", 1)] + ([("same_gpu_hbm_stand_in_striped3", 4)] if args.hbm else []):
        out.append(case(label, n_daemons, args.rows, args.dim, args.bags, args.mean_len, getattr(torch, args.dtype), args.warmup,
                        args.reps))
        if args.out:  # after every case: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
