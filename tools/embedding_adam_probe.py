"""One Adam step on k rows of an embedding table that lives in remote memory, two ways:

  fused      one ocm_x_adam_rows launch (Allocation.adam_rows): the rows, exp_avg and
             exp_avg_sq are read and written where they live;
  get_put    what a caller does without it, built from calls that existed before: three
             indexed gets (rows, exp_avg rows, exp_avg_sq rows) into staging regions of the
             local halves, a torch fp32 update of the staged rows on the GPU, three indexed
             puts.

    python tools/embedding_adam_probe.py --hbm --out out/embedding_adam_probe.json

Per case the two ways alternate, `--reps` timed runs each after `--warmup`; a run starts with
the unique ids and the k x dim gradient in device memory and ends when
torch.cuda.synchronize() and the allocations' wait() have returned (issue to synchronise).
The median and the whole range of both are reported. Tables: the pinned host tier (2 daemons)
and, labelled as a stand-in, HBM of the same GPU (2 daemons on GPU 0); over xGMI: unmeasured.
RemoteEmbeddingAdam.step adds torch.unique and index_add_ in front of the fused launch; the
ids here are unique already and neither way pays for that.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oncilla_amd import api  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402

TABLE_ROWS = 1 << 17
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def hp_of(t):
    return (B1, B2, EPS, 0.0, LR / (1 - B1 ** t), 1 / math.sqrt(1 - B2 ** t))


def spread(vals):
    v = sorted(vals)
    return {"median_us": round(v[len(v) // 2], 1), "min_max_us": [round(v[0], 1), round(v[-1], 1)]}


def case(label, n_daemons, host, k, dim, warmup, reps):
    rb = 4 * dim
    stage = (k * rb + 15) // 16 * 16
    flags = api.OCM_ALLOC_HOST_TIER if host else 0
    with Mesh(n_daemons, gpus=[0] * n_daemons) as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            # table pair: one staging region and the ids; state pair: two staging regions and the ids
            ta = c.alloc(api.OCM_REMOTE_GPU, local_bytes=stage + 8 * k, remote_bytes=TABLE_ROWS * rb, flags=flags)
            sa = c.alloc(api.OCM_REMOTE_GPU, local_bytes=2 * stage + 8 * k, remote_bytes=2 * TABLE_ROWS * rb, flags=flags)
            tiers = sorted({e["tier"] for a in (ta, sa) for e in a.remote_info()["extents"]})
            m_off, v_off = 0, TABLE_ROWS * rb
            traw, sraw = ta.local_tensor(torch.uint8), sa.local_tensor(torch.uint8)
            w_st = traw[:k * rb].view(torch.float32).view(k, dim)
            m_st = sraw[:k * rb].view(torch.float32).view(k, dim)
            v_st = sraw[stage:stage + k * rb].view(torch.float32).view(k, dim)
            gen = torch.Generator().manual_seed(k + dim)
            ids = torch.randperm(TABLE_ROWS, generator=gen)[:k].to("cuda:0")
            traw[stage:stage + 8 * k].view(torch.int64).copy_(ids)
            sraw[2 * stage:2 * stage + 8 * k].view(torch.int64).copy_(ids)
            g = (torch.randn(k, dim, generator=gen) * 0.1).to("cuda:0")
            # the whole table and both moment tables start as zeros, chunk by chunk
            w_st.zero_()
            m_st.zero_()
            torch.cuda.synchronize()
            for r in range(0, TABLE_ROWS, k):
                n = min(k, TABLE_ROWS - r) * rb
                ta.put(0, r * rb, n)
                sa.put(0, m_off + r * rb, n)
                sa.put(0, v_off + r * rb, n)
            step = [0]

            def ops(alloc, put, lo, ro, idx_off):
                return api.indexed_ops([[put, lo, ro, rb, k, rb, rb, api.OCM_INDEX_NONE, idx_off, k, TABLE_ROWS]],
                                       api.OCM_INDEX_I64)

            gets = [(ta, ops(ta, 0, 0, 0, stage)), (sa, ops(sa, 0, 0, m_off, 2 * stage)), (sa, ops(sa, 0, stage, v_off, 2 * stage))]
            puts = [(ta, ops(ta, 1, 0, 0, stage)), (sa, ops(sa, 1, 0, m_off, 2 * stage)), (sa, ops(sa, 1, stage, v_off, 2 * stage))]

            def fused():
                step[0] += 1
                ta.adam_rows(sa, ids, g, (0, rb), (m_off, rb), (v_off, rb), hp_of(step[0]), TABLE_ROWS)

            def get_put():
                step[0] += 1
                hp = hp_of(step[0])
                for a, o in gets:
                    a.indexed_batch(o, async_=True)
                ta.stream_signal()
                sa.stream_signal()
                m_st.lerp_(g, 1 - B1)
                v_st.mul_(B2).addcmul_(g, g, value=1 - B2)
                w_st.addcdiv_(m_st, (v_st.sqrt() * hp[5]).add_(EPS), value=-hp[4])
                ta.stream_wait()
                sa.stream_wait()
                for a, o in puts:
                    a.indexed_batch(o, async_=True)

            def one(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ta.wait()
                sa.wait()
                return (time.perf_counter() - t0) * 1e6

            ways = {"fused": fused, "get_put": get_put}
            samples = {name: [] for name in ways}
            for i in range(warmup + reps):  # the two alternate
                for name, fn in ways.items():
                    us = one(fn)
                    if i >= warmup:
                        samples[name].append(us)
            # both ways ran the same rule on the same rows: the picked rows moved, and are finite
            ta.indexed_batch(gets[0][1])
            torch.cuda.synchronize()
            assert bool(torch.isfinite(w_st).all()) and bool((w_st != 0).any(dim=1).all())
            row = {"case": label, "pool_tiers": tiers, "table_rows": TABLE_ROWS, "dim": dim, "k": k, "dtype": "fp32",
                   "warmup": warmup, "reps": reps, "launches": {"fused": 1, "get_put": 6},
                   "fused": spread(samples["fused"]), "get_put": spread(samples["get_put"])}
            lo, hi = row["get_put"]["min_max_us"]
            fm = row["fused"]["median_us"]
            row["fused_vs_get_put_range"] = "below" if fm < lo else "inside" if fm <= hi else "above"
            row["fused_state_GBps"] = round(7 * k * rb / fm * 1e6 / 1e9, 2)  # 3 reads + 3 writes remote, 1 read local
            print(json.dumps(row), flush=True)
            ta.free()
            sa.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--dim", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--hbm", action="store_true", help="also the same-GPU HBM stand-in (2 daemons on GPU 0)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for label, n_daemons, host in [("host_tier_pool", 2, True)] + ([("same_gpu_hbm_stand_in", 2, False)] if args.hbm else []):
        for dim in args.dim:
            for k in args.k:
                try:
                    rows.append(case(label, n_daemons, host, k, dim, args.warmup, args.reps))
                except api.OcmError as e:  # e.g. a pool too small for the case: recorded, not hidden
                    rows.append({"case": label, "dim": dim, "k": k, "error": str(e)})
                    print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
