"""Paged KV-cache offload on an MI355X: swap KV blocks of idle sequences to a
pool in other GPUs' HBM (or the pinned host tier on a single-daemon node) and
back, each swap list being one batched launch ordered against torch's stream.

    python examples/kv_offload.py [--daemons 4] [--compress [mxfp8|mxfp4]] [--layers N]

--compress keeps the pool as MXFP8 records (33/64 of the bytes in the pool and on the
link), --compress mxfp4 as MXFP4 records (17/64); blocks then come back rounded to that format.
--layers N keeps one cache per layer, [N, blocks, ...], as serving engines do: a block is
N pieces a cache apart, and each swapped block is one strided op (rows = N).
--compress --layers N together keep one record per layer (compress="mxfp8-rows" / "mxfp4-rows"): each
swapped block is one strided converting op, and every layer comes back rounded on its own.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oncilla_amd import api  # noqa: E402
from oncilla_amd.models import PagedKVOffload  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402


def layered(args):
    with Mesh(args.daemons, gpus=[0] * args.daemons, policy="stripe") as mesh:
        with api.Client(daemon_rank=0, gpu=0, ns=mesh.ns) as c:
            # per layer: 256 GPU blocks of (K/V, 16 tokens, 8 heads, 8 dims) fp16 = 4 KiB; pool of 2048 blocks
            kv = PagedKVOffload(c, 256, 2048, (2, 16, 8, 8), dtype=torch.float16, layers=args.layers,
                                compress=args.compress + "-rows" if args.compress else None)
            kv.gpu_cache.normal_()
            before = kv.gpu_cache[:, :64].clone()
            n = kv.swap_out([(g, 1000 + g) for g in range(64)])  # 64 blocks out: one strided op each, one launch
            kv.gpu_cache[:, :64].zero_()
            kv.swap_in([(1000 + g, g) for g in range(64)])
            if args.compress:
                # a record per (layer, block): groups of 32 never span two of them
                want = oracle_roundtrip(before, args.compress)
                assert torch.equal(kv.gpu_cache[:, :64].cpu(), want)  # exactly the format's rounding, per layer
            else:
                assert torch.equal(kv.gpu_cache[:, :64], before)      # every layer of every block
            print(f"64 KV blocks x {args.layers} layers swapped out and back as {n} strided "
                  f"{'converting ' if args.compress else ''}ops; pool block: {kv.pool_block_bytes} bytes, layer-major")
            kv.close()


def oracle_roundtrip(x, fmt):
    from oncilla_amd import ops

    enc, dec = ((ops.mx4_encode_reference, ops.mx4_decode_reference) if fmt == "mxfp4" else
                (ops.mx8_encode_reference, ops.mx8_decode_reference))
    return dec(*enc(x), x.dtype).view(x.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--daemons", type=int, default=4)
    ap.add_argument("--compress", nargs="?", const="mxfp8", default=None, choices=["mxfp8", "mxfp4"],
                    help="keep the pool compressed: MXFP8 records (the default) or MXFP4 ('-rows' records with --layers)")
    ap.add_argument("--layers", type=int, default=0, help="one cache per layer: gpu_cache is [N, blocks, ...] (layers=N)")
    args = ap.parse_args()
    if args.layers:
        return layered(args)
    with Mesh(args.daemons, gpus=[0] * args.daemons, policy="stripe") as mesh:
        with api.Client(daemon_rank=0, gpu=0, ns=mesh.ns) as c:
            # 256 GPU blocks of (K/V, 16 tokens, 8 heads, 128 dims) fp16 = 64 KiB; pool of 2048 blocks
            kv = PagedKVOffload(c, 256, 2048, (2, 16, 8, 128), dtype=torch.float16,
                                compress=args.compress)
            kv.gpu_cache.normal_()
            before = kv.gpu_cache[:64].clone()
            kv.swap_out([(g, 1000 + g) for g in range(64)])     # 64 blocks out (coalesced: 1 op)
            kv.gpu_cache[:64].zero_()                            # blocks reused by other sequences
            kv.swap_in([(1000 + g, g) for g in range(64)])      # ... and back before the next step
            if args.compress:
                want = oracle_roundtrip(before, args.compress)
                assert torch.equal(kv.gpu_cache[:64].cpu(), want)  # exactly the format's rounding
                print(f"pool block: {kv.pool_block_bytes} bytes for {kv.block_bytes} of KV")
            else:
                assert torch.equal(kv.gpu_cache[:64], before)    # torch's stream waited for the copies
            print("64 KV blocks swapped out and back; pool on", sorted({e["owner_rank"] for e in kv.alloc.remote_info()["extents"]}))
            kv.close()


if __name__ == "__main__":
    main()
