"""An embedding table in remote memory, looked up by id (oncilla_amd.models.RemoteEmbedding).

    python examples/embedding_offload.py            # CPU-only daemons: the host path (works anywhere)
    python examples/embedding_offload.py --gpu 0    # daemons and the app on MI355X #0: one kernel per lookup

1. start a 3-daemon mesh; 2. load a random table into a remote half striped over the two
peers; 3. look rows up by id, with repeats, each lookup ONE indexed get whose ids stay
where they are (on the GPU with --gpu), and check them against torch.index_select;
4. scatter new rows into the table and read them back; 5. an id outside the table is
skipped, counted and reported.

    python examples/embedding_offload.py --compress mxfp8     # or mxfp4; with or without --gpu

keeps the table as MX records, one per row (RemoteEmbedding(compress=...)): each lookup ONE indexed
converting get, checked against the oracle round trip (decode of encode) of torch.index_select, and
the table's remote bytes printed against the uncompressed size.

    python examples/embedding_offload.py --gpu 0 --train

trains a second, fp32 table where it lives (oncilla_amd.models.RemoteEmbeddingAdam): a few steps of
a toy regression on looked-up rows, each step ONE fused row-sparse Adam launch, checked against a
dense torch replay of the same rule on the CPU. The fused step is a GPU kernel: without --gpu the
library refuses it ("needs a GPU") and --train reports that instead of training some other way.

    python examples/embedding_offload.py --bags 256           # with or without --gpu

pools bags of ids as nn.EmbeddingBag does (RemoteEmbedding.lookup_bags): sum, weighted sum and mean,
each ONE fused gather-reduce that writes bags x dim sums and no looked-up row, checked against
torch.nn.functional.embedding_bag within the bound that two summation orders can differ by.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oncilla_amd import api  # noqa: E402
from oncilla_amd.models import RemoteEmbedding, RemoteEmbeddingAdam  # noqa: E402
from oncilla_amd.ops import (mx4_decode_reference, mx4_encode_reference, mx8_decode_reference,  # noqa: E402
                             mx8_encode_reference)
from oncilla_amd.parallel import Mesh  # noqa: E402


def train(c, kind, dev, rows, dim, g, steps=5, batch=1024):
    """Pull looked-up rows towards target rows: loss = 0.5 * |emb[ids] - target[ids]|^2 summed, so the
    gradient of a looked-up row is the difference, and ids drawn twice add up."""
    import math

    emb = RemoteEmbedding(c, rows, dim, torch.float32, max_ids=batch, kind=kind, stripe_unit=1 << 16)
    table = torch.randn((rows, dim), generator=g)
    target = torch.randn((rows, dim), generator=g)
    emb.load(table.to(dev))
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    opt = RemoteEmbeddingAdam(emb, lr=lr, betas=(b1, b2), eps=eps)
    m, v = torch.zeros_like(table), torch.zeros_like(table)
    touched = torch.zeros(rows, dtype=torch.bool)
    for t in range(1, steps + 1):
        ids = torch.randint(0, rows, (batch,), generator=g)
        looked = emb.lookup(ids.to(dev))  # sees the step before: no sync in between
        grad = looked - target[ids].to(dev)
        try:
            opt.step(ids.to(dev), grad)
        except api.OcmError as e:
            print(f"--train: the fused row-sparse step did not run: {e}")
            opt.close()
            emb.close()
            return False
        # the dense replay on the CPU: the same rule, the global step in the bias corrections
        uniq, inv = torch.unique(ids, return_inverse=True)
        gsum = torch.zeros(len(uniq), dim).index_add_(0, inv, table[ids] - target[ids])
        m[uniq] = m[uniq] + (1 - b1) * (gsum - m[uniq])
        v[uniq] = b2 * v[uniq] + (1 - b2) * gsum * gsum
        denom = v[uniq].sqrt() * (1 / math.sqrt(1 - b2 ** t)) + eps
        table[uniq] = table[uniq] - lr / (1 - b1 ** t) * (m[uniq] / denom)
        touched[uniq] = True
    for r in range(0, rows, batch):
        ids = torch.arange(r, min(r + batch, rows))
        got = emb.lookup(ids.to(dev), async_=False).cpu()
        same = ~touched[ids]
        assert torch.equal(got[same], table[ids][same]), "a row that was never picked changed"
        assert torch.allclose(got, table[ids], rtol=1e-4, atol=1e-5), "the trained table left the replay"
    assert opt.skipped() == 0
    print(f"--train: {steps} fused row-sparse Adam steps on a {rows} x {dim} fp32 table in remote memory "
          f"({int(touched.sum())} rows touched) equal the dense replay")
    opt.close()
    emb.close()
    return True


def pooled(c, kind, dev, rows, dim, g, n_bags):
    """nn.EmbeddingBag's forward over a float32 table in remote memory: n_bags bags of 0 to 40 ids, ONE
    pooled lookup per call (RemoteEmbedding.lookup_bags), checked against torch's embedding_bag.

    The tolerance, per element of a bag of n entries, with u = 2^-24 and t_i the n terms. Both sides add the
    same terms in different orders. In any order a term passes through at most n - 1 additions, each within a
    factor 1 +- u, so a computed sum is within (n - 1) * u * sum|t_i| of the exact one and two computed sums
    are within 2 * (n - 1) * u * sum|t_i| of each other. A weighted term is fl(w * x) here, two roundings, and
    may be fused on torch's side: at most one more u on each term, (2 * n - 1) * u in all. Both are within
        n * 2^-23 * sum|t_i|,
    the bound for the sum and the weighted sum. The mean is that sum divided by n, once, on either side (torch
    divides as well: its mean equals its sum / n bit for bit): the sums' bound divided by n, plus one rounding
    of the quotient on each side, u * (|ours| + |torch's|). sum|t_i| is formed in float64, so that its own
    rounding does not loosen or tighten the bound."""
    emb = RemoteEmbedding(c, rows, dim, torch.float32, max_ids=40 * n_bags, kind=kind, stripe_unit=1 << 16, max_bags=n_bags)
    table = torch.randn((rows, dim), generator=g)
    emb.load(table.to(dev))
    lens = torch.randint(0, 41, (n_bags,), generator=g)
    offsets = torch.cumsum(lens, 0) - lens
    ids = torch.randint(0, rows, (int(lens.sum()),), generator=g)
    w = torch.randn(ids.shape, generator=g)
    bag_of_id = torch.repeat_interleave(torch.arange(n_bags), lens)
    n = lens.double().unsqueeze(1)
    for weights, mode in ((None, "sum"), (w, "sum"), (None, "mean")):
        got = emb.lookup_bags(ids.to(dev), offsets.to(dev), None if weights is None else weights.to(dev), mode=mode)
        emb.wait()
        got = got.cpu().double()
        ref = torch.nn.functional.embedding_bag(ids, table, offsets, mode=mode, per_sample_weights=weights).double()
        terms = table[ids].double() if weights is None else table[ids].double() * weights.double().unsqueeze(1)
        mag = torch.zeros(n_bags, dim, dtype=torch.float64).index_add_(0, bag_of_id, terms.abs())  # sum |t_i| per bag element
        bound = n * 2.0 ** -23 * mag
        if mode == "mean":
            bound = bound / n.clamp(min=1) + 2.0 ** -24 * (got.abs() + ref.abs())
        assert bool(((got - ref).abs() <= bound).all()), f"the pooled lookup ({mode}) left torch's embedding_bag"
    print(f"--bags: {n_bags} bags ({len(ids)} ids) of a {rows} x {dim} fp32 table in remote memory, one pooled lookup each for "
          f"sum, weighted sum and mean: equal to embedding_bag within the summation-order bound;", api.bag_counters())
    emb.close()


def roundtrip(rows, fmt):
    """What a compressed table gives back for `rows`: the oracle decode of their oracle encode (no format: the rows)."""
    if fmt is None:
        return rows
    enc, dec = {"mxfp8": (mx8_encode_reference, mx8_decode_reference), "mxfp4": (mx4_encode_reference, mx4_decode_reference)}[fmt]
    codes, scales = enc(rows.reshape(-1))
    return dec(codes, scales, rows.dtype).view(rows.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=None)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--compress", choices=["mxfp8", "mxfp4"], default=None, help="keep the table as MX records, one per row")
    ap.add_argument("--train", action="store_true", help="also train a table in place with the fused row-sparse Adam")
    ap.add_argument("--bags", type=int, default=0, metavar="N", help="also pool N bags of ids with one fused gather-reduce per call")
    args = ap.parse_args()
    if args.gpu is None:
        os.environ["OCM_NO_GPU"] = "1"
    gpus = [args.gpu] * 3 if args.gpu is not None else None
    kind = api.OCM_REMOTE_GPU if args.gpu is not None else api.OCM_REMOTE_RDMA
    dev = f"cuda:{args.gpu}" if args.gpu is not None else "cpu"
    g = torch.Generator().manual_seed(0)
    with Mesh(3, gpus=gpus, policy="stripe") as mesh:
        with api.Client(daemon_rank=0, gpu=args.gpu, ns=mesh.ns) as c:
            emb = RemoteEmbedding(c, args.rows, args.dim, torch.float16, max_ids=2048, kind=kind, stripe_unit=1 << 16,
                                  compress=args.compress)
            table = torch.randn((args.rows, args.dim), generator=g).to(torch.float16)
            emb.load(table.to(dev))
            table = roundtrip(table, args.compress)  # what the remote half now holds, decoded
            for dtype in (torch.int64, torch.int32):
                ids = torch.randint(0, args.rows, (2048,), generator=g).to(dtype)
                ids[100:110] = ids[0]  # repeats are fine on the side being read
                rows = emb.lookup(ids.to(dev))
                emb.wait()
                assert torch.equal(rows.cpu(), torch.index_select(table, 0, ids.long()))
            # scatter: unique ids
            ids = torch.randperm(args.rows, generator=g)[:512]
            new = torch.randn((512, args.dim), generator=g).to(torch.float16)
            emb.update(ids.to(dev), new.to(dev))
            new = roundtrip(new, args.compress)
            table[ids] = new
            assert torch.equal(emb.lookup(ids.to(dev), async_=False).cpu(), new)
            # an id outside the table moves nothing and is reported
            bad = torch.tensor([3, args.rows, 5, -1])
            try:
                emb.lookup(bad.to(dev), async_=False)
                raise SystemExit("an id outside the table went unreported")
            except IndexError as e:
                print("out of range:", e)
            assert torch.equal(emb.out[[0, 2]].cpu(), table[[3, 5]])
            if args.compress:
                plain = args.rows * emb.row_bytes
                print(f"{args.rows} x {args.dim} fp16 table in remote memory as {args.compress} records: lookups equal the "
                      f"{args.compress} round trip of index_select; remote bytes {emb.remote_bytes} against {plain} "
                      f"uncompressed ({emb.remote_bytes / plain:.3f});", api.quant_indexed_counters(),
                      {"n_indexed_skipped": api.indexed_counters()["n_indexed_skipped"]})
            else:
                print(f"{args.rows} x {args.dim} fp16 table in remote memory: lookups equal index_select;",
                      {k: v for k, v in api.indexed_counters().items()})
            emb.close()
            if args.train:
                train(c, kind, dev, args.rows, args.dim, g)
            if args.bags:
                pooled(c, kind, dev, args.rows, args.dim, g, args.bags)


if __name__ == "__main__":
    main()
