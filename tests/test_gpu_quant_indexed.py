"""Indexed converting ops on the gfx950 kernel path (csrc/src/kernels/xfer_quant_indexed.hip): every
byte of both halves against the model (quant_indexed_cases), with the pool in the pinned host tier
(one daemon) and striped over three owners (four daemons, a 4 KiB stripe unit), both record formats,
both element types, and int32 and int64 index arrays."""
import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import RemoteEmbedding
from quant_cases import random_elems, read_local
from quant_indexed_cases import (DTYPES, FORMAT_NAMES, ROW_ELEMS, UNIT, Layout, edge_layouts, embedding_reference, mixed_layout,
                                 nominal, record_bytes, record_up32, run_layout, table_reference)
from quant_strided_cases import load_pair
from strided_cases import SENTINEL, remote_bytes_of

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM
ITYPES = [api.OCM_INDEX_I32, api.OCM_INDEX_I64]
INLINE_OPS = 45  # kQuantIndexedInlineOps: the most ops the kernel arguments hold


def _client(mesh_factory, n_daemons):
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _pair(c, local_bytes, remote_bytes, n_daemons):
    assert local_bytes <= 1 << 20 and remote_bytes <= 1 << 20
    a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                stripe_unit=UNIT)
    assert len(a.remote_info()["extents"]) == (1 if n_daemons == 1 else 3)
    return a


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMAT_NAMES)
@pytest.mark.parametrize("rows", [1, 2, 37])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_edge_rows(mesh_factory, n_daemons, rows, fmt, dtype, itype):
    # per row size: gathers with a permutation, duplicates, one row repeated and a reversed order, a scatter,
    # both indices at once, local-index-only puts and gets; strides dense and padded (local + 16, remote + 32 and + 96)
    pads = ((0, 0), (16, 32), (16, 96), (0, 32))
    with _client(mesh_factory, n_daemons) as c:
        for n, re in enumerate(ROW_ELEMS):
            lpad, rpad = pads[(n + rows + itype) % 4]
            for lay in edge_layouts(itype, fmt, re, rows, lpad, rpad):
                a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
                skipped, err, _ = run_layout(a, lay, dtype, seed=re + rows)
                assert skipped == 0 and err is None, err
                a.free()


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMAT_NAMES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_records_across_stripe_units(mesh_factory, n_daemons, fmt, dtype, itype):
    # remote strides that are no multiple of the 4 KiB unit (1024-element records at their size + 32, and
    # 4128-element rows): picked records start mid-unit on every owner, and some codes and some scale bytes
    # lie on two units. The tables start 32 bytes into the half; the rows picked are those whose codes or scale
    # bytes straddle a unit boundary (found here from the geometry), among others.
    tr = 60
    starts = []  # (first byte of a picked record, its code bytes, its scale bytes)
    with _client(mesh_factory, n_daemons) as c:
        for re in (1024, 4128):
            rs = record_up32(re, fmt) + 32
            assert rs % UNIT and rs * tr + 4096 <= 1 << 20
            ncodes, nscales = record_bytes(re, fmt) - re // 32, re // 32
            first = [32 + r * rs for r in range(tr)]
            codes2 = [r for r in range(tr) if first[r] // UNIT != (first[r] + ncodes - 1) // UNIT]
            scales2 = [r for r in range(tr) if (first[r] + ncodes) // UNIT != (first[r] + ncodes + nscales - 1) // UNIT]
            assert codes2 and (scales2 or re == 1024), (re, fmt)  # 32 scale bytes on a 32-byte boundary never straddle
            picked = (scales2[:2] + codes2[:2] + [0, tr - 1, 7])[:5]
            picked = list(dict.fromkeys(picked))  # destinations stay duplicate-free
            for put in (0, 1):
                lay = Layout(itype)
                o = lay.op(put, fmt, re, None, picked, len(picked), tr, 16, 32)
                assert o[2] == 32 and o[6] == rs
                starts += [(o[2] + r * rs, ncodes, nscales) for r in picked]
                a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
                skipped, err, _ = run_layout(a, lay, dtype, seed=re + put)
                assert skipped == 0 and err is None, err
                a.free()
    assert all(s % UNIT for s, _, _ in starts)                                           # every picked record starts mid-unit
    assert len({s // UNIT % 3 for s, _, _ in starts}) == 3                              # ... on every owner
    assert sum(s // UNIT != (s + nc - 1) // UNIT for s, nc, _ in starts) >= 4            # codes on two units
    assert sum((s + nc) // UNIT != (s + nc + ns - 1) // UNIT for s, nc, ns in starts) >= 2  # scale bytes on two units


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("n_ops", [INLINE_OPS, INLINE_OPS + 1, 60])  # the most the kernel arguments hold, one more, a long list
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_lists_and_counters(mesh_factory, n_daemons, n_ops, async_):
    # both formats, both directions, empty ops first, last and adjacent in the middle; past INLINE_OPS the
    # descriptors and the wave table are uploaded
    itype = ITYPES[(n_ops + async_) % 2]
    dtype = DTYPES[(n_ops // 2 + async_) % 2]
    lay = mixed_layout(itype, n_ops, seed=n_ops)
    assert not lay.ops[0][4] and not (lay.ops[-1][3] and lay.ops[-1][4])
    assert all(not (lay.ops[i][3] and lay.ops[i][4]) for i in (n_ops // 2, n_ops // 2 + 1))
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
        before, before_idx, before_all = api.quant_indexed_counters(), api.indexed_counters(), api.counters()
        skipped, err, _ = run_layout(a, lay, dtype, seed=n_ops, async_=async_)
        assert skipped == 0 and err is None, err
        after, after_idx, after_all = api.quant_indexed_counters(), api.indexed_counters(), api.counters()
        rows, src, wire = nominal(lay.ops, lay.formats)
        assert after["n_quant_indexed"] == before["n_quant_indexed"] + 1
        assert after["n_quant_indexed_ops"] == before["n_quant_indexed_ops"] + n_ops
        assert after["n_quant_indexed_rows"] == before["n_quant_indexed_rows"] + rows
        assert after["bytes_quant_indexed_src"] == before["bytes_quant_indexed_src"] + src
        assert after["bytes_quant_indexed_wire"] == before["bytes_quant_indexed_wire"] + wire
        # its own launch: no indexed op, no converting list, no batch (the helpers' plain puts and gets are no batches)
        assert after_idx == before_idx
        assert after_all["n_quant"] == before_all["n_quant"] and after_all["n_batch"] == before_all["n_batch"]
        a.free()


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMAT_NAMES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_out_of_range_rows_are_skipped_and_counted(mesh_factory, n_daemons, fmt, dtype, itype, async_):
    # Chosen so that even a broken check cannot leave the allocation: each table is a window of 8 rows
    # that starts 4 rows into a half of 64 rows, and the bad indices are only -4, -1, 8 and 40, so the
    # addresses they would give stay inside the pair's own halves. A broken check fails the byte comparison.
    re, half_rows = 4128, 64  # rows of three tiles: a skipped row is still counted once
    ls, rs = 2 * re, record_up32(re, fmt)
    rb = record_bytes(re, fmt)
    lidx_off = half_rows * ls
    ridx_off = lidx_off + 256
    local_bytes, remote_bytes = lidx_off + 512, half_rows * rs + 512
    bad = [-4, -1, 8, 40]
    ridx = [3, bad[0], 0, bad[2], 7, bad[3]]                # gather: bad remote ids
    both_l, both_r = [0, bad[1], 2, 3, 5], [4, 5, bad[2], 7, bad[3]]
    dt = np.int32 if itype == api.OCM_INDEX_I32 else np.int64

    def put_ids(local, off, vals):
        raw = np.frombuffer(np.asarray(vals, dtype=dt).tobytes(), dtype=np.uint8).copy()
        assert off + len(raw) <= local_bytes and max(abs(v) for v in vals) <= 40
        local[off:off + len(raw)] = raw

    # every row of both halves holds data of its own: elements on the local side, oracle records on the remote side
    xl = random_elems(half_rows * re, dtype, seed=3 + itype).view(half_rows, re)
    xr = random_elems(half_rows * re, dtype, seed=5 + itype).view(half_rows, re)
    rec_l, _ = table_reference(xl, fmt)   # what a put of local row r writes
    rec_r, back_r = table_reference(xr, fmt)  # what remote row r holds, and what a get of it gives
    local = np.full(local_bytes, SENTINEL, dtype=np.uint8)
    remote = np.full(remote_bytes, SENTINEL, dtype=np.uint8)
    local[:lidx_off] = xl.view(torch.uint8).numpy().reshape(-1)
    for r in range(half_rows):
        remote[r * rs: r * rs + rb] = rec_r[r]
    put_ids(local, lidx_off, both_l)
    put_ids(local, ridx_off, both_r)
    put_ids(local, ridx_off + 64, ridx)
    # the windows: rows 4..11 of either half; the second op's, rows 20..27. A gather into rows in order cannot be
    # a window on the local side (no index: rows 0..5 of the table), so its table starts at the window too
    ops = [[0, 4 * ls, 4 * rs, re, len(ridx), ls, rs, api.OCM_INDEX_NONE, ridx_off + 64, 8, 8],
           [1, 20 * ls, 20 * rs, re, 5, ls, rs, lidx_off, ridx_off, 8, 8]]
    for o in ops:  # whatever index a broken check lets through, -4 .. 40, stays inside both halves
        for side, stride, nbytes, size in ((1, ls, 2 * re, local_bytes), (2, rs, rb, remote_bytes)):
            assert o[side] - 4 * stride >= 0 and o[side] + 40 * stride + nbytes <= size
    want_l, want_r, skipped = local.copy(), remote.copy(), 0
    for j, rr in enumerate(ridx):
        if 0 <= rr < 8:
            want_l[(4 + j) * ls: (4 + j) * ls + 2 * re] = back_r[4 + rr]
        else:
            skipped += 1
    for lr, rr in zip(both_l, both_r):
        if 0 <= lr < 8 and 0 <= rr < 8:
            want_r[(20 + rr) * rs: (20 + rr) * rs + rb] = rec_l[20 + lr]
        else:
            skipped += 1
    assert skipped == 3 + 3  # a row with one bad index of two is skipped whole
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, local_bytes, remote_bytes, n_daemons)
        load_pair(a, local, remote)
        before, before_q = api.indexed_counters(), api.quant_indexed_counters()
        with pytest.raises(api.OcmError, match=rf"indexed ops skipped {skipped} row\(s\)") as ei:
            a.quant_indexed_batch(ops, dtype, itype, async_=async_, format=fmt)
            if async_:
                a.wait()
        assert ("ocm_wait" in str(ei.value)) == async_
        after, after_q = api.indexed_counters(), api.quant_indexed_counters()
        assert after["n_indexed_skipped"] == before["n_indexed_skipped"] + skipped and after["n_indexed"] == before["n_indexed"]
        assert after_q["n_quant_indexed"] == before_q["n_quant_indexed"] + 1
        assert after_q["n_quant_indexed_rows"] == before_q["n_quant_indexed_rows"] + len(ridx) + 5
        a.wait()  # reported once
        got_l = read_local(a, 0, local_bytes).numpy()
        assert np.array_equal(got_l, want_l), np.flatnonzero(got_l != want_l)[:4]
        got_r = remote_bytes_of(a, local_bytes, remote_bytes)
        assert np.array_equal(got_r, want_r), np.flatnonzero(got_r != want_r)[:4]
        # the next op succeeds
        good = [7, 0, 7, 1, 2, 3]
        put_ids(want_l, ridx_off + 64, good)
        load_pair(a, want_l, want_r)
        a.quant_indexed_batch(ops[:1], dtype, itype, format=fmt)
        for j, rr in enumerate(good):
            want_l[(4 + j) * ls: (4 + j) * ls + 2 * re] = back_r[4 + rr]
        assert np.array_equal(read_local(a, 0, local_bytes).numpy(), want_l)
        a.free()


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_same_bytes_as_a_converting_list_of_rows(mesh_factory, n_daemons, dtype, itype):
    # by definition: the same transfer issued as quant_batch with one op per in-range row leaves both halves byte-identical
    lay = mixed_layout(itype, 24, seed=9)
    with _client(mesh_factory, n_daemons) as c:
        got = []
        for indexed in (True, False):
            a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)

            def plain(local):
                rows, formats = lay.plain_ops(local)
                a.quant_batch(api.quant_ops(rows, dtype, formats))

            skipped, err, halves = run_layout(a, lay, dtype, seed=4, run=None if indexed else plain)
            assert skipped == 0 and err is None, err
            got.append(halves)
            a.free()
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMAT_NAMES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_compressed_lookup_ordered_after_the_kernel_that_made_the_ids(mesh_factory, n_daemons, fmt, dtype, ids_dtype):
    g = torch.Generator().manual_seed(5)
    rows, dim = 2000, 160
    with _client(mesh_factory, n_daemons) as c:
        emb = RemoteEmbedding(c, rows, dim, dtype, max_ids=1500, stripe_unit=UNIT, compress=fmt)
        assert emb.record_stride == record_up32(dim, fmt) and emb.remote_bytes == rows * emb.record_stride
        assert emb.alloc.local_bytes <= 1 << 20 and emb.alloc.remote_size() == emb.remote_bytes <= 1 << 20 and emb.out.is_cuda
        table = torch.randn((rows, dim), generator=g).to(dtype)
        emb.load(table.cuda())
        want = embedding_reference(table, fmt)  # a host copy of what the table decodes to
        side = torch.cuda.Stream()
        before = api.quant_indexed_counters()
        with torch.cuda.stream(side):
            for _ in range(2):
                ids = torch.randint(0, rows, (1500,), device="cuda", dtype=ids_dtype)  # made by a kernel on `side`
                looked = emb.lookup(ids)          # async, no host sync in between
                got = looked.clone()              # read by torch on `side`
                side.synchronize()
                assert torch.equal(got.cpu().view(torch.int16), torch.index_select(want, 0, ids.cpu().long()).view(torch.int16))
            # scatter put of rows made on the stream, then looked up again
            uniq = torch.randperm(rows, device="cuda")[:700].to(ids_dtype)
            new = torch.randn((700, dim), device="cuda").to(dtype)
            emb.update(uniq, new, async_=True)
            back = emb.lookup(uniq).clone()
            side.synchronize()
            assert torch.equal(back.cpu().view(torch.int16), embedding_reference(new.cpu(), fmt).view(torch.int16))
            after = api.quant_indexed_counters()
            assert after["n_quant_indexed"] == before["n_quant_indexed"] + 4  # each lookup and the update ONE call
            # an id outside the table: nothing known at the call, IndexError at wait()
            emb.lookup(torch.tensor([1, rows, 3], device="cuda", dtype=ids_dtype))
            with pytest.raises(IndexError, match=r"skipped 1 row\(s\)"):
                emb.wait()
        emb.wait()
        emb.close()
