"""Indexed one-sided ops on the gfx950 kernel path (csrc/src/kernels/xfer_indexed.hip): every byte of
both halves against the numpy model, with the pool in the pinned host tier (one daemon) and striped
over three owners (four daemons, a 4 KiB stripe unit), and int32 and int64 index arrays."""
import numpy as np
import pytest
import torch

from indexed_cases import (ROW_BYTES, UNIT, Layout, edge_layout, exercise_indexed_kv, expand, fill_pair, mixed_layout, model,
                           nominal, read_local, remote_bytes_of, run_layout)
from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload, RemoteEmbedding

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM
ITYPES = [api.OCM_INDEX_I32, api.OCM_INDEX_I64]


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
@pytest.mark.parametrize("rows", [1, 2, 37])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_edge_rows(mesh_factory, n_daemons, rows, itype):
    # per row size: gathers with a permutation, duplicates, one row repeated and a reversed order, a scatter,
    # local-index-only ops and both indices; padded and dense strides, offsets that agree and disagree mod 16
    combos = ((True, True), (False, False), (True, False), (False, True))
    with _client(mesh_factory, n_daemons) as c:
        for n, rb in enumerate(ROW_BYTES):
            for dense, agree in (combos[n % 4], combos[(n + rows) % 4 - 2]):
                lay = edge_layout(itype, rb, rows, dense, agree)
                a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
                skipped, err = run_layout(a, lay, seed=rb + rows)
                assert skipped == 0 and err is None, err
                a.free()


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_rows_across_stripe_units(mesh_factory, n_daemons, itype):
    # remote rows 1000 bytes further apart than they are long: no stride is a multiple of the 4 KiB unit,
    # selected rows start mid-unit on every owner, and rows of 4095 bytes and more straddle two
    with _client(mesh_factory, n_daemons) as c:
        starts = []
        for rb in (17, 4095, 4097, 8195):
            lay = edge_layout(itype, rb, 5, False, True, remote_gap=1000)
            assert all(o[6] % UNIT for o in lay.ops)
            ids = dict(lay.indices)
            for o in lay.ops:
                picked = ids[o[8]] if o[8] in ids else np.arange(o[4])
                starts += [(o[2] + int(r) * o[6], rb) for r in picked]
            a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
            skipped, err = run_layout(a, lay, seed=rb)
            assert skipped == 0 and err is None, err
            a.free()
        assert all(s % UNIT for s, _ in starts)                                     # every selected row starts mid-unit
        assert sum(s // UNIT != (s + n - 1) // UNIT for s, n in starts) >= 15       # rows on two owners (or three)
        assert len({s // UNIT % 3 for s, _ in starts}) == 3                         # rows begin on every owner


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_out_of_range_rows_are_skipped_and_counted(mesh_factory, n_daemons, itype, async_):
    # Chosen so that even a broken check cannot leave the allocation: each table is a window of 8 rows
    # that starts 4 rows into a half of 64 rows, and the bad indices are only -4 .. -1 and 8 .. 40, so the
    # addresses they would give stay inside the pair's own halves. A broken check fails the byte comparison.
    rb, stride = 9000, 9008  # rows of three tiles: a skipped row is still counted once
    win, half_rows = 4 * stride, 64
    lidx_off = half_rows * stride
    ridx_off = lidx_off + 256
    local_bytes = remote_bytes = lidx_off + 512
    bad = [-4, -1, 8, 40]
    ridx = [3, bad[0], 0, bad[2], 7, bad[3]]                # gather: bad remote ids
    both_l, both_r = [0, bad[1], 2, 3, 5], [4, 5, bad[2], 7, bad[3]]
    dt = np.int32 if itype == api.OCM_INDEX_I32 else np.int64
    isz = 4 * itype

    def put_ids(a, local, off, vals):
        raw = np.frombuffer(np.asarray(vals, dtype=dt).tobytes(), dtype=np.uint8).copy()
        assert off + len(raw) <= local_bytes and max(abs(v) for v in vals) <= 40
        local[off:off + len(raw)] = raw
        a.local_tensor(torch.uint8)[off:off + len(raw)].copy_(torch.from_numpy(raw))

    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, local_bytes, remote_bytes, n_daemons)
        local, remote = fill_pair(a, local_bytes, remote_bytes, seed=itype, random_remote=True)
        put_ids(a, local, lidx_off, both_l)
        put_ids(a, local, ridx_off, both_r)
        put_ids(a, local, ridx_off + 64, ridx)
        torch.cuda.synchronize()
        # the windows: local rows 4..11 of its half, remote rows 4..11; a gather into rows in order cannot be a
        # window on the local side (no index: rows 0..5 of the table), so its table starts at the window too
        ops = [[0, win, win, rb, len(ridx), stride, stride, api.OCM_INDEX_NONE, ridx_off + 64, 8, 8],
               [1, win + 16 * stride, win + 16 * stride, rb, 5, stride, stride, lidx_off, ridx_off, 8, 8]]
        for o in ops:  # whatever index a broken check lets through, -4 .. 40, stays inside both halves
            for side, size in ((1, local_bytes), (2, remote_bytes)):
                assert o[side] - 4 * stride >= 0 and o[side] + 40 * stride + rb <= size
        want_l, want_r, skipped = model(local, remote, ops, itype)
        assert skipped == 3 + 3  # a row with one bad index of two is skipped whole
        before = api.indexed_counters()
        with pytest.raises(api.OcmError, match=rf"skipped {skipped} row\(s\)") as ei:
            a.indexed_batch(ops, itype, async_=async_)
            if async_:
                a.wait()
        assert ("ocm_wait" in str(ei.value)) == async_
        after = api.indexed_counters()
        assert after["n_indexed_skipped"] == before["n_indexed_skipped"] + skipped
        assert after["n_indexed"] == before["n_indexed"] + 1
        a.wait()  # reported once
        got_l = read_local(a, 0, local_bytes).numpy()
        assert np.array_equal(got_l, want_l), np.flatnonzero(got_l != want_l)[:4]
        assert np.array_equal(remote_bytes_of(a, local_bytes, remote_bytes), want_r)
        # the next op succeeds
        put_ids(a, want_l, ridx_off + 64, [7, 0, 7, 1, 2, 3])
        torch.cuda.synchronize()
        a.indexed_batch(ops[:1], itype)
        want_l2, _, skipped = model(want_l, want_r, ops[:1], itype)
        assert skipped == 0 and np.array_equal(read_local(a, 0, local_bytes).numpy(), want_l2)
        a.free()


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("n_ops", [16, 17, 40])  # the most ops the kernel arguments hold, one more, and a long list
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_lists_and_counters(mesh_factory, n_daemons, n_ops, async_):
    itype = ITYPES[(n_ops + async_) % 2]
    lay = mixed_layout(itype, n_ops, seed=n_ops)
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
        before, before_all = api.indexed_counters(), api.counters()
        skipped, err = run_layout(a, lay, seed=n_ops, async_=async_)
        assert skipped == 0 and err is None, err
        after, after_all = api.indexed_counters(), api.counters()
        rows, nbytes = nominal(lay.ops)
        assert after["n_indexed"] == before["n_indexed"] + 1 and after["n_indexed_ops"] == before["n_indexed_ops"] + n_ops
        assert after["n_indexed_rows"] == before["n_indexed_rows"] + rows
        assert after["bytes_indexed"] == before["bytes_indexed"] + nbytes
        assert after["n_indexed_skipped"] == before["n_indexed_skipped"]
        # its own launch: neither a strided list nor a batch of rows (the helpers' plain puts and gets are no batches)
        assert after_all["n_strided"] == before_all["n_strided"] and after_all["n_batch"] == before_all["n_batch"]
        a.free()


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_same_bytes_as_strided_and_as_a_batch_of_rows(mesh_factory, n_daemons, itype):
    with _client(mesh_factory, n_daemons) as c:
        # index = arange: the strided op
        lay = Layout(itype)
        for rb, rows in ((17, 5), (4097, 3), (256, 37)):
            lay.op(1, rb, np.arange(rows), None, rows, rows, False, 3, 8)
            lay.op(0, rb, None, np.arange(rows), rows, rows, False, 6, 3)
        strided = [[o[0], o[1], o[2], o[3], o[4], o[5], o[6]] for o in lay.ops]
        # any index: the batch of rows expanded on the host
        mixed = mixed_layout(itype, 20, seed=9)
        for L, other in ((lay, lambda a, local: a.strided_batch(np.asarray(strided, dtype=np.int64))),
                         (mixed, lambda a, local: a.batch(api.batch_ops(expand(local, mixed.ops, itype))))):
            got = []
            for indexed in (True, False):
                a = _pair(c, L.local_bytes, L.remote_bytes, n_daemons)
                local, _ = fill_pair(a, L.local_bytes, L.remote_bytes, seed=4, random_remote=True)
                L.install(a, local)
                if indexed:
                    a.indexed_batch(L.ops, itype)
                else:
                    other(a, local)
                got.append((read_local(a, 0, L.local_bytes).numpy(), remote_bytes_of(a, L.local_bytes, L.remote_bytes)))
                a.free()
            assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_lookup_ordered_after_the_kernel_that_made_the_ids(mesh_factory, n_daemons, dtype):
    g = torch.Generator().manual_seed(5)
    with _client(mesh_factory, n_daemons) as c:
        emb = RemoteEmbedding(c, 2000, 136, torch.float16, max_ids=1500, stripe_unit=UNIT)  # rows of 272 bytes
        assert emb.alloc.local_bytes <= 1 << 20 and emb.alloc.remote_size() <= 1 << 20 and emb.out.is_cuda
        table = torch.randn((2000, 136), generator=g).to(torch.float16)
        emb.load(table.cuda())
        host_table = table.clone()  # a host copy of the table
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(3):
                ids = torch.randint(0, 2000, (1500,), device="cuda", dtype=dtype)  # made by a kernel on `side`
                rows = emb.lookup(ids)           # no host sync in between
                got = rows.clone()               # read by torch on `side`
                side.synchronize()
                assert torch.equal(got.cpu().view(torch.int16), torch.index_select(host_table, 0, ids.cpu().long()).view(torch.int16))
            # scatter put of rows made on the stream, then looked up again
            uniq = torch.randperm(2000, device="cuda")[:700].to(dtype)
            new = torch.randn((700, 136), device="cuda").to(torch.float16)
            emb.update(uniq, new, async_=True)
            back = emb.lookup(uniq).clone()
            side.synchronize()
            assert torch.equal(back.view(torch.int16), new.view(torch.int16))
            with pytest.raises(IndexError, match=r"skipped 1 row\(s\)"):
                emb.lookup(torch.tensor([1, 2000, 3], device="cuda", dtype=dtype), async_=False)
        emb.wait()
        emb.close()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_kv_offload_indexed_gpu(mesh_factory, n_daemons):
    with _client(mesh_factory, n_daemons) as c:
        kv = PagedKVOffload(c, 32, 64, (2, 8, 64), dtype=torch.float16, stripe_unit=UNIT, indexed_ids=32)
        assert kv.block_bytes == 2048 and kv.gpu_cache.is_cuda and tuple(kv.gpu_cache.shape) == (32, 2, 8, 64)
        side = torch.cuda.Stream()
        before = api.indexed_counters()
        with torch.cuda.stream(side):  # torch work on a non-default stream
            exercise_indexed_kv(kv, 6, seed=n_daemons, device="cuda:0")
        torch.cuda.synchronize()
        after = api.indexed_counters()
        assert after["n_indexed"] == before["n_indexed"] + 12 and after["n_indexed_skipped"] == before["n_indexed_skipped"]
        kv.close()
