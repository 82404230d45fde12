"""Indexed one-sided ops (ocm_copy_onesided_indexed) on the host path: a CPU app with host-memory
pairs, on one daemon and striped over three owners with a small stripe unit. Every byte of both
halves is compared with the numpy model (indexed_cases.model), skip rule included."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from indexed_cases import (NONE, ROW_BYTES, SENTINEL, UNIT, Layout, edge_layout, exercise_indexed_kv, fill_pair, mixed_layout,
                           nominal, read_local, remote_bytes_of, run_layout)
from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload, RemoteEmbedding

N_DAEMONS = [1, 4]
ITYPES = [api.OCM_INDEX_I32, api.OCM_INDEX_I64]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=N_DAEMONS)
def client(request, mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(request.param, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        c.n_daemons = request.param
        yield c


def _pair(c, local_bytes, remote_bytes):
    return c.alloc(api.OCM_REMOTE_RDMA, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                   stripe_unit=UNIT)


def test_struct_layout_and_names(native):
    assert ctypes.sizeof(api.OcmIndexedParams) == 88
    assert api.OcmIndexedParams.local_index_offset.offset == 48 and api.OcmIndexedParams.remote_rows.offset == 72
    assert api.OcmIndexedParams.op_flag.offset == 80 and api.OcmIndexedParams.index_type.offset == 84
    assert api.OCM_INDEX_NONE == NONE and (api.OCM_INDEX_I32, api.OCM_INDEX_I64) == (1, 2)
    assert api.COUNTER_KEYS[-3:] == ["n_strided", "n_strided_ops", "bytes_strided"] and len(api.COUNTER_KEYS) == 28
    assert api.INDEXED_COUNTER_KEYS == ["n_indexed", "n_indexed_ops", "n_indexed_rows", "bytes_indexed", "n_indexed_skipped"]
    ops = api.indexed_ops([[1, 2, 3, 4, 5, 6, 7, NONE, 8, 9, 10]], api.OCM_INDEX_I32)
    o = ops.array[0]
    assert ops.indexed and ops.n == 1
    assert (o.op_flag, o.local_offset, o.remote_offset, o.row_bytes, o.rows, o.local_stride, o.remote_stride,
            o.local_index_offset, o.remote_index_offset, o.local_rows, o.remote_rows, o.index_type) == \
        (1, 2, 3, 4, 5, 6, 7, NONE, 8, 9, 10, 1)
    assert api.indexed_ops(np.array([[0, 0, 0, 4, 1, 4, 4, -1, 0, 1, 1]]), torch.int64).array[0].local_index_offset == NONE


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("rows", [1, 2, 37])
def test_gather_scatter_and_both(client, rows, itype):
    for n, rb in enumerate(ROW_BYTES):
        lay = edge_layout(itype, rb, rows, dense=bool(n % 2), agree=bool(n % 3))
        a = _pair(client, lay.local_bytes, lay.remote_bytes)
        skipped, err = run_layout(a, lay, seed=rb)
        assert skipped == 0 and err is None, err
        a.free()


@pytest.mark.parametrize("async_", [False, True])
def test_mixed_list_and_counters(client, async_):
    lay = mixed_layout(api.OCM_INDEX_I32 if async_ else api.OCM_INDEX_I64, 40)
    a = _pair(client, lay.local_bytes, lay.remote_bytes)
    assert len(a.remote_info()["extents"]) == (1 if client.n_daemons == 1 else 3)
    before, before_all = api.indexed_counters(), api.counters()
    skipped, err = run_layout(a, lay, seed=5, async_=async_)
    assert skipped == 0 and err is None, err
    after, after_all = api.indexed_counters(), api.counters()
    rows, nbytes = nominal(lay.ops)
    assert after["n_indexed"] == before["n_indexed"] + 1 and after["n_indexed_ops"] == before["n_indexed_ops"] + 40
    assert after["n_indexed_rows"] == before["n_indexed_rows"] + rows
    assert after["bytes_indexed"] == before["bytes_indexed"] + nbytes
    assert after["n_indexed_skipped"] == before["n_indexed_skipped"]
    assert after_all["n_strided"] == before_all["n_strided"] and list(after_all) == api.COUNTER_KEYS
    a.free()


def test_validation(client):
    LB, RB = 8192, 4 * UNIT
    a = _pair(client, LB, RB)
    lib = client.lib
    #       flag lo ro  rb rows ls  rs  lidx  ridx  lrows rrows
    good = [0, 0, 0, 16, 4, 16, 16, NONE, 4096, 4, 8]

    def fails(row, what, itype=api.OCM_INDEX_I32):
        with pytest.raises(api.OcmError) as ei:
            a.indexed_batch([good, row], itype)  # the bad op is op 1
        msg = str(ei.value)
        assert "op 1" in msg and what in msg, msg

    for bad_type in (0, 3, 7):
        two = api.indexed_ops([good, good], api.OCM_INDEX_I32)
        two.array[1].index_type = bad_type
        with pytest.raises(api.OcmError, match="op 1: index_type"):
            a.indexed_batch(two)
    fails([0, 0, 0, 16, 4, 16, 16, NONE, NONE, 4, 8], "no index on either side")
    fails([0, 0, 0, 16, 1 << 32, 16, 16, NONE, 4096, 4, 8], "2^32")
    fails([0, 0, 0, 16, 4, 16, 16, NONE, 4096, 1 << 32, 8], "local table of")
    fails([0, 0, 0, 16, 4, 16, 16, NONE, 4096, 4, 1 << 32], "remote table of")
    fails([1, 0, 0, 100, 2, 99, 100, NONE, 4096, 2, 2], "local stride")
    fails([1, 0, 0, 100, 2, 100, 99, NONE, 4096, 2, 2], "remote stride")
    fails([0, 4096 - 15 - 48, 0, 16, 4, 16, 16, NONE, 4096, 4, 8], "overlaps")          # the get would write its ids
    fails([0, 0, 0, 16, 4, 16, 16, 60, 4096, 8, 8], "local index array")                # ... either array
    fails([1, LB - 63, 0, 16, 4, 16, 16, NONE, 4096, 4, 8], "local table")              # last row one byte too far
    fails([1, 0, RB - 8 * 16 + 1, 16, 4, 16, 16, NONE, 4096, 4, 8], "remote table")
    fails([1, 0, 0, 16, 4, 16, (RB - 16) // 7 + 1, NONE, 4096, 4, 8], "remote table")   # the TABLE's last row, not the op's
    fails([1, 0, 0, 16, 5, 16, 16, NONE, 4096, 4, 8], "local side has no index")
    fails([1, 0, 0, 16, 5, 16, 16, 4096, NONE, 8, 4], "remote side has no index")
    fails([1, 0, 0, 16, 4, 16, 16, NONE, 4098, 4, 8], "not a multiple")
    fails([1, 0, 0, 16, 4, 16, 16, NONE, 4100, 4, 8], "not a multiple", api.OCM_INDEX_I64)
    fails([1, 0, 0, 16, 4, 16, 16, NONE, LB - 12, 4, 8], "index array")
    fails([1, 0, 0, 16, 4, 16, 16, (1 << 64) - 8, NONE, 8, 4], "index array", api.OCM_INDEX_I64)
    # checks that must not overflow: (rows - 1) * stride wraps 64 bits to something small
    fails([1, 0, 0, 1, 1, 1 << 63, 1, 4096, NONE, (1 << 32) - 1, 1], "local table")
    fails([1, 0, 0, 1, 1, 1, 1 << 62, NONE, 4096, 1, 5], "remote table")                # 4 * 2^62 wraps to 0
    fails([1, 0, 0, 8, 1, (1 << 63) + 8, 8, 4096, NONE, 3, 1], "local table")
    fails([1, 0, (1 << 64) - 4, 8, 1, 8, 8, NONE, 4096, 1, 1], "remote table")          # offset + row_bytes wraps
    one = api.indexed_ops([good], api.OCM_INDEX_I32)
    assert lib.ocm_copy_onesided_indexed(a.handle, one.array, -1, 0) == -1 and "n_ops" in api.last_error()
    assert lib.ocm_copy_onesided_indexed(a.handle, None, 1, 0) == -1 and api.last_error()
    assert lib.ocm_copy_onesided_indexed(None, one.array, 1, 0) == -1 and api.last_error()
    loc = client.alloc(api.OCM_LOCAL_HOST, local_bytes=8192)  # a local allocation is no remote pair
    with pytest.raises(api.OcmError, match="remote pair"):
        loc.indexed_batch([good], api.OCM_INDEX_I32)
    loc.free()
    for other in (api.batch_ops(np.array([[1, 0, 0, 32]])), api.strided_ops(np.array([[1, 0, 0, 16, 2, 16, 16]])),
                  api.quant_ops(np.array([[1, 0, 0, 32]]), torch.float16)):
        with pytest.raises(TypeError):
            a.indexed_batch(other)
    with pytest.raises(TypeError):
        a.strided_batch(one)
    # exact fits pass, and empty ops say anything
    write = torch.zeros(16, dtype=torch.uint8)
    a.local_tensor(torch.uint8)[4096:4112].copy_(write)
    a.indexed_batch([[0, LB - 64, RB - 8 * 16, 16, 4, 16, 16, NONE, 4096, 4, 8]], api.OCM_INDEX_I32)
    before = api.indexed_counters()
    a.indexed_batch([[1, 1 << 40, 1 << 40, 0, 9, 0, 0, 3, 3, 1 << 40, 1 << 40], [0, 5, 5, 9, 0, 0, 0, NONE, NONE, 0, 0]], 9)
    after = api.indexed_counters()
    assert after["n_indexed"] == before["n_indexed"] + 1 and after["n_indexed_ops"] == before["n_indexed_ops"] + 2
    assert after["n_indexed_rows"] == before["n_indexed_rows"] and after["bytes_indexed"] == before["bytes_indexed"]
    a.free()


FAR = {api.OCM_INDEX_I32: [-1, -(1 << 31), 8, (1 << 31) - 1, 40],
       api.OCM_INDEX_I64: [-1, -(1 << 31), 8, (1 << 31) - 1, 1 << 40, -(1 << 63), 1 << 32]}


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("itype", ITYPES)
def test_out_of_range_rows_are_skipped_and_counted(client, itype, async_):
    bad = FAR[itype]
    # tables of 8 rows; rows of three tiles (9000 bytes) so a skipped row has several tiles
    for rb in (16, 9000):
        lay = Layout(itype)
        ridx = [3, bad[0], 0, bad[1], 7] + bad[2:] + [5]
        lay.op(0, rb, None, ridx, len(ridx), 8, False, 3, 8)                       # gather with bad remote ids
        lidx = [2, bad[0], bad[2], 6]
        lay.op(1, rb, lidx, None, 8, len(lidx), False, 6, 3)                       # put with bad local ids
        lay.op(0, rb, [0, bad[1], 2, 3], [4, 5, bad[2], 7], 8, 8, True, 3, 3)      # one bad index of two skips the row whole
        a = _pair(client, lay.local_bytes, lay.remote_bytes)
        before = api.indexed_counters()
        skipped, err = run_layout(a, lay, seed=rb, async_=async_, random_remote=False)  # every other byte per the model
        assert skipped == len(bad) + 2 + 2
        assert isinstance(err, api.OcmError) and f"skipped {skipped} row(s)" in str(err), err
        assert ("ocm_wait" in str(err)) == async_
        after = api.indexed_counters()
        assert after["n_indexed_skipped"] == before["n_indexed_skipped"] + skipped
        assert after["n_indexed"] == before["n_indexed"] + 1  # the transfer was made
        a.wait()  # reported once
        good = Layout(itype)
        good.op(0, rb, None, [7, 0, 7], 3, 8, False, 3, 8)
        skipped, err = run_layout(a, good, seed=3)  # the next call succeeds
        assert skipped == 0 and err is None, err
        a.free()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_remote_embedding(client, dtype):
    g = torch.Generator().manual_seed(7)
    emb = RemoteEmbedding(client, 1000, 24, torch.float16, max_ids=300, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT)
    assert emb.row_bytes == 48 and emb.alloc.remote_size() == 48000
    table = torch.randn((1000, 24), generator=g).to(torch.float16)
    emb.load(table)
    ids = torch.randint(0, 1000, (300,), generator=g).to(dtype)
    ids[5:9] = ids[0]
    for async_ in (True, False):
        rows = emb.lookup(ids, async_=async_)
        emb.wait()
        assert rows.shape == (300, 24) and torch.equal(rows.view(torch.int16), torch.index_select(table, 0, ids.long()).view(torch.int16))
    assert emb.lookup(ids[:0]).shape == (0, 24)
    # scatter put with unique ids, then read back
    uniq = torch.randperm(1000, generator=g)[:100].to(dtype)
    new = torch.randn((100, 24), generator=g).to(torch.float16)
    emb.update(uniq, new)
    table[uniq.long()] = new
    assert torch.equal(emb.lookup(uniq, async_=False).view(torch.int16), new.view(torch.int16))
    # ids outside the table: skipped, counted, and the others moved
    emb.out.zero_()
    bad = torch.tensor([3, 1000, 5, -1, 999], dtype=dtype)
    with pytest.raises(IndexError, match=r"skipped 2 row\(s\)"):
        emb.lookup(bad, async_=False)
    assert torch.equal(emb.out[[0, 2, 4]], table[[3, 5, 999]]) and not emb.out[[1, 3]].any()
    emb.lookup(bad, async_=True)  # async: known at wait()
    with pytest.raises(IndexError, match=r"skipped 2 row\(s\)"):
        emb.wait()
    emb.wait()
    with pytest.raises(ValueError):
        emb.lookup(torch.zeros(301, dtype=dtype))
    with pytest.raises(TypeError):
        emb.lookup(torch.zeros(3, dtype=torch.int16))
    emb.close()


def test_kv_offload_indexed_cpu(client):
    kv = PagedKVOffload(client, 12, 40, (2, 4, 8), dtype=torch.float32, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT, indexed_ids=12)
    assert kv.block_bytes == 256 and kv.alloc.local_bytes == 12 * 256 + 2 * 8 * 12 and tuple(kv.gpu_cache.shape) == (12, 2, 4, 8)
    before = api.indexed_counters()
    exercise_indexed_kv(kv, 6, seed=3, device="cpu")
    after = api.indexed_counters()
    assert after["n_indexed"] == before["n_indexed"] + 12 and after["n_indexed_ops"] == before["n_indexed_ops"] + 12
    with pytest.raises(IndexError, match="skipped 1"):
        kv.swap_out_indexed(torch.tensor([0, 12]), torch.tensor([1, 2]), async_=False)
    kv.swap_in_indexed(torch.tensor([40, 3]), torch.tensor([1, 2]))
    with pytest.raises(IndexError, match="skipped 1"):
        kv.wait()
    with pytest.raises(ValueError):
        kv.swap_out_indexed(torch.arange(13), torch.arange(13))
    kv.close()
    # existing callers: no tail, the same sizes as before
    plain = PagedKVOffload(client, 12, 40, (2, 4, 8), dtype=torch.float32, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT)
    assert plain.alloc.local_bytes == 12 * 256 and plain.indexed_ids == 0
    with pytest.raises(ValueError, match="indexed_ids"):
        plain.swap_out_indexed(torch.tensor([0]), torch.tensor([0]))
    plain.close()
    for kw in ({"layers": 2}, {"compress": "mxfp8"}):
        with pytest.raises(ValueError, match="plain cache"):
            PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, indexed_ids=4, **kw)


def test_embedding_example_cpu(native):
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "embedding_offload.py"), "--rows", "3000"],
                       capture_output=True, text=True, timeout=300, cwd="/tmp", env=dict(os.environ, OCM_NO_GPU="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "lookups equal index_select" in r.stdout and "out of range:" in r.stdout


def test_sentinels_outside_the_rows_stay(client):
    # a gather into a sentinel-filled half: only the selected rows' bytes change on the local side, nothing on the remote
    lay = Layout(api.OCM_INDEX_I64)
    lay.op(0, 100, None, [9, 2, 2, 0], 4, 10, False, 5, 9)
    a = _pair(client, lay.local_bytes, lay.remote_bytes)
    skipped, err = run_layout(a, lay, seed=2, random_remote=False)
    assert skipped == 0 and err is None
    assert (remote_bytes_of(a, lay.local_bytes, lay.remote_bytes) == SENTINEL).all()
    got = read_local(a, 0, lay.local_bytes).numpy()
    o = lay.ops[0]
    for j in range(4):
        assert (got[o[1] + j * o[5]: o[1] + j * o[5] + 100] == SENTINEL).all()
    a.free()
