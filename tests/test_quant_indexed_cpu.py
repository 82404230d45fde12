"""Indexed converting ops (ocm_copy_onesided_quant_indexed) on the host path: a CPU app with
host-memory pairs, on one daemon and striped over three owners with a 4 KiB stripe unit. Every byte
of both halves is compared with the model (quant_indexed_cases: the list expanded into plain
converting rows with the skip rule, each row through the torch oracle of its format)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import RemoteEmbedding, RemoteEmbeddingAdam
from quant_cases import read_local
from quant_indexed_cases import (DTYPES, FORMAT_NAMES, NONE, ROW_ELEMS, UNIT, Layout, edge_layouts, embedding_reference,
                                 mixed_layout, nominal, record_bytes, record_up32, run_layout)
from mx4_cases import FORMATS

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
    P = api.OcmQuantIndexedParams
    assert ctypes.sizeof(P) == 96
    assert [getattr(P, f).offset for f in ("row_elems", "local_index_offset", "remote_rows", "op_flag", "index_type", "dtype",
                                           "reserved")] == [16, 48, 72, 80, 84, 88, 92]
    assert api.QUANT_INDEXED_COUNTER_KEYS == ["n_quant_indexed", "n_quant_indexed_ops", "n_quant_indexed_rows",
                                              "bytes_quant_indexed_src", "bytes_quant_indexed_wire"]
    assert list(api.quant_indexed_counters()) == api.QUANT_INDEXED_COUNTER_KEYS and len(api.COUNTER_KEYS) == 28
    ops = api.quant_indexed_ops([[1, 2, 3, 4, 5, 6, 7, NONE, 8, 9, 10], [0, 0, 0, 32, 1, 64, 64, -1, 0, 1, 1]], torch.bfloat16,
                                api.OCM_INDEX_I32, ["mxfp8", "mxfp4"])
    o = ops.array[0]
    assert ops.quant_indexed and ops.n == 2
    assert (o.op_flag, o.local_offset, o.remote_offset, o.row_elems, o.rows, o.local_stride, o.remote_stride,
            o.local_index_offset, o.remote_index_offset, o.local_rows, o.remote_rows, o.index_type, o.dtype, o.reserved) == \
        (1, 2, 3, 4, 5, 6, 7, NONE, 8, 9, 10, 1, api.OCM_QUANT_BF16, 0)
    assert ops.array[1].dtype == api.OCM_QUANT_BF16 | api.OCM_QUANT_MXFP4 and ops.array[1].local_index_offset == NONE
    assert api.quant_indexed_ops(np.array([[0, 0, 0, 32, 1, 64, 64, -1, 0, 1, 1]]), torch.float16, torch.int64,
                                 "mxfp4").array[0].index_type == api.OCM_INDEX_I64


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("fmt", FORMAT_NAMES)
@pytest.mark.parametrize("rows", [1, 2, 37])
def test_edge_rows(client, rows, fmt, itype):
    for n, re in enumerate(ROW_ELEMS):
        dtype = DTYPES[(n + rows) % 2]
        for lay in edge_layouts(itype, fmt, re, rows, lpad=16 * (n % 2), rpad=(0, 32, 96)[n % 3]):
            a = _pair(client, lay.local_bytes, lay.remote_bytes)
            skipped, err, _ = run_layout(a, lay, dtype, seed=re + rows)
            assert skipped == 0 and err is None, err
            a.free()


@pytest.mark.parametrize("async_", [False, True])
def test_mixed_list_and_counters(client, async_):
    itype = api.OCM_INDEX_I32 if async_ else api.OCM_INDEX_I64
    lay = mixed_layout(itype, 50)
    a = _pair(client, lay.local_bytes, lay.remote_bytes)
    assert len(a.remote_info()["extents"]) == (1 if client.n_daemons == 1 else 3)
    before, before_idx, before_all = api.quant_indexed_counters(), api.indexed_counters(), api.counters()
    skipped, err, _ = run_layout(a, lay, torch.float16, seed=5, async_=async_)
    assert skipped == 0 and err is None, err
    after, after_idx, after_all = api.quant_indexed_counters(), api.indexed_counters(), api.counters()
    rows, src, wire = nominal(lay.ops, lay.formats)
    assert after["n_quant_indexed"] == before["n_quant_indexed"] + 1
    assert after["n_quant_indexed_ops"] == before["n_quant_indexed_ops"] + 50
    assert after["n_quant_indexed_rows"] == before["n_quant_indexed_rows"] + rows
    assert after["bytes_quant_indexed_src"] == before["bytes_quant_indexed_src"] + src
    assert after["bytes_quant_indexed_wire"] == before["bytes_quant_indexed_wire"] + wire
    # its own call: no indexed op, no converting list
    assert after_idx == before_idx and after_all["n_quant"] == before_all["n_quant"] and list(after_all) == api.COUNTER_KEYS
    assert api.quant_strided_counters()["n_quant_strided"] >= 0
    a.free()


FAR = {api.OCM_INDEX_I32: [-1, -(1 << 31), 8, (1 << 31) - 1, 40],
       api.OCM_INDEX_I64: [-1, -(1 << 31), 8, (1 << 31) - 1, 1 << 40, -(1 << 63), 1 << 32]}


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("itype", ITYPES)
def test_out_of_range_rows_are_skipped_and_counted(client, itype, async_):
    bad = FAR[itype]
    # tables of 8 rows; rows of three tiles (4128 elements) so a skipped row has several tiles
    for re, fmt in ((32, "mxfp4"), (4128, "mxfp8")):
        lay = Layout(itype)
        ridx = [3, bad[0], 0, bad[1], 7] + bad[2:] + [5]
        lay.op(0, fmt, re, None, ridx, len(ridx), 8, 16, 32)                      # gather with bad remote ids
        lidx = [2, bad[0], bad[2], 6]
        lay.op(1, fmt, re, lidx, None, 8, len(lidx), 16, 32)                      # put with bad local ids
        lay.op(0, fmt, re, [0, bad[1], 2, 3], [4, 5, bad[2], 7], 8, 8)            # one bad index of two skips the row whole
        a = _pair(client, lay.local_bytes, lay.remote_bytes)
        before, before_q = api.indexed_counters(), api.quant_indexed_counters()
        skipped, err, _ = run_layout(a, lay, torch.bfloat16, seed=re, async_=async_)  # every other byte per the model
        assert skipped == len(bad) + 2 + 2
        assert isinstance(err, api.OcmError) and f"indexed ops skipped {skipped} row(s)" in str(err), err
        assert ("ocm_wait" in str(err)) == async_
        after, after_q = api.indexed_counters(), api.quant_indexed_counters()
        # one skip count for both calls; the transfer was made and counted, nominally
        assert after["n_indexed_skipped"] == before["n_indexed_skipped"] + skipped and after["n_indexed"] == before["n_indexed"]
        assert after_q["n_quant_indexed"] == before_q["n_quant_indexed"] + 1
        assert after_q["n_quant_indexed_rows"] == before_q["n_quant_indexed_rows"] + len(ridx) + len(lidx) + 4
        a.wait()  # reported once
        good = Layout(itype)
        good.op(0, fmt, re, None, [7, 0, 7], 3, 8)
        skipped, err, _ = run_layout(a, good, torch.bfloat16, seed=3)  # the next call succeeds
        assert skipped == 0 and err is None, err
        a.free()


@pytest.mark.parametrize("fmt", FORMAT_NAMES)
def test_indexed_put_read_back_by_a_plain_converting_get(client, fmt):
    # a scatter of 5 rows of 1056 elements into a table of 9 records; then ONE plain converting get of one of them
    dtype, re = torch.float16, 1056
    lay = Layout(api.OCM_INDEX_I64)
    ridx = [6, 1, 8, 0, 3]
    o = lay.op(1, fmt, re, None, ridx, 5, 9, 16, 96)
    stage = lay.index([0] * (2 * re // 8 + 2))  # room in the local half that no op touches, for the get below
    a = _pair(client, lay.local_bytes, lay.remote_bytes)
    skipped, err, (got_l, _) = run_layout(a, lay, dtype, seed=2)
    assert skipped == 0 and err is None, err
    stage = (stage + 15) // 16 * 16
    _, roundtrip = FORMATS[fmt]
    for j in (2, 0):
        a.quant_batch([[0, stage, o[2] + ridx[j] * o[6], re]], dtype, format=fmt)
        src = torch.from_numpy(got_l[o[1] + j * o[5]: o[1] + j * o[5] + 2 * re].copy()).view(dtype)
        assert torch.equal(read_local(a, stage, 2 * re).view(torch.int16), roundtrip(src).view(torch.int16))
    # and a strided converting get of the whole table's first two records
    a.quant_strided_batch([[0, stage, o[2] + ridx[3] * o[6], re, 1, 2 * re, o[6]]], dtype, format=fmt)
    src = torch.from_numpy(got_l[o[1] + 3 * o[5]: o[1] + 3 * o[5] + 2 * re].copy()).view(dtype)
    assert torch.equal(read_local(a, stage, 2 * re).view(torch.int16), roundtrip(src).view(torch.int16))
    a.free()


def test_validation(client):
    LB, RB = 8192, 4 * UNIT
    a = _pair(client, LB, RB)
    lib = client.lib
    #       flag lo ro  re rows ls  rs  lidx  ridx  lrows rrows      (64 elements: 128 local bytes, 66 record bytes)
    good = [0, 0, 0, 64, 4, 128, 96, NONE, 4096, 4, 8]

    def fails(row, what, itype=api.OCM_INDEX_I32, fmt="mxfp8"):
        with pytest.raises(api.OcmError) as ei:
            a.quant_indexed_batch([good, row], torch.float16, itype, format=fmt)  # the bad op is op 1
        msg = str(ei.value)
        assert "quant_indexed op 1" in msg and what in msg, msg

    def fails_field(field, value, what):
        two = api.quant_indexed_ops([good, good], torch.float16, api.OCM_INDEX_I32)
        setattr(two.array[1], field, value)
        with pytest.raises(api.OcmError, match="op 1: .*" + what):
            a.quant_indexed_batch(two)

    for bits in (0, 3, api.OCM_QUANT_FP16 | 0x200, api.OCM_QUANT_FP16 | 0x10000):  # unknown dtype bits
        fails_field("dtype", bits, "")
    for bad_type in (0, 3, 7):
        fails_field("index_type", bad_type, "index_type")
    fails_field("reserved", 1, "reserved")
    fails([0, 0, 0, 64, 4, 128, 96, NONE, NONE, 4, 8], "no index on either side")
    fails([0, 0, 0, 33, 4, 128, 96, NONE, 4096, 4, 8], "multiple of 32")
    fails([0, 0, 0, 1 << 31, 4, 128, 96, NONE, 4096, 4, 8], "2^31")
    fails([0, 0, 0, 64, 1 << 32, 128, 96, NONE, 4096, 4, 8], "2^32")
    fails([0, 0, 0, 64, 4, 128, 96, NONE, 4096, 1 << 32, 8], "local table of")
    fails([0, 0, 0, 64, 4, 128, 96, NONE, 4096, 4, 1 << 32], "remote table of")
    fails([1, 8, 0, 64, 4, 128, 96, NONE, 4096, 4, 8], "local offset")                  # alignment: 16 local, 32 remote
    fails([1, 0, 16, 64, 4, 128, 96, NONE, 4096, 4, 8], "remote offset")
    fails([1, 0, 0, 64, 4, 136, 96, NONE, 4096, 4, 8], "local stride")
    fails([1, 0, 0, 64, 4, 128, 112, NONE, 4096, 4, 8], "remote stride")
    fails([1, 0, 0, 64, 4, 112, 96, NONE, 4096, 4, 8], "local stride")                  # below the row's 128 bytes
    fails([1, 0, 0, 64, 4, 128, 64, NONE, 4096, 4, 8], "remote stride")                 # below the record's 66 bytes
    fails([1, 0, 0, 64, 4, 128, 32, NONE, 4096, 4, 8], "remote stride", fmt="mxfp4")    # below the MXFP4 record's 34
    fails([0, 4096 - 4 * 128 + 16, 0, 64, 4, 128, 96, NONE, 4096, 4, 8], "overlaps")    # the get would write its ids
    fails([0, 0, 0, 64, 4, 128, 96, 200, 4096, 8, 8], "local index array")              # ... either array
    fails([1, LB - 4 * 128 + 16, 0, 64, 4, 128, 96, NONE, 4096, 4, 8], "local table")   # last row 16 bytes too far
    fails([1, 0, RB - 7 * 96 - 64, 64, 4, 128, 96, NONE, 4096, 4, 8], "remote table")   # the record's last two bytes
    fails([1, 0, 0, 64, 4, 128, (RB - 66) // 7 // 32 * 32 + 32, NONE, 4096, 4, 8], "remote table")  # the TABLE's last row
    fails([1, 0, 0, 64, 5, 128, 96, NONE, 4096, 4, 8], "local side has no index")
    fails([1, 0, 0, 64, 5, 128, 96, 4096, NONE, 8, 4], "remote side has no index")
    fails([1, 0, 0, 64, 4, 128, 96, NONE, 4098, 4, 8], "not a multiple")
    fails([1, 0, 0, 64, 4, 128, 96, NONE, 4100, 4, 8], "not a multiple", api.OCM_INDEX_I64)
    fails([1, 0, 0, 64, 4, 128, 96, NONE, LB - 12, 4, 8], "index array")
    fails([1, 0, 0, 64, 4, 128, 96, (1 << 64) - 8, NONE, 8, 4], "index array", api.OCM_INDEX_I64)
    # checks that must not overflow: (rows - 1) * stride wraps 64 bits to something small
    fails([1, 0, 0, 32, 1, 1 << 63, 64, 4096, NONE, (1 << 32) - 1, 1], "local table")
    fails([1, 0, 0, 32, 1, 64, 1 << 62, NONE, 4096, 1, 5], "remote table")              # 4 * 2^62 wraps to 0
    fails([1, 0, 0, 32, 1, (1 << 63) + 64, 64, 4096, NONE, 3, 1], "local table")
    fails([1, 0, (1 << 64) - 32, 32, 1, 64, 64, NONE, 4096, 1, 1], "remote table")      # offset + record bytes wraps
    one = api.quant_indexed_ops([good], torch.float16, api.OCM_INDEX_I32)
    assert lib.ocm_copy_onesided_quant_indexed(a.handle, one.array, -1, 0) == -1 and "n_ops" in api.last_error()
    assert lib.ocm_copy_onesided_quant_indexed(a.handle, None, 1, 0) == -1 and api.last_error()
    assert lib.ocm_copy_onesided_quant_indexed(None, one.array, 1, 0) == -1 and api.last_error()
    loc = client.alloc(api.OCM_LOCAL_HOST, local_bytes=8192)  # a local allocation is no remote pair
    with pytest.raises(api.OcmError, match="remote pair"):
        loc.quant_indexed_batch([good], torch.float16, api.OCM_INDEX_I32)
    loc.free()
    for other in (api.batch_ops(np.array([[1, 0, 0, 32]])), api.strided_ops(np.array([[1, 0, 0, 16, 2, 16, 16]])),
                  api.quant_ops(np.array([[1, 0, 0, 32]]), torch.float16),
                  api.quant_strided_ops(np.array([[1, 0, 0, 32, 1, 64, 64]]), torch.float16),
                  api.indexed_ops([[0, 0, 0, 16, 4, 16, 16, NONE, 4096, 4, 8]], api.OCM_INDEX_I32)):
        with pytest.raises(TypeError):
            a.quant_indexed_batch(other)
    for call in (a.indexed_batch, a.quant_strided_batch, a.quant_batch):
        with pytest.raises(TypeError):
            call(one)
    # exact fits pass: the table's last record ends at the half's end, the index array too; one-row tables with stride 0
    a.local_tensor(torch.uint8)[LB - 16:].zero_()
    a.quant_indexed_batch([[0, 0, RB - 2 * 1056, 1024, 2, 2048, 1056, NONE, LB - 8, 2, 2]], torch.float16, api.OCM_INDEX_I32)
    a.quant_indexed_batch([[1, 0, 0, 64, 1, 0, 0, LB - 16, NONE, 1, 1]], torch.float16, api.OCM_INDEX_I32)
    # empty ops say anything (but a known dtype and a row size that is a multiple of 32)
    before = api.quant_indexed_counters()
    a.quant_indexed_batch([[1, 1 << 40, 1 << 40, 0, 9, 1, 1, 3, 3, 1 << 40, 1 << 40], [0, 5, 5, 64, 0, 0, 0, NONE, NONE, 0, 0]],
                          torch.float16, 9)
    after = api.quant_indexed_counters()
    assert after["n_quant_indexed"] == before["n_quant_indexed"] + 1
    assert after["n_quant_indexed_ops"] == before["n_quant_indexed_ops"] + 2
    assert after["n_quant_indexed_rows"] == before["n_quant_indexed_rows"]
    assert after["bytes_quant_indexed_wire"] == before["bytes_quant_indexed_wire"]
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMAT_NAMES)
def test_remote_embedding_compressed(client, fmt, dtype):
    g = torch.Generator().manual_seed(7)
    rows, dim = 1000, 96
    emb = RemoteEmbedding(client, rows, dim, dtype, max_ids=300, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT, compress=fmt)
    assert emb.record_stride == record_up32(dim, fmt) == {"mxfp8": 128, "mxfp4": 64}[fmt]
    assert emb.remote_bytes == rows * emb.record_stride == emb.alloc.remote_size() and emb.row_bytes == 2 * dim
    assert api.quant_bytes(dim, fmt) == record_bytes(dim, fmt)
    table = torch.randn((rows, dim), generator=g).to(dtype)
    want = embedding_reference(table, fmt)
    before = api.quant_indexed_counters()
    emb.load(table)
    ids_dtype = torch.int32 if dtype == torch.float16 else torch.int64
    ids = torch.randint(0, rows, (300,), generator=g).to(ids_dtype)
    ids[5:9] = ids[0]
    for async_ in (True, False):
        got = emb.lookup(ids, async_=async_)
        emb.wait()
        assert got.shape == (300, dim)
        assert torch.equal(got.view(torch.int16), torch.index_select(want, 0, ids.long()).view(torch.int16))
    after = api.quant_indexed_counters()
    assert after["n_quant_indexed"] == before["n_quant_indexed"] + 2  # each lookup ONE indexed converting get
    assert after["bytes_quant_indexed_wire"] == before["bytes_quant_indexed_wire"] + 2 * 300 * record_bytes(dim, fmt)
    assert emb.lookup(ids[:0]).shape == (0, dim)
    # scatter put with unique ids, then read back: the round trip of the new rows
    uniq = torch.randperm(rows, generator=g)[:100].to(ids_dtype)
    new = torch.randn((100, dim), generator=g).to(dtype)
    emb.update(uniq, new)
    want[uniq.long()] = embedding_reference(new, fmt)
    assert torch.equal(emb.lookup(uniq, async_=False).view(torch.int16), want[uniq.long()].view(torch.int16))
    others = torch.arange(0, 300, dtype=ids_dtype)
    assert torch.equal(emb.lookup(others, async_=False).view(torch.int16), want[:300].view(torch.int16))
    # ids outside the table: skipped, counted, and the others moved
    emb.out.zero_()
    bad = torch.tensor([3, rows, 5, -1, rows - 1], dtype=ids_dtype)
    with pytest.raises(IndexError, match=r"skipped 2 row\(s\)"):
        emb.lookup(bad, async_=False)
    assert torch.equal(emb.out[[0, 2, 4]].view(torch.int16), want[[3, 5, rows - 1]].view(torch.int16)) and not emb.out[[1, 3]].any()
    emb.lookup(bad, async_=True)  # async: known at wait()
    with pytest.raises(IndexError, match=r"skipped 2 row\(s\)"):
        emb.wait()
    emb.wait()
    emb.close()


def test_remote_embedding_refusals_and_the_uncompressed_table(client):
    kw = dict(kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT)
    with pytest.raises(ValueError, match="dim % 32"):
        RemoteEmbedding(client, 100, 24, torch.float16, compress="mxfp8", **kw)
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        RemoteEmbedding(client, 100, 32, torch.float32, compress="mxfp4", **kw)
    with pytest.raises(ValueError, match="mxfp8"):
        RemoteEmbedding(client, 100, 32, torch.float16, compress="fp8", **kw)
    emb = RemoteEmbedding(client, 100, 32, torch.bfloat16, max_ids=16, compress="mxfp8", **kw)
    with pytest.raises(TypeError, match="compressed"):
        RemoteEmbeddingAdam(emb)
    emb.close()
    # compress=None: every size is what it was
    plain = RemoteEmbedding(client, 1000, 24, torch.float16, max_ids=300, **kw)
    assert plain.compress is None and plain.record_stride == plain.row_bytes == 48
    assert plain.remote_bytes == plain.alloc.remote_size() == 48000 and plain.alloc.local_bytes == 300 * 48 + 8 * 300
    plain.close()


@pytest.mark.parametrize("fmt", FORMAT_NAMES)
def test_embedding_example_compressed_cpu(native, fmt):
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "embedding_offload.py"), "--rows", "3000", "--compress", fmt],
                       capture_output=True, text=True, timeout=300, cwd="/tmp", env=dict(os.environ, OCM_NO_GPU="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"lookups equal the {fmt} round trip of index_select" in r.stdout and "out of range:" in r.stdout
    assert "remote bytes" in r.stdout
