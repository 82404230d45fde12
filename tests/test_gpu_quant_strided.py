"""Strided converting ops on the gfx950 kernel path (csrc/src/kernels/xfer_quant_strided.hip):
every byte of both halves against the model (records against the torch oracle, decoded rows
against its round trip, the sentinel everywhere else), with the pool in the pinned host tier
(one daemon) and striped over three owners (four daemons, a 4 KiB stripe unit)."""
import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from oncilla_amd.ops import mx8_rows_reference
from quant_cases import TABLE_ROWS, UNIT, decode_table, random_elems, read_local, roundtrip, write_local, write_remote
from quant_strided_cases import (DTYPES, ROWS, STRIDES, Case, edge_case, exercise_layered_quant_kv, expand, halves,
                                 list_case, load_pair, record_up32, run_case, src_wire_bytes)

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM


def _client(mesh_factory, n_daemons):
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _pair(c, local_bytes, remote_bytes, n_daemons, kind=api.OCM_REMOTE_GPU):
    a = c.alloc(kind, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE, stripe_unit=UNIT)
    assert len(a.remote_info()["extents"]) == (1 if n_daemons == 1 else 3)
    return a


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_edge_rows(mesh_factory, n_daemons, rows):
    with _client(mesh_factory, n_daemons) as c:
        # every stride pairing, the element types alternating over them
        for k, strides in enumerate(STRIDES):
            case = edge_case(rows, *strides)
            a = _pair(c, case.local_bytes, case.remote_bytes, n_daemons)
            before = api.quant_strided_counters()
            run_case(a, case, DTYPES[(k + rows) % 2], seed=rows)
            after = api.quant_strided_counters()
            src, wire = src_wire_bytes(case.ops)
            assert after["n_quant_strided"] == before["n_quant_strided"] + 1
            assert after["bytes_quant_strided_src"] == before["bytes_quant_strided_src"] + src
            assert after["bytes_quant_strided_wire"] == before["bytes_quant_strided_wire"] + wire
            a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_decode_table_rows(mesh_factory, n_daemons, dtype):
    # every code under every scale byte through the strided kernel's own tile location: 32 rows of
    # 2048 elements, one strided get
    t = decode_table()
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, *t.bytes(TABLE_ROWS), n_daemons)
        t.run_strided(a, dtype, TABLE_ROWS)
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_same_bytes_as_the_expanded_list(mesh_factory, n_daemons):
    case = list_case(30, seed=9)  # more ops than travel in the kernel arguments
    dtype = torch.float16
    with _client(mesh_factory, n_daemons) as c:
        got = []
        before = api.counters()
        for strided in (True, False):
            a = _pair(c, case.local_bytes, case.remote_bytes, n_daemons)
            run = None if strided else (lambda ops: a.quant_batch(expand(ops), dtype))
            got.append(run_case(a, case, dtype, seed=6, run=run))
            a.free()
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        assert api.counters()["n_quant"] == before["n_quant"] + 1  # only the expanded list was a converting list


@pytest.mark.parametrize("n_ops", [24, 25])  # the most ops the kernel arguments hold, and one more
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_list_at_the_inline_capacity(mesh_factory, n_daemons, n_ops):
    case = list_case(n_ops, seed=n_ops)
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, case.local_bytes, case.remote_bytes, n_daemons)
        before = api.quant_strided_counters()
        run_case(a, case, torch.bfloat16, seed=n_ops)
        after = api.quant_strided_counters()
        assert after["n_quant_strided_ops"] == before["n_quant_strided_ops"] + n_ops
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_host_path_records_match_kernel_path(mesh_factory, n_daemons):
    re, rows = 2080, 5
    ls, rs = 2 * re + 16, record_up32(re) + 32
    put = Case([[1, 0, 2 * UNIT - 64, re, rows, ls, rs]], 2 * rows * ls, 8 * UNIT)
    get = Case([[0, rows * ls, 2 * UNIT - 64, re, rows, ls, rs]], 2 * rows * ls, 8 * UNIT)
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            local, remote, want_l, want_r = put.prepare(dtype, seed=21)
            h = _pair(c, put.local_bytes, put.remote_bytes, n_daemons, kind=api.OCM_REMOTE_RDMA)  # the host codec
            d = _pair(c, put.local_bytes, put.remote_bytes, n_daemons)                            # the kernel
            recs = []
            for a in (h, d):
                load_pair(a, local, remote)
                a.quant_strided_batch(put.ops, dtype)
                got_l, got_r = halves(a, put)
                assert np.array_equal(got_r, want_r) and np.array_equal(got_l, want_l)
                recs.append(got_r)
            assert np.array_equal(recs[0], recs[1])
            # the host path's records through the kernel's decode, and the other way round
            for a, other in ((h, recs[1]), (d, recs[0])):
                load_pair(a, got_l, other)
                a.quant_strided_batch(get.ops, dtype)
                back = read_local(a, rows * ls, rows * ls).numpy().reshape(rows, ls)
                src = got_l[:rows * ls].reshape(rows, ls)[:, :2 * re].copy()
                want = roundtrip(torch.from_numpy(src).view(dtype)).view(torch.uint8).numpy()
                assert np.array_equal(back[:, :2 * re], want)
            h.free()
            d.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_async_list_signals_a_side_stream(mesh_factory, n_daemons):
    re, rows, dtype = 1056, 5, torch.bfloat16
    rs = record_up32(re) + 32
    n = rows * re
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 8 * n, 8 * UNIT, n_daemons)
        x = random_elems(2 * n, dtype, seed=33).view(2, rows, re)
        for k, ro in enumerate((UNIT - 64, 4 * UNIT + 32)):
            recs = torch.zeros((rows, rs), dtype=torch.uint8)
            recs[:, :re + re // 32] = mx8_rows_reference(x[k])
            write_remote(a, 4 * n, ro, recs)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lt = a.local_tensor(torch.int16)
            lt[:2 * n].fill_(0x5A5A)  # torch writes on the side stream; the list must start after them
            a.stream_wait()
            a.quant_strided_batch(np.array([[0, 0, UNIT - 64, re, rows, 2 * re, rs],
                                            [0, 2 * n, 4 * UNIT + 32, re, rows, 2 * re, rs]]), dtype, async_=True)
            a.stream_signal()
            got = lt[:2 * n].clone()  # read on the side stream, no host sync in between
        side.synchronize()
        assert torch.equal(got.cpu(), roundtrip(x).view(torch.int16).reshape(-1))
        a.wait()
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_kv_offload_layers_mxfp8_rows_gpu(mesh_factory, n_daemons):
    with _client(mesh_factory, n_daemons) as c:
        kv = PagedKVOffload(c, 16, 64, (2, 8, 64), dtype=torch.float16, stripe_unit=UNIT, layers=3, compress="mxfp8-rows")
        assert kv.block_bytes == 2048 and kv.pool_block_bytes == 3 * 1056  # per layer: 1024 codes + 32 scale bytes
        assert tuple(kv.gpu_cache.shape) == (3, 16, 2, 8, 64) and kv.gpu_cache.is_cuda
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # torch work on a non-default stream
            exercise_layered_quant_kv(kv, 8, seed=n_daemons, device="cuda:0")
        torch.cuda.synchronize()
        kv.close()
