"""Strided one-sided ops (ocm_copy_onesided_strided) on the host path: a CPU app with
host-memory pairs, on one daemon and striped over three owners with a small stripe unit.
Every byte of both halves is compared with the numpy model (strided_cases.model)."""
import ctypes

import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from strided_cases import (ROWS, SENTINEL, UNIT, edge_case, exercise_layered_kv, fill_pair, mixed_list, model, moved_bytes,
                           read_local, remote_bytes_of, run_case)

N_DAEMONS = [1, 4]


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


def test_struct_layout(native):
    assert ctypes.sizeof(api.OcmStridedParams) == 56
    assert api.OcmStridedParams.op_flag.offset == 48 and api.OcmStridedParams.reserved.offset == 52
    assert api.COUNTER_KEYS[-3:] == ["n_strided", "n_strided_ops", "bytes_strided"]
    assert api.COUNTER_KEYS[21:25] == ["n_quant", "n_quant_ops", "bytes_quant_src", "bytes_quant_wire"]  # did not move


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dense", [True, False])
def test_edge_rows(client, rows, dense):
    case = edge_case(rows, dense, agree=dense)
    a = _pair(client, case.local_bytes, case.remote_bytes)
    run_case(a, case)
    a.free()


def test_mixed_list_and_counters(client):
    ops, local_bytes, remote_bytes = mixed_list()
    a = _pair(client, local_bytes, remote_bytes)
    assert len(a.remote_info()["extents"]) == (1 if client.n_daemons == 1 else 3)
    local, remote = fill_pair(a, local_bytes, remote_bytes, seed=3, random_remote=True)
    before = api.counters()
    a.strided_batch(ops, async_=True)
    a.wait()
    after = api.counters()
    assert after["n_strided"] == before["n_strided"] + 1
    assert after["n_strided_ops"] == before["n_strided_ops"] + len(ops)
    assert after["bytes_strided"] == before["bytes_strided"] + moved_bytes(ops)
    want_l, want_r = model(local, remote, ops)
    assert np.array_equal(read_local(a, 0, local_bytes).numpy(), want_l)
    assert np.array_equal(remote_bytes_of(a, local_bytes, remote_bytes), want_r)
    a.free()


def test_validation(client):
    LB, RB = 8192, 4 * UNIT
    a = _pair(client, LB, RB)
    lib = client.lib
    good = [1, 0, 0, 16, 2, 16, 16]

    def fails(row, what):
        with pytest.raises(api.OcmError) as ei:
            a.strided_batch(np.array([good, row], dtype=np.uint64))  # the bad op is op 1
        msg = str(ei.value)
        assert "op 1" in msg and what in msg, msg

    fails([1, 0, 0, 16, 1 << 32, 16, 16], "2^32")                          # rows
    fails([1, 0, 0, 100, 2, 99, 100], "local stride")                      # strides below the row
    fails([0, 0, 0, 100, 2, 100, 99], "remote stride")
    fails([1, LB - 15, 0, 16, 1, 0, 0], "local range")                     # one row, one byte too far
    fails([1, LB + 1, 0, 1, 1, 0, 0], "local range")
    fails([0, 0, RB - 15, 16, 1, 0, 0], "remote range")
    fails([1, 0, 0, 16, 4, (LB - 16) // 3 + 1, 16], "local range")         # the last row's end
    fails([1, 0, 0, 16, 4, 16, (RB - 16) // 3 + 1], "remote range")
    # checks that must not overflow: (rows - 1) * stride wraps 64 bits to something small
    fails([1, 0, 0, 1, (1 << 32) - 1, 1 << 63, 1], "local range")
    fails([1, 0, 0, 1, 5, 1, 1 << 62], "remote range")                     # 4 * 2^62 wraps to 0
    fails([1, 0, 0, 8, 3, (1 << 63) + 8, 8], "local range")
    fails([0, 0, 0, 8, 3, 8, (1 << 63) + 8], "remote range")
    two = api.strided_ops(np.array([good, good]))
    two.array[1].reserved = 3
    with pytest.raises(api.OcmError, match="op 1: reserved"):
        a.strided_batch(two)
    one = api.strided_ops(np.array([good]))
    assert lib.ocm_copy_onesided_strided(a.handle, one.array, -1, 0) == -1 and "n_ops" in api.last_error()
    assert lib.ocm_copy_onesided_strided(a.handle, None, 1, 0) == -1 and api.last_error()
    assert lib.ocm_copy_onesided_strided(None, one.array, 1, 0) == -1 and api.last_error()
    loc = client.alloc(api.OCM_LOCAL_HOST, local_bytes=4096)  # a local allocation is no remote pair
    with pytest.raises(api.OcmError, match="remote pair"):
        loc.strided_batch(np.array([good]))
    loc.free()
    with pytest.raises(TypeError):
        a.strided_batch(api.batch_ops(np.array([[1, 0, 0, 32]])))
    with pytest.raises(TypeError):
        a.strided_batch(api.quant_ops(np.array([[1, 0, 0, 32]]), torch.float16))
    # exact fits pass
    a.strided_batch(np.array([[1, 0, 0, 16, 4, (LB - 16) // 3, (RB - 16) // 3]]))
    a.free()


def test_empty_calls_do_nothing(client):
    LB, RB = 4096, 2 * UNIT
    a = _pair(client, LB, RB)
    local, remote = fill_pair(a, LB, RB, seed=9)
    before = api.counters()
    assert client.lib.ocm_copy_onesided_strided(a.handle, None, 0, 0) == 0       # zero ops
    a.strided_batch(np.zeros((0, 7), dtype=np.int64))
    # zero rows and zero bytes, wherever they point and whatever their strides
    a.strided_batch(np.array([[1, 0, 0, 64, 0, 64, 64], [0, 0, 0, 0, 5, 0, 0], [1, LB, RB, 0, 3, 0, 0],
                              [0, 1 << 40, 1 << 40, 7, 0, 1, 1]]), async_=True)
    a.wait()
    after = api.counters()
    assert after["n_strided"] == before["n_strided"] + 3 and after["n_strided_ops"] == before["n_strided_ops"] + 4
    assert after["bytes_strided"] == before["bytes_strided"]
    assert np.array_equal(read_local(a, 0, LB).numpy(), local)
    assert np.array_equal(remote_bytes_of(a, LB, RB), remote) and (remote == SENTINEL).all()
    a.free()


def test_kv_offload_layers_cpu(client):
    kv = PagedKVOffload(client, 12, 40, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT, layers=3)
    assert kv.block_bytes == 128 and kv.pool_block_bytes == 3 * 128
    assert tuple(kv.gpu_cache.shape) == (3, 12, 2, 4, 8)
    assert kv.alloc.local_bytes == 3 * 12 * 128 and kv.alloc.remote_size() == 40 * 3 * 128
    ops = kv._ops([(5, 7)], put=True)
    o = ops.array[0]
    assert (o.op_flag, o.local_offset, o.remote_offset, o.row_bytes, o.rows, o.local_stride, o.remote_stride) == \
        (1, 5 * 128, 7 * 384, 128, 3, 12 * 128, 128)
    exercise_layered_kv(kv, 6, seed=3, device="cpu")
    with pytest.raises(IndexError):
        kv.swap_out([(12, 0)])
    with pytest.raises(IndexError):
        kv.swap_in([(40, 0)])
    with pytest.raises(ValueError):
        kv.swap_out([(0, 5), (1, 5)])  # two blocks into one pool block
    kv.close()
    with pytest.raises(ValueError):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, compress="mxfp8", layers=2)
    # layers=0 is the cache of whole blocks, coalesced runs, plain batches
    plain = PagedKVOffload(client, 4, 8, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT, layers=0)
    assert plain.layers == 0 and tuple(plain.gpu_cache.shape) == (4, 2, 4, 8)
    ops = plain._ops([(0, 0), (1, 1), (3, 2)], put=True)
    assert ops.n == 2 and not getattr(ops, "strided", False)
    assert [(o.src_offset, o.dest_offset, o.bytes, o.op_flag) for o in ops.array[:2]] == [(0, 0, 256, 1), (384, 256, 128, 1)]
    before = api.counters()
    assert plain.swap_out([(0, 0), (1, 1), (3, 2)], async_=False) == 2
    after = api.counters()
    assert after["n_batch"] == before["n_batch"] + 1 and after["n_strided"] == before["n_strided"]
    plain.close()
