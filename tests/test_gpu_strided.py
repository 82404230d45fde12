"""Strided one-sided ops on the gfx950 kernel path (csrc/src/kernels/xfer_strided.hip):
every byte of both halves against the numpy model, with the pool in the pinned host
tier (one daemon) and striped over three owners (four daemons, a 4 KiB stripe unit)."""
import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from strided_cases import (ROWS, UNIT, edge_case, exercise_layered_kv, expand, fill_pair, mixed_list, model, moved_bytes,
                           read_local, remote_bytes_of, run_case)

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM


def _client(mesh_factory, n_daemons):
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _pair(c, local_bytes, remote_bytes, n_daemons):
    assert local_bytes <= 1 << 20 and remote_bytes <= 1 << 20
    a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                stripe_unit=UNIT)
    assert len(a.remote_info()["extents"]) == (1 if n_daemons == 1 else 3)
    return a


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_edge_rows(mesh_factory, n_daemons, rows):
    with _client(mesh_factory, n_daemons) as c:
        # dense strides with offsets that agree mod 16, padded strides with offsets that do not, and the two crossed
        for dense, agree in ((True, True), (False, False), (True, False), (False, True)):
            case = edge_case(rows, dense, agree)
            a = _pair(c, case.local_bytes, case.remote_bytes, n_daemons)
            run_case(a, case, seed=rows)
            a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_rows_across_stripe_units(mesh_factory, n_daemons):
    # remote rows 1000 bytes further apart than they are long: no stride is a multiple of the 4 KiB
    # unit, rows start mid-unit, and rows of 4095 bytes and more straddle two owners
    case = edge_case(5, False, True, remote_gap=1000)
    assert all(p[6] % UNIT for p in case.puts)
    rows = [(p[2] + r * p[6], p[3]) for p in case.puts for r in range(p[4])]  # (remote start, bytes)
    assert all(s % UNIT for s, _ in rows)                                      # every row starts mid-unit
    assert sum(s // UNIT != (s + n - 1) // UNIT for s, n in rows) >= 15        # rows on two owners (or three)
    assert len({s // UNIT % 3 for s, _ in rows}) == 3                          # rows begin on every owner
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, case.local_bytes, case.remote_bytes, n_daemons)
        run_case(a, case, seed=7)
        a.free()


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_seventy_op_list(mesh_factory, n_daemons, async_):
    ops, local_bytes, remote_bytes = mixed_list(70)
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, local_bytes, remote_bytes, n_daemons)
        local, remote = fill_pair(a, local_bytes, remote_bytes, seed=3, random_remote=True)
        before = api.counters()
        a.strided_batch(ops, async_=async_)
        if async_:
            a.wait()
        after = api.counters()
        assert after["n_strided"] == before["n_strided"] + 1
        assert after["n_strided_ops"] == before["n_strided_ops"] + 70
        assert after["bytes_strided"] == before["bytes_strided"] + moved_bytes(ops)
        assert after["n_batch"] == before["n_batch"]  # its own launch, not a batch of rows
        want_l, want_r = model(local, remote, ops)
        assert np.array_equal(read_local(a, 0, local_bytes).numpy(), want_l)
        assert np.array_equal(remote_bytes_of(a, local_bytes, remote_bytes), want_r)
        a.free()


@pytest.mark.parametrize("n_ops", [24, 25])  # the most ops the kernel arguments hold, and one more
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_list_at_the_inline_capacity(mesh_factory, n_daemons, n_ops):
    # op i owns local [i * slot, +slot) and remote [i * rslot, +rslot): 1 to 3 rows of 16 to 5000 bytes,
    # odd paddings and offsets; ops of no bytes first, last and two in a row; every third op a get
    slot, rslot = 3 * 5008 + 64, 3 * 5016 + 64
    sizes = (16, 5000, 17, 4096, 255, 4097, 1024, 33)
    ops = []
    for i in range(n_ops):
        rb = 0 if i in (0, 7, 8, n_ops - 1) else sizes[i % len(sizes)]
        ops.append([i % 3 != 1, i * slot + i % 16, i * rslot + (5 * i) % 32, rb, 1 + i % 3, rb + (0, 1, 5)[i % 3],
                    rb + (0, 3, 16)[(i // 3) % 3]])
    ops[8][4] = 0  # an op without rows as well
    ops = np.asarray(ops, dtype=np.int64)
    local_bytes, remote_bytes = n_ops * slot, (n_ops * rslot + UNIT - 1) // UNIT * UNIT
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, local_bytes, remote_bytes, n_daemons)
        local, remote = fill_pair(a, local_bytes, remote_bytes, seed=n_ops, random_remote=True)
        before = api.counters()
        a.strided_batch(ops)
        after = api.counters()
        assert after["n_strided_ops"] == before["n_strided_ops"] + n_ops
        assert after["bytes_strided"] == before["bytes_strided"] + moved_bytes(ops)
        want_l, want_r = model(local, remote, ops)
        assert np.array_equal(read_local(a, 0, local_bytes).numpy(), want_l)
        assert np.array_equal(remote_bytes_of(a, local_bytes, remote_bytes), want_r)
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_same_bytes_as_a_batch_of_rows(mesh_factory, n_daemons):
    ops, local_bytes, remote_bytes = mixed_list(30, seed=5)  # 30 strided ops: more than the inline count too
    with _client(mesh_factory, n_daemons) as c:
        got = []
        for strided in (True, False):
            a = _pair(c, local_bytes, remote_bytes, n_daemons)
            fill_pair(a, local_bytes, remote_bytes, seed=4, random_remote=True)
            if strided:
                a.strided_batch(ops)
            else:
                a.batch(api.batch_ops(expand(ops)))
            got.append((read_local(a, 0, local_bytes).numpy(), remote_bytes_of(a, local_bytes, remote_bytes)))
            a.free()
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_kv_offload_layers_gpu(mesh_factory, n_daemons):
    with _client(mesh_factory, n_daemons) as c:
        kv = PagedKVOffload(c, 32, 64, (2, 8, 64), dtype=torch.float16, stripe_unit=UNIT, layers=3)
        assert kv.block_bytes == 2048 and kv.pool_block_bytes == 3 * 2048
        assert tuple(kv.gpu_cache.shape) == (3, 32, 2, 8, 64) and kv.gpu_cache.is_cuda
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # torch work on a non-default stream
            exercise_layered_kv(kv, 6, seed=n_daemons, device="cuda:0")
        torch.cuda.synchronize()
        kv.close()
