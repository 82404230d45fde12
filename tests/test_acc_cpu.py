"""One-sided accumulate (ocm_copy_onesided_accumulate) on the host path: a CPU app with
host-memory pairs striped over three owners, and one pair on the network tier. The
accumulators are compared bit for bit with the torch oracle
(oncilla_amd.ops.accumulate_reference)."""
import ctypes

import numpy as np
import pytest
import torch

from acc_cases import (DTYPES, UNIT, AccList, assert_bits, edge_vectors, exercise_grad_accumulator, random_elems,
                       run_edge_vectors)
from oncilla_amd import api
from oncilla_amd.models import OffloadedGradAccumulator
from oncilla_amd.ops import accumulate_reference
from quant_cases import read_local, read_remote, write_local, write_remote


@pytest.fixture
def client(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(4, policy="stripe")  # the app on rank 0: pools stripe over the three others
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        yield c


def _pair(c, local_bytes, remote_bytes):
    return c.alloc(api.OCM_REMOTE_RDMA, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                   stripe_unit=UNIT)


def test_params_layout(native):
    assert ctypes.sizeof(api.OcmAccParams) == 32
    offs = {f: getattr(api.OcmAccParams, f).offset for f, _ in api.OcmAccParams._fields_}
    assert offs == {"local_offset": 0, "remote_offset": 8, "elems": 16, "dtype": 24, "scale": 28}
    assert (api.OCM_ACC_F32, api.OCM_ACC_BF16, api.OCM_ACC_FP16) == (1, 2, 3)
    assert [api.acc_dtype(d) for d in DTYPES] == [1, 2, 3] and api.acc_dtype("bf16") == 2 and api.acc_dtype(3) == 3
    with pytest.raises(ValueError):
        api.acc_dtype(torch.int32)
    ops = api.acc_ops(np.array([[16, 32, 8], [48, 64, 4]]), torch.float16, scale=-0.5)
    assert ops.acc and ops.n == 2
    assert (ops.array[1].local_offset, ops.array[1].remote_offset, ops.array[1].elems) == (48, 64, 4)
    assert ops.array[1].dtype == 3 and ops.array[1].scale == -0.5
    five = api.acc_ops(np.array([[16, 32, 8, 1, 0.25], [48, 64, 4, 2, 3.0]]))
    assert (five.array[0].dtype, five.array[0].scale, five.array[1].dtype, five.array[1].scale) == (1, 0.25, 2, 3.0)
    # an (n, 5) array carries its own dtypes and scales: arguments beside it would be ignored, so they are refused
    for kw in ({"dtype": torch.float32}, {"scale": 2.0}):
        with pytest.raises(ValueError):
            api.acc_ops(np.array([[16, 32, 8, 1, 0.25]]), **kw)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError):
            api.acc_dtype(bad)


def test_oracle_is_two_roundings():
    for dtype in DTYPES:
        edge_vectors(dtype)  # the builder asserts that the tell-tale differs from a fused result
    acc, x = random_elems(4096, torch.float32, 1), random_elems(4096, torch.bfloat16, 2)
    s = 1.0 / 3.0
    p = (x.float().double() * float(np.float32(s))).float()  # the product, rounded once
    assert_bits(accumulate_reference(acc, x, s), (acc.double() + p.double()).float(), "oracle")


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_vectors(client, dtype):
    a = _pair(client, 8192, 4 * UNIT)
    run_edge_vectors(a, dtype, stage=4096)
    a.free()


def test_sixty_op_list(client):
    al = AccList()
    a = _pair(client, al.local_bytes, al.remote_bytes)
    assert len(a.remote_info()["extents"]) == 3
    before = api.acc_counters()
    al.run(a, async_=True)
    after = api.acc_counters()
    assert after["n_acc"] == before["n_acc"] + 1 and after["n_acc_ops"] == before["n_acc_ops"] + 60
    assert after["bytes_acc"] == before["bytes_acc"] + 4 * al.elems
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_apply_the_rule_twice(client, dtype):
    n = 1028
    esize = torch.empty((), dtype=dtype).element_size()
    a = _pair(client, 16384, 4 * UNIT)
    acc, x = random_elems(n, torch.float32, 5), random_elems(n, dtype, 6)
    roff = UNIT - 64
    write_local(a, 0, x)
    write_remote(a, 8192, roff, acc)
    a.accumulate_batch(np.array([[0, roff, n]]), dtype, 1.0 / 3.0)
    write_local(a, 0, (-x))
    a.accumulate_batch(np.array([[0, roff, n]]), dtype, 3.0, async_=True)
    a.wait()
    want = accumulate_reference(accumulate_reference(acc, x, 1.0 / 3.0), -x, 3.0)
    assert_bits(read_remote(a, 8192, roff, 4 * n).view(torch.float32), want, str(dtype))
    assert torch.equal(read_local(a, 0, esize * n), (-x).view(torch.uint8))
    a.free()


def test_validation(client):
    a = _pair(client, 4096, 2 * UNIT)
    lib = client.lib

    def fails(row, dtype=torch.float32, scale=1.0, what=""):
        with pytest.raises(api.OcmError) as ei:
            dt = api.acc_dtype(dtype)
            a.accumulate_batch(np.array([[0, 0, 4, dt, 1.0], row + [dt, scale]]))  # the bad op is op 1
        msg = str(ei.value)
        assert "op 1" in msg and what in msg, msg

    fails([8, 64, 4], what="local offset 8 is not a multiple of 16")
    fails([0, 72, 4], what="remote offset 72 is not a multiple of 16")
    fails([0, 64, 6], what="multiple of 4")                      # elems % 4
    fails([0, 64, 1 << 31], what="below 2^31")                   # elems >= 2^31
    fails([4096 - 16, 64, 8], what="local range")                # 32 bytes at 4080 of 4096
    fails([4096 - 16, 64, 12], dtype=torch.bfloat16, what="local range")  # 24 bytes there
    fails([4112, 64, 0], what="local range")                     # an empty op past the end
    fails([0, 2 * UNIT - 16, 8], what="remote range")
    fails([0, 2 * UNIT + 16, 0], what="remote range")
    fails([0, 64, 4], scale=float("inf"), what="scale is not finite")
    fails([0, 64, 4], scale=float("-inf"), what="scale is not finite")
    fails([0, 64, 4], scale=float("nan"), what="scale is not finite")
    fails([0, 64, 4], scale=1e39, what="scale is not finite")   # overflows fp32
    for bad in (0, 4):
        two = api.acc_ops(np.array([[0, 0, 4], [0, 64, 4]]), torch.float32)
        two.array[1].dtype = bad
        with pytest.raises(api.OcmError, match=f"op 1: unknown element type {bad}"):
            a.accumulate_batch(two)
    # offsets at the top of the address space: no sum wraps around
    for field, what in (("local_offset", "local range"), ("remote_offset", "remote range")):
        two = api.acc_ops(np.array([[0, 0, 4], [0, 64, 4]]), torch.float32)
        setattr(two.array[1], field, 2 ** 64 - 16)
        with pytest.raises(api.OcmError, match=f"op 1: {what}"):
            a.accumulate_batch(two)
    big = api.acc_ops(np.array([[0, 0, 4], [0, 64, 2 ** 31 - 4]]), torch.float32)
    with pytest.raises(api.OcmError, match="op 1: local range"):
        a.accumulate_batch(big)
    arr = api.acc_ops(np.array([[0, 0, 4]]), torch.float16)
    assert lib.ocm_copy_onesided_accumulate(a.handle, arr.array, -1, 0) == -1 and "n_ops" in api.last_error()
    assert lib.ocm_copy_onesided_accumulate(a.handle, None, 1, 0) == -1 and api.last_error()
    assert lib.ocm_copy_onesided_accumulate(None, arr.array, 1, 0) == -1 and api.last_error()
    # a local allocation is no remote pair
    loc = client.alloc(api.OCM_LOCAL_HOST, local_bytes=4096)
    with pytest.raises(api.OcmError, match="remote pair"):
        loc.accumulate_batch(np.array([[0, 0, 4]]), torch.float32)
    loc.free()
    with pytest.raises(ValueError):
        a.accumulate_batch(np.array([[0, 0, 4]]), torch.int32)
    with pytest.raises(ValueError):
        a.accumulate_batch(arr, scale=2.0)  # a prepared list has its scales already
    with pytest.raises(ValueError):
        a.accumulate_batch(np.array([[0, 0, 4, 1, 1.0]]), dtype=torch.float32)
    for other in (api.batch_ops(np.array([[1, 0, 0, 32]])), api.quant_ops(np.array([[1, 0, 0, 32]]), torch.float16),
                  api.strided_ops(np.array([[1, 0, 0, 16, 1, 16, 16]]))):
        with pytest.raises(TypeError):
            a.accumulate_batch(other)
    # a failed call changed nothing and counted nothing; empty lists and empty ops succeed and count
    write_remote(a, 0, 0, torch.arange(64, dtype=torch.uint8))
    before = api.acc_counters()
    with pytest.raises(api.OcmError):
        a.accumulate_batch(np.array([[0, 0, 4], [8, 0, 4]]), torch.float32)
    assert api.acc_counters() == before
    assert lib.ocm_copy_onesided_accumulate(a.handle, None, 0, 0) == 0
    a.accumulate_batch(np.zeros((0, 3), dtype=np.int64), torch.bfloat16)
    a.accumulate_batch(np.array([[0, 0, 0], [4096, 2 * UNIT, 0]]), torch.bfloat16)  # empty ops, even at the very end
    after = api.acc_counters()
    assert after == {"n_acc": before["n_acc"] + 3, "n_acc_ops": before["n_acc_ops"] + 2, "bytes_acc": before["bytes_acc"]}
    assert torch.equal(read_remote(a, 128, 0, 64), torch.arange(64, dtype=torch.uint8))
    a.free()


def test_counters(client):
    a = _pair(client, 8192, 2 * UNIT)
    write_local(a, 0, torch.zeros(2048, dtype=torch.float32))
    a.put(0, 0, 8192)
    plain = api.counters()
    before = api.acc_counters()
    assert set(before) == {"n_acc", "n_acc_ops", "bytes_acc"} and len(api.COUNTER_KEYS) == 28
    a.accumulate_batch(np.array([[0, 0, 1024], [4096, 4096, 8], [0, 4160, 0]]), torch.float32)
    after = api.acc_counters()
    assert after == {"n_acc": before["n_acc"] + 1, "n_acc_ops": before["n_acc_ops"] + 3,
                     "bytes_acc": before["bytes_acc"] + 4 * 1032}
    now = api.counters()
    assert now["n_batch"] == plain["n_batch"] and now["n_quant"] == plain["n_quant"]
    a.free()


def test_network_tier(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(2, rank_env={0: {"OCM_HOST_ALIAS": "nodeA"}, 1: {"OCM_HOST_ALIAS": "nodeB"}})
    n = 300000  # more than one 1 MiB chunk of accumulators
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        a = c.alloc(api.OCM_REMOTE_RDMA, local_bytes=8 * n, remote_bytes=4 * n + 64)
        ext = a.remote_info()["extents"]
        assert len(ext) == 1 and ext[0]["net"]
        acc, x = random_elems(n, torch.float32, 7), random_elems(n, torch.bfloat16, 8)
        write_local(a, 0, x)
        write_remote(a, 4 * n, 64, acc)
        a.accumulate_batch(np.array([[0, 64, n]]), torch.bfloat16, -0.5)
        assert_bits(read_remote(a, 4 * n, 64, 4 * n).view(torch.float32), accumulate_reference(acc, x, -0.5), "network tier")
        a.free()


def test_grad_accumulator_cpu(client):
    torch.manual_seed(0)
    sizes = [5, 64, 1030]  # 5 and 1030 are padded to 4 elements
    for dtypes in ([torch.float32] * 3, [torch.bfloat16] * 3, [torch.bfloat16, torch.float32, torch.float16]):
        params = [torch.nn.Parameter(torch.randn(n).to(dt)) for n, dt in zip(sizes, dtypes)]
        acc = OffloadedGradAccumulator(params, client, stripe_unit=UNIT)
        assert acc.total_elems == 8 + 64 + 1032 and acc.alloc.remote_size() == 4 * acc.total_elems
        assert all(p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype for p in params)
        scales = [1.0, 0.25, 1.0 / 3.0, -3.0]
        grads = [[random_elems(n, dt, seed=100 * m + k) for k, (n, dt) in enumerate(zip(sizes, dtypes))] for m in range(4)]
        exercise_grad_accumulator(acc, params, grads, scales)
        # autograd accumulates into the installed views
        acc.zero_grads()
        sum((p.float() ** 2).sum() for p in params).backward()
        assert acc.add() >= 1
        for p, g in zip(params, acc.read()):
            assert_bits(g, accumulate_reference(torch.zeros(p.shape), p.grad, 1.0), "autograd")
        acc.close()
    with pytest.raises(ValueError):
        OffloadedGradAccumulator([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], client)


def test_train_example_with_accum(native, tool):
    import os
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rc, out = tool([sys.executable, os.path.join(repo, "examples", "train_offload.py"), "--steps", "30", "--accum", "2"])
    assert rc == 0 and "loss" in out and "30 steps" in out, out
