"""Strided converting ops (ocm_copy_onesided_quant_strided) on the host path: a CPU app
with host-memory pairs striped over three daemons. Every byte of both halves is compared
with the model (quant_strided_cases: the list expanded into plain converting rows, each
through the torch oracle)."""
import ctypes

import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from oncilla_amd.ops import mx8_record_reference, mx8_rows_reference
from quant_cases import UNIT, random_elems, read_local, roundtrip, write_local
from quant_strided_cases import (DTYPES, ROWS, STRIDES, Case, edge_case, exercise_layered_quant_kv, expand, halves,
                                 list_case, load_pair, record_up32, run_case, src_wire_bytes)
from strided_cases import SENTINEL


@pytest.fixture
def client(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(3, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        yield c


def _pair(c, local_bytes, remote_bytes):
    return c.alloc(api.OCM_REMOTE_RDMA, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                   stripe_unit=UNIT)


def test_struct_layout_and_oracle(native):
    assert ctypes.sizeof(api.OcmQuantStridedParams) == 56
    assert api.OcmQuantStridedParams.op_flag.offset == 48 and api.OcmQuantStridedParams.dtype.offset == 52
    assert len(api.COUNTER_KEYS) == 28  # the fixed array did not grow
    x = random_elems(3 * 64, torch.float16, seed=2).view(3, 64)
    recs = mx8_rows_reference(x)
    assert recs.shape == (3, 66) and recs.dtype == torch.uint8
    for r in range(3):
        assert torch.equal(recs[r], mx8_record_reference(x[r]))
    assert mx8_rows_reference(x[:0]).shape == (0, 66)
    with pytest.raises(ValueError):
        mx8_rows_reference(x.view(-1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("strides", STRIDES, ids=["-".join(s) for s in STRIDES])
@pytest.mark.parametrize("rows", ROWS)
def test_edge_rows(client, rows, strides, dtype):
    case = edge_case(rows, *strides)
    a = _pair(client, case.local_bytes, case.remote_bytes)
    assert len(a.remote_info()["extents"]) > 1
    run_case(a, case, dtype, seed=rows)
    a.free()


def test_mixed_list_async_and_counters(client):
    case = list_case(30)
    a = _pair(client, case.local_bytes, case.remote_bytes)
    before, before_all = api.quant_strided_counters(), api.counters()
    run_case(a, case, torch.bfloat16, seed=4,
             run=lambda ops: (a.quant_strided_batch(ops, torch.bfloat16, async_=True), a.wait()))
    after, after_all = api.quant_strided_counters(), api.counters()
    src, wire = src_wire_bytes(case.ops)
    assert set(before) == set(api.QUANT_STRIDED_COUNTER_KEYS)
    assert after == {"n_quant_strided": before["n_quant_strided"] + 1,
                     "n_quant_strided_ops": before["n_quant_strided_ops"] + 30,
                     "bytes_quant_strided_src": before["bytes_quant_strided_src"] + src,
                     "bytes_quant_strided_wire": before["bytes_quant_strided_wire"] + wire}
    # its own kind: neither a converting list nor a strided copy was counted
    assert all(after_all[k] == before_all[k] for k in ("n_quant", "n_quant_ops", "n_strided", "n_strided_ops"))
    a.free()


def test_empty_ops_do_nothing(client):
    LB, RB = 4096, 2 * UNIT
    a = _pair(client, LB, RB)
    case = Case(np.zeros((0, 7), dtype=np.int64), LB, RB)
    local, remote, _, _ = case.prepare(torch.float16, 1)
    load_pair(a, local, remote)
    before = api.quant_strided_counters()
    assert client.lib.ocm_copy_onesided_quant_strided(a.handle, None, 0, 0) == 0  # zero ops
    a.quant_strided_batch(np.zeros((0, 7), dtype=np.int64), torch.float16)
    # zero rows and zero elements, wherever they point and whatever their strides
    a.quant_strided_batch(np.array([[1, 0, 0, 64, 0, 128, 96], [0, 0, 0, 0, 5, 0, 0], [1, LB, RB, 0, 3, 8, 8],
                                    [0, 1 << 40, 1 << 40, 32, 0, 1, 1]]), torch.bfloat16, async_=True)
    a.wait()
    after = api.quant_strided_counters()
    assert after["n_quant_strided"] == before["n_quant_strided"] + 3
    assert after["n_quant_strided_ops"] == before["n_quant_strided_ops"] + 4
    assert after["bytes_quant_strided_src"] == before["bytes_quant_strided_src"]
    assert after["bytes_quant_strided_wire"] == before["bytes_quant_strided_wire"]
    got_l, got_r = halves(a, case)
    assert (got_l == SENTINEL).all() and (got_r == SENTINEL).all()
    a.free()


LB, RB = 8192, 4 * UNIT
GOOD = [1, 0, 0, 64, 2, 128, 96]
# name -> (the bad op [op_flag, local_offset, remote_offset, row_elems, rows, local_stride, remote_stride],
#          its dtype (None: float16), what the message must name)
RULES = {
    "dtype_is_bf16_or_fp16": ([1, 0, 0, 64, 2, 128, 96], 7, "element type"),
    "row_elems_multiple_of_32": ([1, 0, 0, 48, 2, 128, 96], None, "multiple of 32"),
    "row_elems_below_2_31": ([1, 0, 0, 1 << 31, 1, 0, 0], None, "2^31"),
    "rows_below_2_32": ([1, 0, 0, 64, 1 << 32, 128, 96], None, "2^32"),
    "local_offset_multiple_of_16": ([1, 8, 0, 64, 2, 128, 96], None, "local offset"),
    "local_stride_multiple_of_16": ([1, 0, 0, 64, 2, 136, 96], None, "local stride"),
    "remote_offset_multiple_of_32": ([0, 0, 16, 64, 2, 128, 96], None, "remote offset"),
    "remote_stride_multiple_of_32": ([0, 0, 0, 64, 2, 128, 80], None, "remote stride"),
    "local_stride_covers_the_row": ([1, 0, 0, 64, 2, 112, 96], None, "local stride"),
    "remote_stride_covers_the_record": ([1, 0, 0, 64, 2, 128, 64], None, "remote stride"),  # 64 < 66
    "local_range_one_row": ([1, LB - 112, 0, 64, 1, 0, 0], None, "local range"),
    "local_range_last_row": ([1, 0, 0, 64, 4, (LB - 128) // 3 // 16 * 16 + 16, 96], None, "local range"),
    "remote_range_one_row": ([0, 0, RB - 64, 64, 1, 0, 0], None, "remote range"),
    "remote_range_last_row": ([0, 0, 0, 64, 4, 128, (RB - 66) // 3 // 32 * 32 + 32], None, "remote range"),
    # checks that must not overflow: (rows - 1) * stride wraps 64 bits to something small
    "local_range_no_overflow_rows": ([1, 0, 0, 32, (1 << 32) - 1, 1 << 63, 64], None, "local range"),
    "remote_range_no_overflow_stride": ([1, 0, 0, 32, 5, 64, 1 << 62], None, "remote range"),  # 4 * 2^62 wraps to 0
    "local_range_no_overflow_sum": ([1, 0, 0, 32, 3, (1 << 63) + 64, 64], None, "local range"),
    "remote_range_no_overflow_sum": ([0, 0, 0, 32, 3, 64, (1 << 63) + 64], None, "remote range"),
}


@pytest.mark.parametrize("rule", RULES)
def test_validator_rule(client, rule):
    row, dtype, what = RULES[rule]
    a = _pair(client, LB, RB)
    lists = api.quant_strided_ops(np.array([GOOD, row], dtype=np.uint64), torch.float16)  # the bad op is op 1
    if dtype is not None:
        lists.array[1].dtype = dtype
    with pytest.raises(api.OcmError) as ei:
        a.quant_strided_batch(lists)
    msg = str(ei.value)
    assert "op 1" in msg and what in msg, msg
    a.free()


def test_arguments_and_exact_fits(client):
    a = _pair(client, LB, RB)
    lib = client.lib
    one = api.quant_strided_ops(np.array([GOOD]), torch.float16)
    assert lib.ocm_copy_onesided_quant_strided(a.handle, one.array, -1, 0) == -1 and "n_ops" in api.last_error()
    assert lib.ocm_copy_onesided_quant_strided(a.handle, None, 1, 0) == -1 and api.last_error()
    assert lib.ocm_copy_onesided_quant_strided(None, one.array, 1, 0) == -1 and api.last_error()
    loc = client.alloc(api.OCM_LOCAL_HOST, local_bytes=4096)  # a local allocation is no remote pair
    with pytest.raises(api.OcmError, match="remote pair"):
        loc.quant_strided_batch(np.array([GOOD]), torch.float16)
    loc.free()
    for other in (api.batch_ops(np.array([[1, 0, 0, 32]])), api.quant_ops(np.array([[1, 0, 0, 32]]), torch.float16),
                  api.strided_ops(np.array([[1, 0, 0, 16, 2, 16, 16]])), api.acc_ops(np.array([[0, 0, 4]]), torch.float32)):
        with pytest.raises(TypeError):
            a.quant_strided_batch(other)
    with pytest.raises(TypeError):
        a.quant_batch(one)
    with pytest.raises(ValueError):
        a.quant_strided_batch(np.array([GOOD]), torch.float32)
    # exact fits pass: the last row ends with its half on both sides
    write_local(a, 0, torch.zeros(LB // 2, dtype=torch.float16))
    a.quant_strided_batch(np.array([[1, 0, 0, 64, 4, (LB - 128) // 3 // 16 * 16, 96]]), torch.float16)
    a.quant_strided_batch(np.array([[1, LB - 128, RB - 96, 64, 1, 0, 0]]), torch.float16)
    a.free()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_plain_get_reads_one_row_of_a_strided_put(client, dtype):
    re, rows, rs = 1056, 5, record_up32(1056) + 32
    a = _pair(client, 2 * rows * 2 * re, 8 * UNIT)
    x = random_elems(rows * re, dtype, seed=8).view(rows, re)
    write_local(a, 0, x)
    a.quant_strided_batch(np.array([[1, 0, UNIT - 64, re, rows, 2 * re, rs]]), dtype)
    back = rows * 2 * re
    for r in (3, 0):  # one row's record, read by the plain converting call
        write_local(a, back, torch.full((re,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(np.array([[0, back, UNIT - 64 + r * rs, re]]), dtype)
        got = read_local(a, back, 2 * re).view(torch.int16)
        assert torch.equal(got, roundtrip(x[r]).view(torch.int16)), r
    # and the other way round: a strided get reads records that plain puts wrote
    a.quant_batch(np.array([[1, r * 2 * re, 4 * UNIT + r * rs, re] for r in range(rows)]), dtype)
    a.quant_strided_batch(np.array([[0, back, 4 * UNIT, re, rows, 2 * re, rs]]), dtype)
    assert torch.equal(read_local(a, back, rows * 2 * re).view(torch.int16), roundtrip(x).view(torch.int16).reshape(-1))
    a.free()


def test_kv_offload_layers_mxfp8_rows_cpu(client):
    kv = PagedKVOffload(client, 12, 40, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT, layers=3,
                        compress="mxfp8-rows")
    assert kv.block_bytes == 128 and kv.pool_block_bytes == 3 * 96  # 64 codes + 2 scale bytes, rounded up to 96
    assert tuple(kv.gpu_cache.shape) == (3, 12, 2, 4, 8)
    assert kv.alloc.local_bytes == 3 * 12 * 128 and kv.alloc.remote_size() == 40 * 3 * 96
    ops = kv._ops([(5, 7)], put=True)
    assert ops.n == 1 and ops.quant_strided
    o = ops.array[0]
    assert (o.op_flag, o.local_offset, o.remote_offset, o.row_elems, o.rows, o.local_stride, o.remote_stride, o.dtype) == \
        (1, 5 * 128, 7 * 288, 64, 3, 12 * 128, 96, api.OCM_QUANT_FP16)
    o = kv._ops([(7, 5)], put=False).array[0]
    assert (o.op_flag, o.local_offset, o.remote_offset) == (0, 5 * 128, 7 * 288)
    before = api.quant_strided_counters()
    exercise_layered_quant_kv(kv, 6, seed=3, device="cpu")
    after = api.quant_strided_counters()
    assert after["n_quant_strided"] == before["n_quant_strided"] + 12  # six swaps out, six in, one call each
    with pytest.raises(IndexError):
        kv.swap_out([(12, 0)])
    with pytest.raises(IndexError):
        kv.swap_in([(40, 0)])
    with pytest.raises(ValueError):
        kv.swap_out([(0, 5), (1, 5)])  # two blocks into one pool block
    kv.close()


def test_kv_offload_mxfp8_rows_needs_layers(client):
    with pytest.raises(ValueError, match="layers"):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, compress="mxfp8-rows")
    with pytest.raises(ValueError, match="layers"):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, compress="mxfp8-rows", layers=0)
    # the block-record value still cannot be layered, and says where to go
    with pytest.raises(ValueError, match="mxfp8-rows"):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, compress="mxfp8", layers=2)
    # the dtype and element-count checks of compress="mxfp8"
    with pytest.raises(ValueError):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float32, kind=api.OCM_REMOTE_RDMA, compress="mxfp8-rows", layers=2)
    with pytest.raises(ValueError):
        PagedKVOffload(client, 4, 4, (3, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, compress="mxfp8-rows", layers=2)
