"""MXFP4 records (OCM_QUANT_MXFP4) on the host path: a CPU app with host-memory pairs striped
over three daemons. Records and decoded elements are compared byte for byte with the torch
oracle (oncilla_amd.ops.mx4_*_reference); the oracle itself against the format's rule."""
import ctypes

import numpy as np
import pytest
import torch

from mx4_cases import (DTYPES, TABLE_ROWS, MixedList, decode_table, edge_groups, exercise_kv, roundtrip, run_strided, sweep,
                       up32)
from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from oncilla_amd.ops import mx4_decode_reference, mx4_encode_reference, mx4_record_reference, mx4_rows_reference
from quant_cases import UNIT, random_elems, read_local, read_remote, run_nonfinite_put, write_local, write_remote

VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


@pytest.fixture
def client(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(3, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        yield c


def _pair(c, local_bytes, remote_bytes):
    return c.alloc(api.OCM_REMOTE_RDMA, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                   stripe_unit=UNIT)


def _nibbles(codes):
    return torch.stack([codes & 15, codes >> 4], dim=1).reshape(-1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_properties(dtype):
    xs = [random_elems(32 * 2048, dtype, seed) for seed in (1, 2)] + [sweep(dtype)[0]]
    for x in xs:
        codes, scales = mx4_encode_reference(x)
        assert codes.numel() == x.numel() // 2 and scales.numel() == x.numel() // 32
        g = x.double().view(-1, 32)
        amax = g.abs().amax(dim=1)
        e = scales.to(torch.float64) - 127
        scaled = amax * torch.pow(2.0, -e)
        nz = amax > 0
        clamped = scales == 0
        # the scale rule is minimal: the scaled maximum fits in 6, and with one less exponent it would not
        assert nz.any() and (scaled <= 6).all() and (scaled[nz & ~clamped] > 3).all()
        assert (scales[~nz] == 127).all() and (scales != 255).all()
        # decode of encode is within half a code step of x * 2^-e: the steps are 0.5 below 2, 1 below 4, 2 above
        nib = _nibbles(codes).to(torch.int64).view(-1, 32)
        y = g * torch.pow(2.0, -e)[:, None]
        val = torch.where((nib & 8) != 0, -VALUES[nib & 7], VALUES[nib & 7])
        half_step = torch.where(y.abs() > 4, 1.0, torch.where(y.abs() > 2, 0.5, 0.25))
        assert ((val - y).abs() <= half_step).all()
        assert (((nib & 8) != 0) == torch.signbit(g)).all()  # the sign survives, of -0 and of what rounds to it too
        back = mx4_decode_reference(codes, scales, dtype).double().view(-1, 32)
        finite = torch.isfinite(back)
        exact = val * torch.pow(2.0, e)[:, None]
        # the decoded element is value * 2^e wherever the element type holds it exactly (bf16 always does;
        # fp16 rounds below 2^-24 steps and overflows past 65504)
        holds = (exact.abs() <= 65504) & ((exact.abs() >= 2.0 ** -14) | (exact == 0)) if dtype == torch.float16 else finite
        assert (back[holds] == exact[holds]).all()
        assert (back[~nz] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_record_layout(dtype):
    x = torch.zeros(64, dtype=dtype)
    x[1], x[32 + 6] = 6.0, -1.0  # code 7 in the high nibble of byte 0; -1 = -4 * 2^-2: code 14, low nibble of byte 19
    rec = mx4_record_reference(x)
    want = torch.zeros(34, dtype=torch.uint8)
    want[0], want[19], want[32], want[33] = 0x70, 0x0E, 127, 125
    assert torch.equal(rec, want)
    rows = mx4_rows_reference(random_elems(3 * 64, dtype, 4).view(3, 64))
    assert rows.shape == (3, 34) and mx4_rows_reference(torch.zeros((0, 64), dtype=dtype)).shape == (0, 34)
    with pytest.raises(ValueError):
        mx4_encode_reference(torch.zeros(48, dtype=dtype))
    with pytest.raises(ValueError):
        mx4_encode_reference(torch.zeros(32))


def test_quant_bytes_fmt(native):
    assert api.quant_bytes(0, "mxfp4") == 0 and api.quant_bytes(32, "mxfp4") == 17 and api.quant_bytes(2048, "mxfp4") == 1088
    assert api.quant_bytes(1024) == api.quant_bytes(1024, "mxfp8") == 1056
    lib = api.load()
    assert lib.ocm_quant_bytes_fmt(64, api.OCM_QUANT_MXFP4) == 34 and lib.ocm_quant_bytes_fmt(64, api.OCM_QUANT_MXFP8) == 66
    assert lib.ocm_quant_bytes_fmt(64, 0x200) == 0 and lib.ocm_quant_bytes_fmt(64, 1) == 0
    assert ctypes.sizeof(api.OcmQuantParams) == 32 and ctypes.sizeof(api.OcmQuantStridedParams) == 56
    with pytest.raises(ValueError):
        api.quant_bytes(32, "mxfp6")


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_groups_put_raw_and_get(client, dtype):
    groups = edge_groups(dtype)
    a = _pair(client, 8192, 4 * UNIT)
    stage = 4096
    # two groups as one op whose 32 code bytes end a stripe unit: its scale bytes sit on the next one
    # (a record starts on a multiple of 32, so a single group's 17 bytes never cross a unit)
    pair = torch.cat([groups["rne_ties"], groups["largest"]])
    write_local(a, 0, pair)
    a.quant_batch(np.array([[1, 0, UNIT - 32, 64]]), dtype, format="mxfp4")
    assert torch.equal(read_remote(a, stage, UNIT - 32, 34), mx4_record_reference(pair))
    a.quant_batch(np.array([[0, 128, UNIT - 32, 64]]), dtype, format="mxfp4")
    assert torch.equal(read_local(a, 128, 128).view(torch.int16), roundtrip(pair).view(torch.int16))
    for k, (name, x) in enumerate(groups.items()):
        roff = UNIT + 32 + 32 * k
        write_local(a, 0, x)
        a.quant_batch(np.array([[1, 0, roff, 32]]), dtype, format="mxfp4")
        raw = read_remote(a, stage, roff, 17)
        codes, scales = mx4_encode_reference(x)
        assert torch.equal(raw[:16], codes), name
        assert raw[16] == scales[0], name
        write_local(a, 64, torch.full((32,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(np.array([[0, 64, roff, 32]]), dtype, format="mxfp4")
        got = read_local(a, 64, 64).view(torch.int16)
        assert torch.equal(got, mx4_decode_reference(codes, scales, dtype).view(torch.int16)), name
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_patterns_sweep(client, dtype):
    x, record, decoded = sweep(dtype)
    n = x.numel()
    a = _pair(client, 4 * n, (UNIT + record.numel() + UNIT) // UNIT * UNIT)
    write_local(a, 0, x)
    a.quant_batch(np.array([[1, 0, UNIT - 64, n]]), dtype, format="mxfp4")
    assert torch.equal(read_remote(a, 2 * n, UNIT - 64, record.numel()), record)
    a.quant_batch(np.array([[0, 0, UNIT - 64, n]]), dtype, format="mxfp4")
    assert torch.equal(read_local(a, 0, 2 * n).view(torch.int16), decoded.view(torch.int16))
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_table(client, dtype):
    t = decode_table()
    assert t.elems == 130560 and t.codes.numel() == 65280 and t.scales.numel() == 4080
    a = _pair(client, *t.bytes())
    t.run(a, dtype)
    a.free()
    a = _pair(client, *t.bytes(TABLE_ROWS))
    t.run_strided(a, dtype, TABLE_ROWS)
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_groups_stay_contained(client, dtype):
    # the put direction alone: E2M1 has no NaN code, and scale byte 255 is not specified
    a = _pair(client, 16384, 4 * UNIT)
    run_nonfinite_put(a, dtype, "mxfp4", mx4_record_reference)
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_mixed_sixty_op_list(client, dtype):
    ml = MixedList()
    a = _pair(client, ml.local_bytes, ml.remote_bytes)
    before = api.counters()
    ml.run(a, dtype, async_=(dtype == torch.float16))
    after = api.counters()
    elems = sum(o[3] for o in ml.ops)
    assert after["n_quant"] == before["n_quant"] + 1 and after["n_quant_ops"] == before["n_quant_ops"] + 60
    assert after["bytes_quant_src"] == before["bytes_quant_src"] + 2 * elems
    assert after["bytes_quant_wire"] == before["bytes_quant_wire"] + ml.wire_bytes()
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_put_rows_and_plain_get_of_one(client, dtype):
    a = _pair(client, 1 << 16, 8 * UNIT)
    before = api.quant_strided_counters()
    run_strided(a, dtype, rows=3, row_elems=2080, extra_stride=64, seed=8)
    after = api.quant_strided_counters()
    assert after["n_quant_strided"] == before["n_quant_strided"] + 2
    assert after["bytes_quant_strided_wire"] == before["bytes_quant_strided_wire"] + 2 * 3 * (1040 + 65)
    assert after["bytes_quant_strided_src"] == before["bytes_quant_strided_src"] + 2 * 3 * 4160
    run_strided(a, dtype, rows=1, row_elems=32, extra_stride=0, seed=9)
    a.free()


def test_validation(client):
    a = _pair(client, 4096, 2 * UNIT)
    mx4 = api.OCM_QUANT_MXFP4

    def fails(row, what, dt=api.OCM_QUANT_BF16 | mx4):
        two = api.quant_ops(np.array([[1, 0, 0, 32], row]), torch.bfloat16, "mxfp4")
        two.array[1].dtype = dt  # the bad op is op 1
        with pytest.raises(api.OcmError) as ei:
            a.quant_batch(two)
        msg = str(ei.value)
        assert "op 1: " in msg and what in msg, msg

    fails([1, 0, 64, 32], "unknown record format 0x200", dt=0x201)
    fails([1, 0, 64, 32], "unknown record format 0xff00", dt=0xFF02)
    fails([1, 0, 64, 32], "stray bits in dtype 0x10101", dt=0x10101)
    fails([1, 0, 64, 32], "stray bits in dtype 0x80000002", dt=0x80000002)
    fails([1, 0, 64, 32], "op 1: unknown element type 7", dt=7)       # today's message, as before formats
    fails([1, 0, 64, 32], "unknown element type 7", dt=7 | mx4)
    fails([1, 0, 64, 32], "unknown element type 0", dt=mx4)
    fails([1, 0, 64, 48], "multiple of 32")                           # elems % 32
    fails([1, 0, 64, 1 << 31], "below 2^31")
    fails([1, 8, 64, 32], "local offset 8 is not a multiple of 16")
    fails([0, 0, 80, 32], "remote offset 80 is not a multiple of 32")  # 16-aligned is not enough
    fails([1, 4096 - 32, 64, 32], "local range")
    fails([0, 0, 2 * UNIT - 16, 32], "remote offset")
    fails([0, 0, 2 * UNIT, 32], "remote range")
    # the record's own size decides the range: 2 * UNIT - 32 holds the 17 bytes of an MXFP4 record, not the 33 of MXFP8
    a.quant_batch(np.array([[1, 0, 2 * UNIT - 32, 32]]), torch.bfloat16, format="mxfp4")
    with pytest.raises(api.OcmError, match="op 0: remote range"):
        a.quant_batch(np.array([[1, 0, 2 * UNIT - 32, 32]]), torch.bfloat16)
    fails([0, 0, 2 * UNIT - 1024, 2048], r"remote range [7168,+1088)")  # 1024 code bytes fit, the 64 scale bytes do not

    def sfails(row, what, dt=api.OCM_QUANT_FP16 | mx4):
        two = api.quant_strided_ops(np.array([[1, 0, 0, 32, 1, 64, 32], row]), torch.float16, "mxfp4")
        two.array[1].dtype = dt
        with pytest.raises(api.OcmError) as ei:
            a.quant_strided_batch(two)
        msg = str(ei.value)
        assert "op 1: " in msg and what in msg, msg

    sfails([1, 0, 64, 32, 2, 64, 32], "unknown record format 0x300", dt=0x302)
    sfails([1, 0, 64, 32, 2, 64, 32], "stray bits in dtype 0x1000102", dt=0x1000102)
    sfails([1, 0, 64, 32, 2, 64, 32], "op 1: unknown element type 7", dt=7)
    sfails([1, 0, 64, 64, 2, 128, 48], "remote stride 48 is not a multiple of 32")
    sfails([1, 0, 64, 64, 2, 128, 32], "remote stride 32 is below the row's 34 bytes")   # 32 + 2
    sfails([1, 0, 64, 64, 2, 112, 64], "local stride 112 is below the row's 128 bytes")
    sfails([1, 0, 80, 64, 2, 128, 64], "remote offset 80 is not a multiple of 32")
    sfails([1, 0, 2 * UNIT - 64, 64, 2, 128, 64], "remote range")                       # the second row's scale bytes
    a.quant_strided_batch(np.array([[1, 0, 64, 64, 2, 128, 64]]), torch.float16, format="mxfp4")  # 34 <= 64 < 66
    with pytest.raises(api.OcmError, match="remote stride 64 is below the row's 66 bytes"):
        a.quant_strided_batch(np.array([[1, 0, 64, 64, 2, 128, 64]]), torch.float16)
    a.quant_strided_batch(np.array([[1, 0, 64, 64, 1, 0, 0]]), torch.float16, format="mxfp4")     # one row: no stride rule
    with pytest.raises(ValueError, match="'mxfp8' or 'mxfp4'"):
        a.quant_batch(np.array([[1, 0, 0, 32]]), torch.float16, format="mxfp6")
    # empty ops of the new format do nothing, even at the very end
    write_remote(a, 0, 0, torch.arange(64, dtype=torch.uint8))
    a.quant_batch(np.array([[1, 0, 0, 0], [0, 4096, 2 * UNIT, 0]]), torch.bfloat16, format="mxfp4")
    assert torch.equal(read_remote(a, 128, 0, 64), torch.arange(64, dtype=torch.uint8))
    a.free()


def test_kv_offload_mxfp4_cpu(client):
    kv = PagedKVOffload(client, 12, 40, (2, 4, 8), dtype=torch.bfloat16, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT,
                        compress="mxfp4")
    assert kv.block_bytes == 128 and kv.record_bytes == kv.pool_block_bytes == 64  # 32 code + 2 scale bytes, up to 32s
    assert kv.alloc.remote_size() == 40 * 64
    exercise_kv(kv, 5, seed=3, device="cpu")
    with pytest.raises(IndexError):
        kv.swap_out([(12, 0)])
    with pytest.raises(ValueError):
        kv.swap_out([(0, 5), (1, 5)])
    kv.close()
    rows = PagedKVOffload(client, 6, 20, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT,
                          compress="mxfp4-rows", layers=3)
    assert rows.record_bytes == 64 and rows.pool_block_bytes == 3 * 64 and rows.gpu_cache.shape == (3, 6, 2, 4, 8)
    exercise_kv(rows, 5, seed=4, device="cpu")
    rows.close()
    kw = dict(kind=api.OCM_REMOTE_RDMA)
    with pytest.raises(ValueError, match="cannot be combined with compress='mxfp4'.*use compress='mxfp4-rows'"):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, compress="mxfp4", layers=2, **kw)
    with pytest.raises(ValueError, match="compress='mxfp4-rows' keeps one record per layer: it needs layers > 0"):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, compress="mxfp4-rows", **kw)
    with pytest.raises(ValueError, match="needs float16 or bfloat16 blocks"):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float32, compress="mxfp4", **kw)
    with pytest.raises(ValueError, match="multiple of 32"):
        PagedKVOffload(client, 4, 4, (3, 8), dtype=torch.float16, compress="mxfp4", **kw)
    with pytest.raises(ValueError, match="unknown compression 'mxfp6'.*'mxfp4' or 'mxfp4-rows'"):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, compress="mxfp6", **kw)
