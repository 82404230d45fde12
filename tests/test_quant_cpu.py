"""Converting one-sided ops (ocm_copy_onesided_quant) on the host path: a CPU app with
host-memory pairs striped over three daemons. Records and decoded elements are compared
byte for byte with the torch oracle (oncilla_amd.ops.mx8_*_reference)."""
import ctypes

import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from oncilla_amd.ops import mx8_decode_reference, mx8_encode_reference, mx8_record_reference
from quant_cases import (TABLE_ROWS, UNIT, OpList, decode_table, edge_groups, exercise_kv, random_elems, read_local,
                         read_remote, roundtrip, run_nan_codes_get, run_nonfinite_put, run_sweep, sweep, sweep_bytes,
                         write_local, write_remote)

DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture
def client(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(3, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        yield c


def _pair(c, local_bytes, remote_bytes):
    return c.alloc(api.OCM_REMOTE_RDMA, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                   stripe_unit=UNIT)


@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_properties(dtype):
    for seed in (1, 2, 3):
        x = random_elems(32 * 2048, dtype, seed)
        codes, scales = mx8_encode_reference(x)
        g = x.float().view(-1, 32)
        amax = g.abs().amax(dim=1)
        e = scales.to(torch.float64) - 127
        scaled = amax.double() * torch.pow(2.0, -e)
        nz = amax > 0
        assert nz.any() and (scaled[nz] > 224).all() and (scaled[nz] <= 448).all()
        assert (scales[~nz] == 127).all() and (scales != 255).all()
        assert not ((codes & 0x7F) == 0x7F).any()  # no NaN codes
        back = mx8_decode_reference(codes, scales, dtype).float().view(-1, 32)
        err = (back.double() - g.double()).abs().amax(dim=1)
        assert (err[nz] <= amax[nz].double() / 14).all()
        assert (back[~nz] == 0).all()


def test_quant_bytes(native):
    assert api.quant_bytes(0) == 0 and api.quant_bytes(32) == 33 and api.quant_bytes(1024) == 1056
    assert ctypes.sizeof(api.OcmQuantParams) == 32


@pytest.mark.parametrize("dtype", DTYPES)
def test_edge_groups_put_raw_and_get(client, dtype):
    groups = edge_groups(dtype)
    a = _pair(client, 8192, 4 * UNIT)
    stage = 4096
    for k, (name, x) in enumerate(groups.items()):
        roff = UNIT - 32 + 64 * k  # the first record's scale byte sits on the next stripe unit
        write_local(a, 0, x)
        a.quant_batch(np.array([[1, 0, roff, 32]]), dtype)
        raw = read_remote(a, stage, roff, 33)
        codes, scales = mx8_encode_reference(x)
        assert torch.equal(raw[:32], codes), name
        assert raw[32] == scales[0], name
        write_local(a, 64, torch.full((32,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(np.array([[0, 64, roff, 32]]), dtype)
        got = read_local(a, 64, 64).view(torch.int16)
        assert torch.equal(got, mx8_decode_reference(codes, scales, dtype).view(torch.int16)), name
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_quant_get_of_oracle_records(client, dtype):
    n = 32 * 100
    x = random_elems(n, dtype, seed=5)
    a = _pair(client, 4 * n, 4 * UNIT)
    write_remote(a, 2 * n, UNIT - 320, mx8_record_reference(x))  # the codes cross a unit boundary
    a.quant_batch(np.array([[0, 0, UNIT - 320, n]]), dtype)
    assert torch.equal(read_local(a, 0, 2 * n).view(torch.int16), roundtrip(x).view(torch.int16))
    a.free()


def test_sweep_strength():
    """What the all-patterns sweep reaches, so that it cannot be hollowed out later: floors under
    the measured 212 codes and 248 scale bytes (bf16) and 174 codes (fp16)."""
    x, record, _ = sweep(torch.bfloat16)
    n = x.numel()
    assert n == 131072 and record.numel() == n + n // 32
    codes, scales = record[:n].unique(), record[n:].unique()
    print("bf16 sweep:", codes.numel(), "codes,", scales.numel(), "scale bytes")
    assert codes.numel() >= 200 and scales.numel() >= 240 and int(scales[0]) == 0
    x, record, _ = sweep(torch.float16)
    codes, scales = record[:n].unique(), record[n:].unique()
    print("fp16 sweep:", codes.numel(), "codes,", scales.numel(), "scale bytes")
    assert codes.numel() >= 170
    # both halves of the sweep hold every finite pattern once
    for dtype, finite in ((torch.bfloat16, 65536 - 2 * 128), (torch.float16, 65536 - 2 * 1024)):
        p = sweep(dtype)[0].view(torch.int16).to(torch.int32) & 0xFFFF
        for half in (p[:65536], p[65536:]):
            assert half.unique().numel() == finite and int((half == 0).sum()) == 65536 - finite + 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_patterns_sweep(client, dtype):
    a = _pair(client, *sweep_bytes())
    run_sweep(a, dtype)
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_table(client, dtype):
    t = decode_table()
    assert t.elems == 65536 and t.record().numel() == 67584 and int(t.nan.sum()) == 512
    a = _pair(client, *t.bytes())
    t.run(a, dtype)
    a.free()
    a = _pair(client, *t.bytes(TABLE_ROWS))
    t.run_strided(a, dtype, TABLE_ROWS)
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_groups_stay_contained(client, dtype):
    a = _pair(client, 16384, 4 * UNIT)
    run_nonfinite_put(a, dtype, "mxfp8", mx8_record_reference)
    run_nan_codes_get(a, dtype)
    a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sixty_op_list(client, dtype):
    ol = OpList()
    a = _pair(client, ol.local_bytes, ol.remote_bytes)
    before = api.counters()
    ol.run(a, dtype, async_=(dtype == torch.float16))
    after = api.counters()
    elems = sum(o[3] for o in ol.ops)
    assert after["n_quant"] == before["n_quant"] + 1 and after["n_quant_ops"] == before["n_quant_ops"] + 60
    assert after["bytes_quant_src"] == before["bytes_quant_src"] + 2 * elems
    assert after["bytes_quant_wire"] == before["bytes_quant_wire"] + elems + elems // 32
    a.free()


def test_validation(client):
    a = _pair(client, 4096, 2 * UNIT)
    lib = client.lib

    def fails(row, dtype=torch.bfloat16, what=""):
        with pytest.raises(api.OcmError) as ei:
            a.quant_batch(np.array([[1, 0, 0, 32], row]), dtype)  # the bad op is op 1
        msg = str(ei.value)
        assert "op 1" in msg and what in msg, msg

    fails([1, 0, 64, 48], what="multiple of 32")                 # elems % 32
    fails([1, 0, 64, 1 << 31], what="below 2^31")                # elems >= 2^31
    fails([1, 8, 64, 32], what="local offset")                   # local_offset % 16
    fails([0, 0, 80, 32], what="remote offset")                  # remote_offset % 32
    fails([1, 4096 - 32, 64, 32], what="local range")            # 64 bytes at 4064 of 4096
    fails([1, 4096, 64, 32], what="local range")
    fails([0, 0, 2 * UNIT - 32, 32], what="remote range")        # the scale byte falls outside
    fails([0, 0, 2 * UNIT, 32], what="remote range")
    two = api.quant_ops(np.array([[1, 0, 0, 32], [1, 0, 64, 32]]), torch.bfloat16)
    two.array[1].dtype = 7                                       # unknown element type
    with pytest.raises(api.OcmError, match="op 1: unknown element type 7"):
        a.quant_batch(two)
    arr = api.quant_ops(np.array([[1, 0, 0, 32]]), torch.float16)
    assert lib.ocm_copy_onesided_quant(a.handle, arr.array, -1, 0) == -1 and "n_ops" in api.last_error()
    assert lib.ocm_copy_onesided_quant(a.handle, None, 1, 0) == -1 and api.last_error()
    assert lib.ocm_copy_onesided_quant(None, arr.array, 1, 0) == -1 and api.last_error()
    # a local allocation is no remote pair
    loc = client.alloc(api.OCM_LOCAL_HOST, local_bytes=4096)
    with pytest.raises(api.OcmError, match="remote pair"):
        loc.quant_batch(np.array([[1, 0, 0, 32]]), torch.float16)
    loc.free()
    with pytest.raises(ValueError):
        a.quant_batch(np.array([[1, 0, 0, 32]]), torch.float32)
    with pytest.raises(TypeError):
        a.quant_batch(api.batch_ops(np.array([[1, 0, 0, 32]])))
    # nothing to do: fine, and nothing is touched
    write_remote(a, 0, 0, torch.arange(64, dtype=torch.uint8))
    assert lib.ocm_copy_onesided_quant(a.handle, None, 0, 0) == 0
    a.quant_batch(np.zeros((0, 4), dtype=np.int64), torch.bfloat16)
    a.quant_batch(np.array([[1, 0, 0, 0], [0, 4096, 2 * UNIT, 0]]), torch.bfloat16)  # empty ops, even at the very end
    assert torch.equal(read_remote(a, 128, 0, 64), torch.arange(64, dtype=torch.uint8))
    a.free()


def test_kv_offload_mxfp8_cpu(client):
    kv = PagedKVOffload(client, 12, 40, (2, 4, 8), dtype=torch.bfloat16, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT,
                        compress="mxfp8")
    assert kv.block_bytes == 128 and kv.pool_block_bytes == 96  # 64 codes + 2 scale bytes, rounded up to 32
    assert kv.alloc.remote_size() == 40 * 96
    exercise_kv(kv, 6, seed=3, device="cpu")
    with pytest.raises(IndexError):
        kv.swap_out([(12, 0)])
    with pytest.raises(IndexError):
        kv.swap_in([(40, 0)])
    with pytest.raises(ValueError):
        kv.swap_out([(0, 5), (1, 5)])  # two blocks into one pool block
    kv.close()
    with pytest.raises(ValueError):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float32, kind=api.OCM_REMOTE_RDMA, compress="mxfp8")
    with pytest.raises(ValueError):
        PagedKVOffload(client, 4, 4, (3, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, compress="mxfp8")
    with pytest.raises(ValueError):
        PagedKVOffload(client, 4, 4, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, compress="zip")
    # the default is untouched: plain blocks, coalesced runs
    plain = PagedKVOffload(client, 4, 8, (2, 4, 8), dtype=torch.float16, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT)
    assert plain.compress is None and plain.pool_block_bytes == plain.block_bytes == 128
    assert plain.swap_out([(0, 0), (1, 1), (2, 2)], async_=False) == 1
    plain.close()
