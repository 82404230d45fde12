"""Converting one-sided ops on the gfx950 kernel path (csrc/src/kernels/xfer_quant.hip):
records and decoded elements byte for byte against the torch oracle, with the pool in
the pinned host tier (one daemon) and striped over three owners (four daemons)."""
import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from oncilla_amd.ops import mx8_decode_reference, mx8_encode_reference, mx8_record_reference
from quant_cases import (UNIT, OpList, decode_table, edge_groups, exercise_kv, random_elems, read_local, read_remote,
                         roundtrip, run_nan_codes_get, run_nonfinite_put, run_sweep, sweep_bytes, write_local, write_remote)

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM


def _client(mesh_factory, n_daemons):
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _pair(c, local_bytes, remote_bytes, kind=api.OCM_REMOTE_GPU):
    return c.alloc(kind, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE, stripe_unit=UNIT)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_edge_groups(mesh_factory, n_daemons, dtype):
    groups = edge_groups(dtype)
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 16384, 4 * UNIT)
        stage = 8192
        # group k: elements at local 64 k, record at UNIT - 32 + 64 k (the first one's scale byte
        # sits on the next stripe unit), decoded again at local 4096 + 64 k
        puts, gets = [], []
        for k, x in enumerate(groups.values()):
            write_local(a, 64 * k, x)
            puts.append([1, 64 * k, UNIT - 32 + 64 * k, 32])
            gets.append([0, 4096 + 64 * k, UNIT - 32 + 64 * k, 32])
        a.quant_batch(np.array(puts), dtype)
        for k, (name, x) in enumerate(groups.items()):
            raw = read_remote(a, stage, UNIT - 32 + 64 * k, 33)
            assert torch.equal(raw, mx8_record_reference(x)), (name, raw.tolist())
        write_local(a, 4096, torch.full((2048,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(np.array(gets), dtype)
        for k, (name, x) in enumerate(groups.items()):
            got = read_local(a, 4096 + 64 * k, 64).view(torch.int16)
            assert torch.equal(got, roundtrip(x).view(torch.int16)), (name, got.tolist())
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_all_patterns_sweep(mesh_factory, n_daemons, dtype):
    # every finite 16-bit pattern through put_tile's multiply, clamp and packed convert, and back
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, *sweep_bytes())
        run_sweep(a, dtype)
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_decode_table(mesh_factory, n_daemons, dtype):
    # records no encoder wrote: every code under every scale byte through get_tile (ldexpf into fp32
    # subnormals and past the fp32 range, the narrowing of both, the NaN codes)
    t = decode_table()
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, *t.bytes())
        t.run(a, dtype)
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_nonfinite_groups_stay_contained(mesh_factory, n_daemons, dtype):
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 16384, 4 * UNIT)
        run_nonfinite_put(a, dtype, "mxfp8", mx8_record_reference)
        run_nan_codes_get(a, dtype)
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_sixty_op_list(mesh_factory, n_daemons, dtype):
    ol = OpList()
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, ol.local_bytes, ol.remote_bytes)
        info = a.remote_info()
        assert len(info["extents"]) == (1 if n_daemons == 1 else 3)
        before = api.counters()
        ol.run(a, dtype, async_=(dtype == torch.float16))
        after = api.counters()
        assert after["n_quant"] == before["n_quant"] + 1 and after["n_quant_ops"] == before["n_quant_ops"] + 60
        a.free()


@pytest.mark.parametrize("n_ops", [48, 49])  # the most ops the kernel arguments hold, and one more
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_list_at_the_inline_capacity(mesh_factory, n_daemons, n_ops):
    dtype = torch.bfloat16
    # 32 to 96 elements; ops of no elements first, last and two in a row; every third op a get
    sizes = [0 if i in (0, 5, 6, n_ops - 1) else 32 * (1 + i % 3) for i in range(n_ops)]
    lslot, rslot = 192, 128           # bytes per op in the local and in the remote half
    stage, base = n_ops * lslot, UNIT - 64  # the records cross two stripe-unit boundaries
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, stage + n_ops * rslot, 4 * UNIT)
        local = torch.full((stage,), 0x5A, dtype=torch.uint8)
        remote = torch.full((n_ops * rslot,), 0xA5, dtype=torch.uint8)
        rows, elems = [], {}
        for i, n in enumerate(sizes):
            put, lo, ro = i % 3 != 1, i * lslot, i * rslot
            rows.append([int(put), lo, base + ro, n])
            if n:
                elems[i] = x = random_elems(n, dtype, seed=500 + i)
                if put:
                    local[lo:lo + 2 * n] = x.view(torch.uint8)
                else:
                    remote[ro:ro + api.quant_bytes(n)] = mx8_record_reference(x)
        want_local, want_remote = local.clone(), remote.clone()
        for i, x in elems.items():
            put, lo, ro, n = rows[i][0], i * lslot, i * rslot, sizes[i]
            if put:
                want_remote[ro:ro + api.quant_bytes(n)] = mx8_record_reference(x)
            else:
                want_local[lo:lo + 2 * n] = roundtrip(x).view(torch.uint8)
        assert {r[0] for r in rows if r[3]} == {0, 1}
        write_remote(a, stage, base, remote)
        write_local(a, 0, local)
        before = api.counters()
        a.quant_batch(np.array(rows), dtype)
        after = api.counters()
        assert after["n_quant"] == before["n_quant"] + 1 and after["n_quant_ops"] == before["n_quant_ops"] + n_ops
        assert torch.equal(read_local(a, 0, stage), want_local)
        assert torch.equal(read_remote(a, stage, base, n_ops * rslot), want_remote)
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_host_path_records_match_kernel_path(mesh_factory, n_daemons):
    n = 32 * 150
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            x = random_elems(n, dtype, seed=21)
            x[:32] = edge_groups(dtype)["fp8_subnormals"]
            h = _pair(c, 4 * n, 8 * UNIT, kind=api.OCM_REMOTE_RDMA)  # host local half: the host codec
            d = _pair(c, 4 * n, 8 * UNIT)                            # device local half: the kernel
            roff = 2 * UNIT - 32 - n  # the codes cross one stripe-unit boundary, the scale bytes the next
            for a in (h, d):
                write_local(a, 0, x)
                a.quant_batch(np.array([[1, 0, roff, n]]), dtype)
            rec_h = read_remote(h, 2 * n, roff, api.quant_bytes(n))
            rec_d = read_remote(d, 2 * n, roff, api.quant_bytes(n))
            assert torch.equal(rec_h, rec_d) and torch.equal(rec_h, mx8_record_reference(x))
            # the host path's record through the kernel's decode, and the other way round
            write_remote(d, 2 * n, 4 * UNIT, rec_h)
            write_remote(h, 2 * n, 4 * UNIT, rec_d)
            for a in (h, d):
                a.quant_batch(np.array([[0, 0, 4 * UNIT, n]]), dtype)
                assert torch.equal(read_local(a, 0, 2 * n).view(torch.int16), roundtrip(x).view(torch.int16))
            h.free()
            d.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_async_list_signals_a_side_stream(mesh_factory, n_daemons):
    n, dtype = 32 * 160, torch.bfloat16
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 8 * n, 8 * UNIT)
        x = random_elems(2 * n, dtype, seed=33)
        write_remote(a, 4 * n, 0, mx8_record_reference(x[:n]))
        write_remote(a, 4 * n, 2 * UNIT + 32, mx8_record_reference(x[n:]))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lt = a.local_tensor(torch.int16)
            lt[:2 * n].fill_(0x5A5A)  # torch writes on the side stream; the list must start after them
            a.stream_wait()
            a.quant_batch(np.array([[0, 0, 0, n], [0, 2 * n, 2 * UNIT + 32, n]]), dtype, async_=True)
            a.stream_signal()
            got = lt[:2 * n].clone()  # read on the side stream, no host sync in between
        side.synchronize()
        assert torch.equal(got.cpu(), roundtrip(x).view(torch.int16))
        a.wait()
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_kv_offload_mxfp8_gpu(mesh_factory, n_daemons):
    with _client(mesh_factory, n_daemons) as c:
        kv = PagedKVOffload(c, 64, 256, (2, 8, 64), dtype=torch.float16, stripe_unit=UNIT, compress="mxfp8")
        assert kv.block_bytes == 2048 and kv.pool_block_bytes == 1056  # 1024 codes + 32 scale bytes
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # torch work on a non-default stream
            exercise_kv(kv, 8, seed=n_daemons, device="cuda:0")
        torch.cuda.synchronize()
        kv.close()
