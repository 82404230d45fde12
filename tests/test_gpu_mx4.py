"""MXFP4 records on the gfx950 kernel path (the _mx4 tile bodies of csrc/src/kernels/quant_tile.h,
reached from xfer_quant.hip and xfer_quant_strided.hip): records and decoded elements byte for
byte against the torch oracle, with the pool in the pinned host tier (one daemon) and striped
over three owners (four daemons, a 4 KiB stripe unit)."""
import numpy as np
import pytest
import torch

from mx4_cases import (DTYPES, TABLE_ROWS, MixedList, decode_table, edge_groups, exercise_kv, roundtrip, run_strided, sweep,
                       up32)
from oncilla_amd import api
from oncilla_amd.models import PagedKVOffload
from oncilla_amd.ops import mx4_record_reference
from quant_cases import UNIT, random_elems, read_local, read_remote, run_nonfinite_put, write_local, write_remote

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM


def _client(mesh_factory, n_daemons):
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _pair(c, local_bytes, remote_bytes, n_daemons, kind=api.OCM_REMOTE_GPU):
    a = c.alloc(kind, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE, stripe_unit=UNIT)
    assert len(a.remote_info()["extents"]) == (1 if n_daemons == 1 else 3)
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_edge_groups(mesh_factory, n_daemons, dtype):
    groups = edge_groups(dtype)
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 16384, 4 * UNIT, n_daemons)
        stage = 8192
        # op 0: two groups whose 32 code bytes end a stripe unit, so the scale bytes sit on the next one
        # (a record starts on a multiple of 32: a single group's 17 bytes never cross a unit). Then group
        # k as a 32-element op: elements at local 128 + 64 k, record at UNIT + 32 + 32 k, decoded again
        # 4096 further on.
        pair = torch.cat([groups["rne_ties"], groups["largest"]])
        write_local(a, 0, pair)
        puts, gets = [[1, 0, UNIT - 32, 64]], [[0, 4096, UNIT - 32, 64]]
        for k, x in enumerate(groups.values()):
            write_local(a, 128 + 64 * k, x)
            puts.append([1, 128 + 64 * k, UNIT + 32 + 32 * k, 32])
            gets.append([0, 4096 + 128 + 64 * k, UNIT + 32 + 32 * k, 32])
        a.quant_batch(np.array(puts), dtype, format="mxfp4")
        raw = read_remote(a, stage, UNIT - 32, 34)
        assert torch.equal(raw, mx4_record_reference(pair)), ("pair", raw.tolist())
        for k, (name, x) in enumerate(groups.items()):
            raw = read_remote(a, stage, UNIT + 32 + 32 * k, 17)
            assert torch.equal(raw, mx4_record_reference(x)), (name, raw.tolist(), mx4_record_reference(x).tolist())
        write_local(a, 4096, torch.full((2048,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(np.array(gets), dtype, format="mxfp4")
        assert torch.equal(read_local(a, 4096, 128).view(torch.int16), roundtrip(pair).view(torch.int16))
        for k, (name, x) in enumerate(groups.items()):
            got = read_local(a, 4096 + 128 + 64 * k, 64).view(torch.int16)
            assert torch.equal(got, roundtrip(x).view(torch.int16)), (name, got.tolist())
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_all_patterns_sweep(mesh_factory, n_daemons, dtype):
    x, record, decoded = sweep(dtype)
    n = x.numel()
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 4 * n, (2 * UNIT + record.numel()) // UNIT * UNIT, n_daemons)
        write_local(a, 0, x)
        a.quant_batch(np.array([[1, 0, UNIT - 64, n]]), dtype, format="mxfp4")
        got = read_remote(a, 2 * n, UNIT - 64, record.numel())
        bad = (got != record).nonzero().reshape(-1)
        assert bad.numel() == 0, (bad.numel(), [(int(i), int(got[i]), int(record[i])) for i in bad[:12]])
        write_local(a, 0, torch.full((n,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(np.array([[0, 0, UNIT - 64, n]]), dtype, format="mxfp4")
        got = read_local(a, 0, 2 * n).view(torch.int16)
        want = decoded.view(torch.int16)
        bad = (got != want).nonzero().reshape(-1)
        assert bad.numel() == 0, (bad.numel(), [(int(i), hex(int(got[i]) & 0xFFFF), hex(int(want[i]) & 0xFFFF)) for i in bad[:12]])
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_decode_table(mesh_factory, n_daemons, dtype):
    # records no encoder wrote: every code byte under every scale byte 0..254 through get_tile_mx4
    # (the nibble-to-lane mapping, the scale operand of the packed converts at both ends)
    t = decode_table()
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, *t.bytes(), n_daemons)
        t.run(a, dtype)
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_nonfinite_groups_stay_contained(mesh_factory, n_daemons, dtype):
    # the put direction alone: E2M1 has no NaN code, and scale byte 255 is not specified
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 16384, 4 * UNIT, n_daemons)
        run_nonfinite_put(a, dtype, "mxfp4", mx4_record_reference)
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_tile_edges(mesh_factory, n_daemons, dtype):
    # a tile short of a group, a whole tile, a group more, two tiles and a group; each twice: once its
    # codes cross a stripe-unit boundary (the record starts 64 bytes before one) and once its scale
    # bytes do (they start 16 or 32 bytes before one). At these sizes the code bytes are shorter than
    # a stripe unit, so one record cannot do both; test_host_path_records_match_kernel_path has one.
    sizes = [2048 - 32, 2048, 2048 + 32, 4096 + 32]
    gets_at, stage = 1 << 16, 3 << 16
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 1 << 18, 8 * len(sizes) * UNIT, n_daemons)
        xs, puts, gets, lo = [], [], [], 0
        for i, n in enumerate(sizes):
            unit0 = 8 * i * UNIT
            cross_codes = unit0 + 2 * UNIT - 64
            cross_scales = unit0 + 6 * UNIT - (16 if (n // 2) % 32 else 32) - n // 2
            assert cross_codes // UNIT < (cross_codes + n // 2 - 1) // UNIT
            assert (cross_scales + n // 2) // UNIT < (cross_scales + n // 2 + n // 32 - 1) // UNIT
            for ro in (cross_codes, cross_scales):
                assert ro % 32 == 0
                xs.append(random_elems(n, dtype, seed=40 + len(xs)))
                write_local(a, lo, xs[-1])
                write_remote(a, stage, ro - 32, torch.full((api.quant_bytes(n, "mxfp4") + 64,), 0xA5, dtype=torch.uint8))
                puts.append([1, lo, ro, n])
                gets.append([0, gets_at + lo, ro, n])
                lo += 2 * n
        assert lo <= gets_at
        a.quant_batch(np.array(puts), dtype, format="mxfp4")
        for x, (_, _, ro, n) in zip(xs, puts):
            # 32 bytes before the record and after it keep the fill
            got = read_remote(a, stage, ro - 32, api.quant_bytes(n, "mxfp4") + 64)
            fill = torch.full((32,), 0xA5, dtype=torch.uint8)
            want = torch.cat([fill, mx4_record_reference(x), fill])
            assert torch.equal(got, want), (n, ro, (got != want).nonzero()[:8].reshape(-1).tolist())
        write_local(a, gets_at, torch.full((lo,), 0x5A, dtype=torch.uint8))
        a.quant_batch(np.array(gets), dtype, format="mxfp4")
        for x, (_, l, _, n) in zip(xs, gets):
            assert torch.equal(read_local(a, l, 2 * n).view(torch.int16), roundtrip(x).view(torch.int16)), n
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_mixed_list(mesh_factory, n_daemons, dtype):
    ml = MixedList()  # both formats, both directions, two empty ops
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, ml.local_bytes, ml.remote_bytes, n_daemons)
        before = api.counters()
        ml.run(a, dtype, async_=(dtype == torch.float16))
        after = api.counters()
        assert after["n_quant"] == before["n_quant"] + 1 and after["n_quant_ops"] == before["n_quant_ops"] + 60
        assert after["bytes_quant_wire"] == before["bytes_quant_wire"] + ml.wire_bytes()
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_host_path_records_match_kernel_path(mesh_factory, n_daemons):
    n = 32 * 300  # 4800 code bytes: more than a stripe unit
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            x = random_elems(n, dtype, seed=21)
            x[:32] = edge_groups(dtype)["rne_ties"]
            x[32:64] = edge_groups(dtype)["to_zero_and_half"]
            h = _pair(c, 4 * n, 8 * UNIT, n_daemons, kind=api.OCM_REMOTE_RDMA)  # host local half: the host codec
            d = _pair(c, 4 * n, 8 * UNIT, n_daemons)                            # device local half: the kernel
            roff = 2 * UNIT - 32 - n // 2  # the codes cross one stripe-unit boundary, the scale bytes the next
            for a in (h, d):
                write_local(a, 0, x)
                a.quant_batch(np.array([[1, 0, roff, n]]), dtype, format="mxfp4")
            rb = api.quant_bytes(n, "mxfp4")
            rec_h, rec_d = read_remote(h, 2 * n, roff, rb), read_remote(d, 2 * n, roff, rb)
            assert torch.equal(rec_h, rec_d) and torch.equal(rec_h, mx4_record_reference(x))
            # the host path's record through the kernel's decode, and the other way round
            write_remote(d, 2 * n, 4 * UNIT, rec_h)
            write_remote(h, 2 * n, 4 * UNIT, rec_d)
            for a in (h, d):
                a.quant_batch(np.array([[0, 0, 4 * UNIT, n]]), dtype, format="mxfp4")
                assert torch.equal(read_local(a, 0, 2 * n).view(torch.int16), roundtrip(x).view(torch.int16))
            h.free()
            d.free()


@pytest.mark.parametrize("extra_stride", [0, 96])  # the rounded record size itself, and a larger stride
@pytest.mark.parametrize("row_elems", [32, 2080])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_strided_rows(mesh_factory, n_daemons, rows, row_elems, extra_stride):
    dtype = DTYPES[(rows + row_elems // 32 + extra_stride // 96) % 2]
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 1 << 16, 4 * UNIT, n_daemons)
        before = api.quant_strided_counters()
        run_strided(a, dtype, rows, row_elems, extra_stride, seed=rows + row_elems, base=UNIT - 32 if row_elems > 32 else UNIT - 32 * rows + 32)
        after = api.quant_strided_counters()
        assert after["n_quant_strided"] == before["n_quant_strided"] + 2
        assert after["bytes_quant_strided_wire"] == before["bytes_quant_strided_wire"] + 2 * rows * api.quant_bytes(row_elems, "mxfp4")
        a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_decode_table_rows(mesh_factory, n_daemons, dtype):
    # the decode table through the strided kernel's own tile location: 30 rows of 4352 elements
    t = decode_table()
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, *t.bytes(TABLE_ROWS), n_daemons)
        t.run_strided(a, dtype, TABLE_ROWS)
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_kv_offload_mxfp4_rows_gpu(mesh_factory, n_daemons):
    with _client(mesh_factory, n_daemons) as c:
        kv = PagedKVOffload(c, 16, 64, (2, 8, 64), dtype=torch.float16, stripe_unit=UNIT, compress="mxfp4-rows", layers=3)
        assert kv.block_bytes == 2048 and kv.record_bytes == up32(512 + 32) == 544 and kv.pool_block_bytes == 3 * 544
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):  # torch work on a non-default stream
            exercise_kv(kv, 4, seed=n_daemons, device="cuda:0")
        torch.cuda.synchronize()
        kv.close()
