"""Pooled lookups (ocm_copy_onesided_bag) on the host path: a CPU app with host-memory pairs, on one
daemon and striped over three owners with a small stripe unit. The cases of test_gpu_bag.py at their
smallest sizes, every byte of both halves compared with the numpy model (bag_cases.model), skip
reporting included."""
import ctypes

import numpy as np
import pytest
import torch

from bag_cases import (DTYPES, ESIZE, F32, IN_FLIGHT, LENGTHS, MEAN, NONE, SUM, UNIT, Layout, bag_lengths, bag_sum,
                       bag_sum_fma, clamp_layout, fma_case, grid_values, mixed_layout, model, narrow, nominal, order_layout,
                       order_values, run_layout, shapes_layout, widen, window_layout)
from oncilla_amd import api
from oncilla_amd.models import RemoteEmbedding

N_DAEMONS = [1, 4]
ITYPES = [api.OCM_INDEX_I32, api.OCM_INDEX_I64]


@pytest.fixture(params=N_DAEMONS)
def client(request, mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(request.param, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        c.n_daemons = request.param
        yield c


def _pair(c, local_bytes, remote_bytes):
    assert local_bytes <= 1 << 20 and remote_bytes <= 1 << 20
    a = c.alloc(api.OCM_REMOTE_RDMA, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                stripe_unit=UNIT)
    assert len(a.remote_info()["extents"]) == (1 if c.n_daemons == 1 else 3)
    return a


def _run(c, lay, seed=1, async_=False):
    a = _pair(c, lay.local_bytes, lay.remote_bytes)
    skipped, err = run_layout(a, lay, seed=seed, async_=async_)
    a.free()
    return skipped, err


def test_struct_layout_and_names(native):
    assert ctypes.sizeof(api.OcmBagParams) == 104
    assert api.OcmBagParams.index_offset.offset == 64 and api.OcmBagParams.weights_offset.offset == 80
    assert api.OcmBagParams.index_type.offset == 88 and api.OcmBagParams.reserved.offset == 100
    assert (api.OCM_BAG_SUM, api.OCM_BAG_MEAN) == (0, 1) and (SUM, MEAN) == (0, 1) and IN_FLIGHT == 4
    assert api.BAG_COUNTER_KEYS == ["n_bag", "n_bag_ops", "n_bag_bags", "n_bag_ids", "bytes_bag"]
    assert list(api.bag_counters()) == api.BAG_COUNTER_KEYS
    # the counters of the other calls are what they were
    assert len(api.COUNTER_KEYS) == 28 and len(api.indexed_counters()) == 5
    ops = api.bag_ops([[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, NONE], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]], torch.bfloat16, api.OCM_INDEX_I32,
                      ["sum", "mean"])
    o = ops.array[0]
    assert ops.bag and ops.n == 2
    assert (o.local_offset, o.remote_offset, o.row_elems, o.bags, o.ids, o.local_stride, o.remote_stride, o.remote_rows,
            o.index_offset, o.offsets_offset, o.weights_offset, o.index_type, o.dtype, o.mode, o.reserved) == \
        (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, NONE, 1, api.OCM_ACC_BF16, 0, 0)
    assert ops.array[1].mode == 1 and ops.array[1].weights_offset == 11
    assert api.bag_ops(np.array([[0, 0, 4, 1, 0, 16, 16, 1, 0, 0, -1]]), "fp32").array[0].weights_offset == NONE
    with pytest.raises(ValueError, match="sum"):
        api.bag_ops([[0] * 11], torch.float32, mode="max")


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("bags", [1, 2, 37])
def test_shapes_and_bag_lengths(client, bags, itype):
    # rows of one vector (one live lane on the kernel path), exactly one tile, one tile and a vector; every dtype;
    # per list a sum, a weighted sum, a mean and an op without ids
    if bags == 37:
        lens = bag_lengths(37)
        assert lens[0] == 0 and lens[-1] == 0 and set(lens) == set(LENGTHS)
    for dtype in DTYPES:
        for rb in (16, 1024, 1040):
            lay = shapes_layout(itype, dtype, rb, bags, seed=rb + bags + dtype)
            assert lay.ops[-1][4] == 0 and lay.ops[-1][3] == bags
            skipped, err = _run(client, lay, seed=rb)
            assert skipped == 0 and err is None, err


@pytest.mark.parametrize("itype", ITYPES)
def test_rows_across_stripe_units(client, itype):
    lay = shapes_layout(itype, F32, 4112, 2, seed=2, table_rows=23, gap=1008)
    assert lay.ops[0][6] == 5120 and lay.ops[0][6] % UNIT
    skipped, err = _run(client, lay)
    assert skipped == 0 and err is None, err


def _cases_discriminate(dtype):
    # the values the order / fma cases use give other bits under another order or a fused multiply-add
    vals = [np.array([v], dtype=np.float32) for v in order_values(dtype)]
    assert bag_sum(vals) != bag_sum(vals[::-1]) and bag_sum(vals)[0] == vals[1][0] and bag_sum(vals[::-1])[0] == 0
    x, w = fma_case(dtype)
    rows = [r for r in x]
    want = bag_sum(rows, w)
    assert want != bag_sum(rows[::-1], w[::-1]) and want != bag_sum_fma(rows, w)
    # also after narrowing to the table's type: 2^-8, 0 and 2^-8 + the bit the product drops
    three = [bytes(narrow(v, dtype)) for v in (want, bag_sum(rows[::-1], w[::-1]), bag_sum_fma(rows, w))]
    assert len(set(three)) == 3 and want[0] == np.float32(2.0 ** -8)
    assert np.array_equal(widen(narrow(x.reshape(-1), dtype), dtype), x.reshape(-1))  # exact in the table's type


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_order_rounding_mean_and_ties(client, dtype, itype):
    _cases_discriminate(dtype)
    lay = order_layout(itype, dtype)
    local, remote = lay.images(1)
    want, _ = model(local, remote, lay.ops, lay.modes, itype, dtype)
    o = lay.ops[0]  # the two bags of the order case differ: in order and reversed
    rb = o[2] * ESIZE[dtype]
    assert not np.array_equal(want[o[0]:o[0] + rb], want[o[0] + o[5]:o[0] + o[5] + rb])
    o = lay.ops[1]  # and so do the two of the fma case
    assert not np.array_equal(want[o[0]:o[0] + rb], want[o[0] + o[5]:o[0] + o[5] + rb])
    assert lay.modes[2] == MEAN and lay.ops[2][3] == 2
    if dtype != F32:  # the sums on ties went to even: 1 and 1 + 2 ulp
        o = lay.ops[3]
        got = widen(want[o[0]:o[0] + 16], dtype)
        ulp = 2.0 ** -7 if dtype == api.OCM_ACC_BF16 else 2.0 ** -10
        assert got[0] == 1.0 and got[4] == np.float32(1.0 + 2 * ulp)
    skipped, err = _run(client, lay)
    assert skipped == 0 and err is None, err


@pytest.mark.parametrize("itype", ITYPES)
def test_offsets_are_clamped(client, itype):
    for dtype in DTYPES:
        skipped, err = _run(client, clamp_layout(itype, dtype))
        assert skipped == 0 and err is None, err


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("itype", ITYPES)
def test_out_of_range_ids_are_skipped_and_counted(client, itype, async_):
    lay, k = window_layout(itype, api.OCM_ACC_BF16 if async_ else F32)
    a = _pair(client, lay.local_bytes, lay.remote_bytes)
    before, before_bag = api.indexed_counters(), api.bag_counters()
    skipped, err = run_layout(a, lay, async_=async_)
    assert skipped == k == 18
    assert isinstance(err, api.OcmError) and f"indexed ops skipped {k} row(s)" in str(err), err
    assert ("ocm_wait" in str(err)) == async_
    after, after_bag = api.indexed_counters(), api.bag_counters()
    assert after["n_indexed_skipped"] == before["n_indexed_skipped"] + k and after["n_indexed"] == before["n_indexed"]
    assert after_bag["n_bag"] == before_bag["n_bag"] + 1  # the lookup was made
    a.wait()  # reported once
    good = Layout(itype, lay.dtype)
    good.bag(good.table(grid_values(np.random.RandomState(1), 8, 8)), [7, 0, 7], [0, 1, 3])
    skipped, err = run_layout(a, good)  # the next call succeeds
    assert skipped == 0 and err is None, err
    a.free()


@pytest.mark.parametrize("async_", [False, True])
def test_mixed_list_and_counters(client, async_):
    itype, dtype = (api.OCM_INDEX_I32, api.OCM_ACC_FP16) if async_ else (api.OCM_INDEX_I64, F32)
    lay = mixed_layout(itype, dtype, 20)
    assert [i for i, o in enumerate(lay.ops) if o[3] == 0] == [0, 10, 11, 19]
    a = _pair(client, lay.local_bytes, lay.remote_bytes)
    before, before_idx = api.bag_counters(), api.indexed_counters()
    skipped, err = run_layout(a, lay, seed=5, async_=async_)
    assert skipped == 0 and err is None, err
    after = api.bag_counters()
    bags, ids, nbytes = nominal(lay.ops, dtype)
    assert after["n_bag"] == before["n_bag"] + 1 and after["n_bag_ops"] == before["n_bag_ops"] + 20
    assert after["n_bag_bags"] == before["n_bag_bags"] + bags and after["n_bag_ids"] == before["n_bag_ids"] + ids
    assert after["bytes_bag"] == before["bytes_bag"] + nbytes
    assert api.indexed_counters() == before_idx
    a.free()


def test_validation(client):
    LB, RB = 16384, 4 * UNIT
    a = _pair(client, LB, RB)
    #       lo ro re bags ids ls  rs  rrows ioff  ooff  woff
    good = [0, 0, 4, 4, 8, 16, 16, 10, 4096, 8192, NONE]

    def fails(row, what, dtype=torch.float32, itype=api.OCM_INDEX_I32, mode="sum"):
        with pytest.raises(api.OcmError) as ei:
            a.bag_batch(api.bag_ops([good, row], dtype, itype, ["sum", mode]))  # the bad op is op 1
        assert "bag op 1" in str(ei.value) and what in str(ei.value), str(ei.value)

    for field, value, what in (("index_type", 3, "index_type"), ("dtype", 4, "element type"), ("mode", 2, "mode 2"), ("reserved", 1, "reserved")):
        two = api.bag_ops([good, good], torch.float32, api.OCM_INDEX_I32)
        setattr(two.array[1], field, value)
        with pytest.raises(api.OcmError, match="bag op 1.*" + what):
            a.bag_batch(two)
    fails([0, 0, 4, 4, 8, 16, 16, 10, 4096, 8192, 12288], "weights", mode="mean")
    fails([0, 0, 6, 4, 8, 32, 32, 10, 4096, 8192, NONE], "multiple of 16")
    fails([8, 0, 4, 4, 8, 16, 16, 10, 4096, 8192, NONE], "local offset")
    fails([0, 0, 4, 4, 8, 16, 24, 10, 4096, 8192, NONE], "multiple of 16")
    fails([0, 0, 8, 4, 8, 16, 32, 10, 4096, 8192, NONE], "local stride")
    fails([0, RB - 10 * 16 + 16, 4, 4, 8, 16, 16, 10, 4096, 8192, NONE], "remote table")
    fails([LB - 48, 0, 4, 4, 8, 16, 16, 10, 4096, 8192, NONE], "local table")
    fails([0, 0, 4, 4, 8, 16, 16, 10, 4098, 8192, NONE], "not a multiple")
    fails([0, 0, 4, 4, 8, 16, 16, 10, LB - 28, 8192, NONE], "ids index array")
    fails([0, 0, 4, 4, 8, 16, 16, 10, 4096, LB - 16, NONE], "offsets index array")   # bags + 1 entries
    fails([0, 0, 4, 4, 8, 16, 16, 10, 4096, 8192, 32], "overlaps")
    fails([4096 + 16, 0, 4, 4, 8, 16, 16, 10, 4096, 8192, NONE], "overlaps")
    fails([0, 0, 4, 4, 8, 16, 1 << 62, 5, 4096, 8192, NONE], "remote table")           # 4 * 2^62 wraps to 0
    lib = client.lib
    one = api.bag_ops([good], torch.float32, api.OCM_INDEX_I32)
    assert lib.ocm_copy_onesided_bag(a.handle, one.array, -1, 0) == -1 and "n_ops" in api.last_error()
    assert lib.ocm_copy_onesided_bag(a.handle, None, 1, 0) == -1 and api.last_error()
    assert lib.ocm_copy_onesided_bag(None, one.array, 1, 0) == -1 and api.last_error()
    for other in (api.batch_ops(np.array([[1, 0, 0, 32]])), api.indexed_ops([[0, 0, 0, 16, 4, 16, 16, NONE, 4096, 4, 8]])):
        with pytest.raises(TypeError):
            a.bag_batch(other)
    with pytest.raises(TypeError):
        a.indexed_batch(one)
    # exact fits pass; an op without bags says anything and is counted as an op only
    a.local_tensor(torch.uint8).zero_()
    a.bag_batch([[LB - 64, RB - 160, 4, 4, 8, 16, 16, 10, 4096, 8192, NONE]], torch.float32, api.OCM_INDEX_I32)
    # an op without ids names no id array at all, also over a table with fewer rows than it has bags: zeros
    a.local_tensor(torch.uint8)[:64].fill_(0xff)
    a.bag_batch([[0, 0, 4, 4, 0, 16, 16, 2, NONE, 8192, NONE]], torch.float32, api.OCM_INDEX_I32)
    assert not a.local_tensor(torch.uint8)[:64].any()
    before = api.bag_counters()
    a.bag_batch([[3, 1 << 40, 5, 0, 1 << 40, 1, 1, 1 << 40, 3, 3, 3]], torch.float32, 9, 9)
    after = api.bag_counters()
    assert after["n_bag"] == before["n_bag"] + 1 and after["n_bag_ops"] == before["n_bag_ops"] + 1
    assert after["n_bag_bags"] == before["n_bag_bags"] and after["bytes_bag"] == before["bytes_bag"]
    a.free()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_remote_embedding_bags(client, dtype):
    g = torch.Generator().manual_seed(7)
    emb = RemoteEmbedding(client, 500, 24, dtype, max_ids=300, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT, max_bags=40)
    plain = RemoteEmbedding(client, 500, 24, dtype, max_ids=300, kind=api.OCM_REMOTE_RDMA, stripe_unit=UNIT)
    assert plain.alloc.local_bytes == plain._ids_off + 8 * 300 and emb._ids_off == plain._ids_off  # max_bags=0: as it always was
    with pytest.raises(ValueError, match="max_bags"):
        plain.lookup_bags(torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    plain.close()
    table = (torch.randint(-127, 128, (500, 24), generator=g).float() / 16).to(dtype)
    emb.load(table)
    lens = torch.tensor([0, 1, 2, 4, 5, 9, 37, 0, 3, 7])
    offsets = torch.cumsum(lens, 0) - lens
    ids = torch.randint(0, 500, (int(lens.sum()),), generator=g)
    w = torch.randint(-64, 65, ids.shape, generator=g).float() / 48

    def want(weights, mean):
        out = []
        for b in range(len(lens)):
            lo, n = int(offsets[b]), int(lens[b])
            rows = [table[int(i)].float().numpy() for i in ids[lo:lo + n]]
            acc = bag_sum(rows, weights[lo:lo + n].numpy() if weights is not None else None) if rows else np.zeros(24, np.float32)
            out.append(acc / np.float32(n) if mean and n else acc)
        return torch.from_numpy(np.stack(out)).to(dtype)

    for itype in (torch.int64, torch.int32):
        for weights, mode in ((None, "sum"), (w, "sum"), (None, "mean")):
            got = emb.lookup_bags(ids.to(itype), offsets.to(itype), weights, mode=mode, async_=weights is None)
            emb.wait()
            assert got.shape == (10, 24) and torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                                         want(weights, mode == "mean").view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    # the same as lookup(ids) followed by an in-order fp32 sum on the host
    rows = emb.lookup(ids, async_=False).float().numpy()
    host = np.stack([bag_sum([rows[j] for j in range(int(offsets[b]), int(offsets[b]) + int(lens[b]))]) if lens[b] else np.zeros(24, np.float32)
                     for b in range(len(lens))])
    got = emb.lookup_bags(ids, offsets, async_=False)
    assert torch.equal(got.float(), torch.from_numpy(host).to(dtype).float())
    # torch's own pooled lookup agrees to rounding
    ref = torch.nn.functional.embedding_bag(ids, table.float(), offsets, mode="sum")
    assert torch.allclose(got.float(), ref, rtol=2 ** -7 if dtype == torch.bfloat16 else 1e-6, atol=1e-5)
    assert emb.lookup_bags(ids[:0], offsets[:0]).shape == (0, 24)
    assert not emb.lookup_bags(ids[:0], torch.zeros(3, dtype=torch.int64), async_=False).any()  # three empty bags: zeros
    # ids outside the table add nothing, are counted, and the bags are written all the same
    bad = torch.tensor([3, 500, 5, -1, 499])
    with pytest.raises(IndexError, match=r"skipped 2 row\(s\)"):
        emb.lookup_bags(bad, torch.tensor([0, 2]), async_=False)
    assert torch.equal(emb.bag_out[:2].float(), torch.stack([table[3].float(), table[5].float() + table[499].float()]).to(dtype).float())
    emb.lookup_bags(bad, torch.tensor([0, 2]), async_=True)  # async: known at wait()
    with pytest.raises(IndexError, match=r"skipped 2 row\(s\)"):
        emb.wait()
    emb.wait()
    with pytest.raises(ValueError):
        emb.lookup_bags(ids, torch.zeros(41, dtype=torch.int64))
    with pytest.raises(ValueError, match="sum"):
        emb.lookup_bags(ids, offsets, w, mode="mean")
    with pytest.raises(TypeError):
        emb.lookup_bags(ids, offsets.to(torch.int16))
    emb.close()
    comp = RemoteEmbedding(client, 64, 32, torch.bfloat16, max_ids=16, kind=api.OCM_REMOTE_RDMA, compress="mxfp8", max_bags=4)
    with pytest.raises(TypeError, match="compressed"):
        comp.lookup_bags(torch.zeros(3, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    comp.close()
