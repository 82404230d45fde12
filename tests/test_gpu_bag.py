"""Pooled lookups on the gfx950 kernel path (csrc/src/kernels/xfer_bag.hip): every output byte, and every
other byte of both halves, against the numpy model (bag_cases.model), with the pool in the pinned host
tier (one daemon) and striped over three owners (four daemons, a 4 KiB stripe unit), and int32 and int64
ids."""
import numpy as np
import pytest
import torch

from bag_cases import (BF16, DTYPES, ESIZE, F32, FP16, IN_FLIGHT, LENGTHS, MEAN, TORCH_DTYPE, TORCH_INDEX, UNIT, Layout, bag_lengths,
                       bag_sum, bag_sum_fma, clamp_layout, fma_case, grid_values, mixed_layout, model, narrow, nominal, order_layout,
                       order_values, run_layout, shapes_layout, widen, window_layout)
from oncilla_amd import api
from oncilla_amd.models import RemoteEmbedding, RemoteEmbeddingAdam

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM
ITYPES = [api.OCM_INDEX_I32, api.OCM_INDEX_I64]
DEV = "cuda:0"


def _client(mesh_factory, n_daemons):
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _pair(c, local_bytes, remote_bytes, n_daemons):
    assert local_bytes <= 1 << 20 and remote_bytes <= 1 << 20
    a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE,
                stripe_unit=UNIT)
    assert len(a.remote_info()["extents"]) == (1 if n_daemons == 1 else 3)
    return a


def _run(c, lay, n_daemons, seed=1, async_=False):
    a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
    skipped, err = run_layout(a, lay, seed=seed, async_=async_)
    a.free()
    return skipped, err


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("bags", [1, 2, 37])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_shapes_and_bag_lengths(mesh_factory, n_daemons, bags, itype):
    # rows of one vector (one live lane), exactly one tile, one tile and a vector; every dtype; per list a sum, a
    # weighted sum, a mean and an op without ids. 37 bags: every length of LENGTHS, the first and the last bag empty;
    # duplicates inside bags, one id through a whole bag
    if bags == 37:
        lens = bag_lengths(37)
        assert lens[0] == 0 and lens[-1] == 0 and set(lens) == set(LENGTHS)
        assert {0, 1, 2, IN_FLIGHT, IN_FLIGHT + 1, 2 * IN_FLIGHT + 1, 37} == set(LENGTHS)
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            for rb in (16, 1024, 1040):
                lay = shapes_layout(itype, dtype, rb, bags, seed=rb + bags + dtype)
                assert lay.ops[-1][4] == 0 and lay.ops[-1][3] == bags  # ids == 0
                skipped, err = _run(c, lay, n_daemons, seed=rb)
                assert skipped == 0 and err is None, err


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_rows_across_stripe_units(mesh_factory, n_daemons, itype):
    # rows of 4112 bytes (five tiles, the last of one vector) 5120 bytes apart: no multiple of the 4 KiB unit, so
    # picked rows start mid-unit on every owner and most straddle two
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            lay = shapes_layout(itype, dtype, 4112, 37, seed=dtype, table_rows=23, gap=1008)
            starts = []
            for o in lay.ops[:3]:
                assert o[6] == 5120 and o[6] % UNIT
                ids = np.frombuffer(lay.images(1)[0][o[8]:o[8] + o[4] * 4 * itype].tobytes(), dtype=np.int32 if itype == 1 else np.int64)
                starts += [o[1] + int(r) * o[6] for r in ids]
            assert all(s % UNIT for s in starts)                                        # every picked row starts mid-unit
            assert len({s // UNIT % 3 for s in starts}) == 3                            # on every owner
            assert sum(s // UNIT != (s + 4111) // UNIT for s in starts) >= 15           # and rows straddle two
            skipped, err = _run(c, lay, n_daemons)
            assert skipped == 0 and err is None, err


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_order_rounding_mean_and_ties(mesh_factory, n_daemons, itype):
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            # on the CPU first: these values give other bits under another order or a fused multiply-add
            vals = [np.array([v], dtype=np.float32) for v in order_values(dtype)]
            assert bag_sum(vals)[0] == vals[1][0] and bag_sum(vals[::-1])[0] == 0
            x, w = fma_case(dtype)
            rows = [r for r in x]
            three = [bag_sum(rows, w), bag_sum(rows[::-1], w[::-1]), bag_sum_fma(rows, w)]
            assert three[0] != three[1] and three[0] != three[2]
            assert len({bytes(narrow(v, dtype)) for v in three}) == 3  # also after narrowing to the table's type
            lay = order_layout(itype, dtype)
            local, remote = lay.images(1)
            want, _ = model(local, remote, lay.ops, lay.modes, itype, dtype)
            for o in lay.ops[:2]:  # the second bag of each is the first reversed: other bits
                assert not np.array_equal(want[o[0]:o[0] + 16], want[o[0] + o[5]:o[0] + o[5] + 16])
            assert lay.modes[2] == MEAN and [b - a for a, b in ((0, 3), (3, 10))] == [3, 7]
            if dtype != F32:  # sums on ties of the narrow type go to even: 1 and 1 + 2 ulp
                o = lay.ops[3]
                got = widen(want[o[0]:o[0] + 16], dtype)
                ulp = 2.0 ** -7 if dtype == BF16 else 2.0 ** -10
                assert got[0] == 1.0 and got[4] == np.float32(1.0 + 2 * ulp)
            skipped, err = _run(c, lay, n_daemons)
            assert skipped == 0 and err is None, err


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_offsets_are_clamped(mesh_factory, n_daemons, itype):
    # an offsets entry above ids, a decreasing pair, a negative entry
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            skipped, err = _run(c, clamp_layout(itype, dtype), n_daemons)
            assert skipped == 0 and err is None, err


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_out_of_range_ids_are_skipped_and_counted(mesh_factory, n_daemons, itype, async_):
    # the window construction of test_gpu_indexed.py: whatever a broken check lets through stays inside the pair and
    # fails the byte comparison. Rows of three tiles: an entry is counted once all the same.
    dtype = (F32, BF16, FP16)[(itype + async_) % 3]
    lay, k = window_layout(itype, dtype)
    assert k == 18 and lay.ops[0][2] * ESIZE[dtype] == 2064
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
        before, before_bag = api.indexed_counters(), api.bag_counters()
        skipped, err = run_layout(a, lay, async_=async_)
        assert skipped == k
        assert isinstance(err, api.OcmError) and f"indexed ops skipped {k} row(s)" in str(err), err
        assert ("ocm_wait" in str(err)) == async_
        after, after_bag = api.indexed_counters(), api.bag_counters()
        assert after["n_indexed_skipped"] == before["n_indexed_skipped"] + k
        assert after_bag["n_bag"] == before_bag["n_bag"] + 1  # the lookup was made
        a.wait()  # reported once
        good = Layout(itype, dtype)
        good.bag(good.table(grid_values(np.random.RandomState(1), 8, 8)), [7, 0, 7], [0, 1, 3])
        skipped, err = run_layout(a, good)  # the next call succeeds
        assert skipped == 0 and err is None, err
        a.free()


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_list_of_twenty_mixed_ops(mesh_factory, n_daemons, async_):
    # over the 16 ops the kernel arguments hold: the uploaded path; ops without bags first, in the middle and last
    itype = ITYPES[async_]
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            lay = mixed_layout(itype, dtype, 20, seed=dtype)
            assert [i for i, o in enumerate(lay.ops) if o[3] == 0] == [0, 10, 11, 19]
            a = _pair(c, lay.local_bytes, lay.remote_bytes, n_daemons)
            before, before_idx, before_all = api.bag_counters(), api.indexed_counters(), api.counters()
            skipped, err = run_layout(a, lay, seed=5, async_=async_)
            assert skipped == 0 and err is None, err
            after = api.bag_counters()
            bags, ids, nbytes = nominal(lay.ops, dtype)
            assert after["n_bag"] == before["n_bag"] + 1 and after["n_bag_ops"] == before["n_bag_ops"] + 20
            assert after["n_bag_bags"] == before["n_bag_bags"] + bags and after["n_bag_ids"] == before["n_bag_ids"] + ids
            assert after["bytes_bag"] == before["bytes_bag"] + nbytes
            # its own launch: no indexed list and no batch (the helpers' plain puts and gets are no batches)
            assert api.indexed_counters() == before_idx and api.counters()["n_batch"] == before_all["n_batch"]
            a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_lookup_bags_ordered_after_the_kernel_that_made_the_ids(mesh_factory, n_daemons, dtype):
    tdt, idt = TORCH_DTYPE[dtype], TORCH_INDEX[1 + dtype % 2]
    g = torch.Generator().manual_seed(5)
    rows, dim, bags = 1500, 136, 64  # rows of 544 or 272 bytes
    lens = torch.tensor([LENGTHS[(i + 1) % len(LENGTHS)] for i in range(bags)])
    lens[0] = lens[-1] = 0
    offsets = (torch.cumsum(lens, 0) - lens)
    k = int(lens.sum())
    with _client(mesh_factory, n_daemons) as c:
        emb = RemoteEmbedding(c, rows, dim, tdt, max_ids=700, stripe_unit=UNIT, max_bags=bags)
        assert emb.alloc.local_bytes <= 1 << 20 and emb.alloc.remote_size() <= 1 << 20 and emb.bag_out.is_cuda and k <= 700
        table = (torch.randint(-127, 128, (rows, dim), generator=g).float() / 16).to(tdt)
        emb.load(table.cuda())
        weights = torch.randint(-64, 65, (k,), generator=g).float() / 48
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for w, mode in ((None, "sum"), (weights, "sum"), (None, "mean")):
                ids = torch.randint(0, rows, (k,), device="cuda", dtype=idt)  # made by a kernel on `side`
                offs = offsets.to(device="cuda", dtype=idt)
                got = emb.lookup_bags(ids, offs, None if w is None else w.cuda(), mode=mode)  # no host sync in between
                kept = got.clone()                                                             # read by torch on `side`
                side.synchronize()
                # bit for bit the model: the in-order fp32 sum of the table's rows, narrowed once
                hid = ids.cpu()
                want = []
                for b in range(bags):
                    lo, n = int(offsets[b]), int(lens[b])
                    terms = [table[int(i)].float().numpy() for i in hid[lo:lo + n]]
                    acc = bag_sum(terms, w[lo:lo + n].numpy() if w is not None else None) if terms else np.zeros(dim, np.float32)
                    want.append(acc / np.float32(n) if mode == "mean" and n else acc)
                want = np.stack(want)
                assert np.array_equal(kept.cpu().view(torch.uint8).numpy().reshape(-1), narrow(want.reshape(-1), dtype))
                if w is None and mode == "sum":
                    # and what lookup(ids) followed by an in-order fp32 sum on the host gives
                    looked = emb.lookup(ids).clone()
                    side.synchronize()
                    looked = looked.cpu().float().numpy()
                    host = np.stack([bag_sum([looked[j] for j in range(int(offsets[b]), int(offsets[b]) + int(lens[b]))])
                                     if lens[b] else np.zeros(dim, np.float32) for b in range(bags)])
                    assert np.array_equal(host, want)
            with pytest.raises(IndexError, match=r"skipped 1 row\(s\)"):
                emb.lookup_bags(torch.tensor([1, rows, 3], device="cuda", dtype=idt), torch.tensor([0, 1], device="cuda", dtype=idt),
                                async_=False)
            assert torch.equal(emb.bag_out[:2].cpu(), torch.stack([table[1], table[3]]))  # the bad id added nothing
        emb.wait()
        emb.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_step_bags_is_step_on_the_expanded_rows(mesh_factory, n_daemons, dtype):
    gen = torch.Generator().manual_seed(3)
    rows, dim = 64, 24
    w0 = torch.randn(rows, dim, generator=gen).to(dtype)
    lens = torch.tensor([0, 3, 1, 5, 0, 2])
    offsets = torch.cumsum(lens, 0) - lens
    ids = torch.randint(0, rows, (int(lens.sum()),), generator=gen)
    gb = torch.randn(len(lens), dim, generator=gen)
    psw = torch.randint(-8, 9, ids.shape, generator=gen).float() / 4
    with _client(mesh_factory, n_daemons) as c:
        for weights in (None, psw):
            got = []
            for bagged in (True, False):
                emb = RemoteEmbedding(c, rows, dim, dtype=dtype, max_ids=64, stripe_unit=UNIT, max_bags=8)
                emb.load(w0.to(DEV))
                opt = RemoteEmbeddingAdam(emb, lr=1e-2)
                for _ in range(2):
                    if bagged:
                        opt.step_bags(ids.to(DEV), offsets.to(DEV), gb.to(DEV), None if weights is None else weights.to(DEV), scale=0.5)
                    else:  # the rows by hand: bag b's gradient for each of its ids, times the id's weight
                        grad = torch.cat([gb[b:b + 1].expand(int(n), dim) for b, n in enumerate(lens)])
                        if weights is not None:
                            grad = grad * weights.unsqueeze(1)
                        opt.step(ids.to(DEV), grad.to(DEV), scale=0.5)
                every = torch.arange(rows, device=DEV)
                after = emb.lookup(every).clone()
                m, v = opt.moments(every)
                master = opt.master(every) if dtype == torch.bfloat16 else m
                torch.cuda.synchronize()
                assert opt.skipped() == 0 and opt.t == 2 and bool((after.cpu() != w0).any())
                got.append((after.cpu(), m.cpu(), v.cpu(), master.cpu()))
                opt.close()
                emb.close()
            for x, y in zip(*got):
                assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
