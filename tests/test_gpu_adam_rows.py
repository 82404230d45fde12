"""The row-sparse fused Adam kernel (csrc/src/kernels/optim_rows.hip) through Allocation.adam_rows and
RemoteEmbeddingAdam, against the fp64 oracle of tests/adam_rows_cases.py: fp32 and bf16 tables, int32
and int64 ids, HBM, host-tier and striped placement, row strides larger than the rows with guard
words in the padding and around every table, out-of-range ids, the gradient scale, special values,
and the refusals of the real library.

Every case prints the ratio of the kernel's error to the fp32 yardstick's before it asserts
("adam-rows-ratio", "adam-rows-worst"; read with -s)."""
import math

import pytest
import torch

from adam_acc_cases import scaled
from adam_cases import (FLOOR, KERNEL_OVER_TORCH, QUANTITIES, STEPS, Step, assert_bf16_rounding, bound, check, errors, hyper,
                        reference)
from adam_rows_cases import (DIMS, HP_NAME, TABLE_ROWS, build_case, case, check_rows, kernel_hp_rows, make_table,
                             rows_oracle, rows_torch)
from oncilla_amd import api
from oncilla_amd.models import RemoteEmbedding, RemoteEmbeddingAdam
from quant_cases import read_remote, write_remote
from test_gpu_adam import EXTENTS, GUARD16, GUARD32, UNIT, _alloc, _client

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD_BYTES = 272
RATIOS = []
HP = hyper(HP_NAME)[0]
IN_FLIGHT, WAVES, WG_PER_CU = 4, 4, 4  # kAdamRowsInFlight, kListWaves, kAdamRowsWgPerCu of ocm/adam_rows.h


def _up(x, m):
    return (x + m - 1) // m * m


class Tab:
    """One table of `rows` rows of row_bytes at `stride` from byte `off` of a remote half."""

    def __init__(self, off, stride, row_bytes, rows, dtype):
        self.off, self.stride, self.row_bytes, self.rows, self.dtype = off, stride, row_bytes, rows, dtype
        self.end = off + (rows - 1) * stride + row_bytes

    @property
    def at(self):
        return (self.off, self.stride)

    def view(self, img):
        return img.as_strided((self.rows, self.row_bytes), (self.stride, 1), self.off)

    def write(self, img, values):
        self.view(img).copy_(values.to(self.dtype).contiguous().view(torch.uint8).view(self.rows, self.row_bytes))

    def read(self, img):
        return self.view(img).contiguous().clone().view(self.dtype)

    def mark(self, mask, ids):
        self.view(mask)[torch.as_tensor(ids, dtype=torch.int64)] = 1


class Layout:
    """The tables of one case in their remote halves: `names` in the state's half, the embedding table in
    the same one (shared) or in a half of its own. Offsets are 16-byte and not 256-byte aligned (a bf16
    table: 8-byte and not 16-byte), strides larger than the row likewise unless `dense`."""

    def __init__(self, rows, dim, bf16, shared, dense=False):
        self.rows, self.dim, self.bf16, self.shared = rows, dim, bf16, shared
        self.names = ("m", "v", "w") if bf16 else ("m", "v")
        pos = {"table": GUARD_BYTES, "state": GUARD_BYTES}
        self.tabs = {}
        order = (("v", "state"), ("table", "state" if shared else "table"), ("m", "state"), ("w", "state"))
        for name, half in order:
            if name == "w" and not bf16:
                continue
            small = name == "table" and bf16
            dtype = torch.bfloat16 if small else torch.float32
            rb, al = dim * (2 if small else 4), 8 if small else 16
            stride = rb if dense else rb + al
            if not dense and stride % (16 * al) == 0:
                stride += al
            off = _up(pos[half], 16) + (8 if small else 0)
            if off % 256 == 0:
                off += 16
            self.tabs[name] = Tab(off, stride, rb, rows, dtype)
            pos[half] = self.tabs[name].end + GUARD_BYTES
        gran = EXTENTS * UNIT
        self.state_bytes = _up(pos["state"], gran)
        self.table_bytes = self.state_bytes if shared else _up(pos["table"], gran)
        for name, t in self.tabs.items():
            al = 8 if t.dtype == torch.bfloat16 else 16
            assert t.off % al == 0 and t.stride % al == 0 and (dense or (t.off % (16 * al) and t.stride > t.row_bytes))

    def image(self, nbytes, bf16_guard):
        if bf16_guard:
            return torch.full((nbytes // 2,), GUARD16, dtype=torch.int16).view(torch.uint8)
        return torch.full((nbytes // 4,), GUARD32, dtype=torch.int32).view(torch.uint8)


class Runner:
    """Tables written into the pair(s), steps run one by one; after each, every byte outside the rows the
    step picked is compared with what it was, and the id and gradient buffers with what they were."""

    def __init__(self, table_alloc, state_alloc, lay, p0, m0=None, v0=None):
        self.ta, self.sa, self.lay = table_alloc, state_alloc, lay
        shared = table_alloc is state_alloc
        assert shared == lay.shared
        self.simg = lay.image(lay.state_bytes, False)
        self.timg = self.simg if shared else lay.image(lay.table_bytes, lay.bf16)
        zeros = torch.zeros(lay.rows, lay.dim)
        lay.tabs["m"].write(self.simg, zeros if m0 is None else m0)
        lay.tabs["v"].write(self.simg, zeros if v0 is None else v0)
        if lay.bf16:
            lay.tabs["w"].write(self.simg, p0)
        lay.tabs["table"].write(self.timg, p0)
        write_remote(state_alloc, 0, 0, self.simg)
        if not shared:
            write_remote(table_alloc, 0, 0, self.timg)
        self.counter = torch.zeros(1, dtype=torch.int64, device=DEV)

    def step(self, t, ids, g_rows, index_dtype=torch.int64, gscale=None, count=True, valid=None, pad=4):
        """Global step t on `ids` with gradient rows g_rows (fp32 CPU values); `valid`: the ids that are
        inside the table (default all). The gradient sits in a buffer with `pad` elements between rows."""
        lay = self.lay
        gdtype = torch.bfloat16 if lay.bf16 else torch.float32
        k = len(ids)
        gbuf = torch.full((k, lay.dim + pad), -7.0).to(gdtype)
        gbuf[:, :lay.dim] = g_rows.to(gdtype)
        gdev, idev = gbuf.to(DEV), torch.tensor(list(ids), dtype=index_dtype, device=DEV)
        kw = {} if gscale is None else {"gscale": gscale}
        self.ta.adam_rows(self.sa, idev, gdev[:, :lay.dim], lay.tabs["table"].at, lay.tabs["m"].at, lay.tabs["v"].at,
                          kernel_hp_rows(HP, t), lay.rows, master=lay.tabs["w"].at if lay.bf16 else None,
                          skipped=self.counter if count else None, **kw)
        torch.cuda.synchronize()
        assert torch.equal(gdev.cpu().view(torch.int16 if lay.bf16 else torch.int32),
                           gbuf.view(torch.int16 if lay.bf16 else torch.int32)), "the gradient buffer changed"
        assert idev.cpu().tolist() == list(ids), "the id buffer changed"
        self.verify_untouched(ids if valid is None else valid)

    def verify_untouched(self, ids):
        lay, shared = self.lay, self.ta is self.sa
        sgot = read_remote(self.sa, 0, 0, lay.state_bytes)
        tgot = sgot if shared else read_remote(self.ta, 0, 0, lay.table_bytes)
        smask = torch.zeros(lay.state_bytes, dtype=torch.uint8)
        tmask = smask if shared else torch.zeros(lay.table_bytes, dtype=torch.uint8)
        for name in lay.names:
            lay.tabs[name].mark(smask, ids)
        lay.tabs["table"].mark(tmask, ids)
        for what, got, was, mask in (("state", sgot, self.simg, smask), ("table", tgot, self.timg, tmask)):
            bad = (got != was) & (mask == 0)
            assert not bool(bad.any()), f"{what} half: byte {int(bad.nonzero()[0])} outside the picked rows changed"
        self.simg, self.timg = sgot, tgot

    def tables(self):
        """(p, m, v, table): p is the master for bf16, the table itself for fp32."""
        lay = self.lay
        table = lay.tabs["table"].read(self.timg)
        p = lay.tabs["w"].read(self.simg) if lay.bf16 else table
        return p, lay.tabs["m"].read(self.simg), lay.tabs["v"].read(self.simg), table


def _record(path):
    worst = {}
    for what, q, r in RATIOS:
        if what.startswith(path):
            worst[q] = max(worst.get(q, 0.0), r)
    print(f"adam-rows-worst {path}: " + " ".join(f"{q}={r:.2f}" for q, r in sorted(worst.items())))


def _max_bytes(shared):
    return max(max(Layout(TABLE_ROWS, d, b, shared).state_bytes, Layout(TABLE_ROWS, d, b, shared).table_bytes)
               for d in DIMS for b in (False, True))


@pytest.mark.parametrize("state", ["hbm", "host", "striped"])
def test_every_path_against_the_oracle(mesh_factory, state):
    with _client(mesh_factory, state) as c:
        nbytes = max(_max_bytes(False), _max_bytes(True))
        ta, sa = _alloc(c, state, nbytes), _alloc(c, state, nbytes)
        try:
            for bf16 in (False, True):
                for n, dim in enumerate(DIMS):
                    cs = case(dim, bf16)
                    for index_dtype in (torch.int32, torch.int64):
                        # the table in a pair of its own, and (every other case) in the state's
                        shared = (n + (index_dtype == torch.int64)) % 2 == 1
                        lay = Layout(TABLE_ROWS, dim, bf16, shared)
                        if dim == 1028:  # rows of 4112 bytes: longer than a stripe unit
                            assert all(t.row_bytes > UNIT for nm, t in lay.tabs.items() if t.dtype == torch.float32)
                        run = Runner(sa if shared else ta, sa, lay, cs.p)
                        for t, (ids, g) in enumerate(cs.steps, 1):
                            run.step(t, ids, g, index_dtype)
                        p, m, v, table = run.tables()
                        what = f"{'bf16' if bf16 else 'fp32'}/{state} dim={dim} {str(index_dtype)[6:]}{' shared' if shared else ''}"
                        if bf16:
                            assert_bf16_rounding(table, p, what)
                        check_rows((p, m, v), cs, what, RATIOS)
                        assert int(run.counter.item()) == 0
                _record(f"{'bf16' if bf16 else 'fp32'}/{state}")
        finally:
            ta.free()
            sa.free()


def test_dense_cross_check(mesh_factory):
    """Every row picked at every step, rows contiguous, zero initial moments: the dense fused Adam's case,
    inside adam_cases.check() of adam_cases.reference() for rows * dim elements."""
    dim = 260
    n = TABLE_ROWS * dim
    ref = reference(n, n, "default")
    lay = Layout(TABLE_ROWS, dim, False, True, dense=True)
    with _client(mesh_factory, "hbm") as c:
        a = _alloc(c, "hbm", lay.state_bytes)
        try:
            run = Runner(a, a, lay, ref.p.view(TABLE_ROWS, dim))
            gen = torch.Generator().manual_seed(5)
            for t in range(STEPS):
                perm = torch.randperm(TABLE_ROWS, generator=gen)
                run.step(t + 1, perm.tolist(), ref.g_list[t].view(TABLE_ROWS, dim)[perm], pad=0)
            p, m, v, _ = run.tables()
            check((p.reshape(-1), m.reshape(-1), v.reshape(-1)), ref, "default", "rows-as-dense")
        finally:
            a.free()
    reference.cache_clear()


def second_round_rows(cus):
    """A k (dim 8: one tile a row) at which the capped grid's waves own one tile more than they keep in
    flight and the last wave with tiles owns fewer: adam_rows_launch_shape and list_wave_range of
    csrc/include/ocm, restated."""
    cap = WG_PER_CU * cus
    for k in range(cap * WAVES * IN_FLIGHT + 1, cap * WAVES * IN_FLIGHT + 16):
        grid = min((k + WAVES * IN_FLIGHT - 1) // (WAVES * IN_FLIGHT), cap)
        per = (k + grid * WAVES - 1) // (grid * WAVES)
        if grid == cap and per == IN_FLIGHT + 1 and 0 < k % per < IN_FLIGHT:
            return k
    raise AssertionError("no such k")


def test_second_round(mesh_factory):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    k = second_round_rows(cus)
    grid = WG_PER_CU * cus
    per = (k + grid * WAVES - 1) // (grid * WAVES)
    assert per > IN_FLIGHT and 0 < k - (k // per) * per < IN_FLIGHT and k // per < grid * WAVES
    dim = 8
    p, gs = make_table(k, dim, 77, steps=1)
    ids = torch.randperm(k, generator=torch.Generator().manual_seed(3)).tolist()
    cs = build_case(p, gs, [ids])
    lay = Layout(k, dim, False, False)
    with _client(mesh_factory, "hbm") as c:
        ta, sa = _alloc(c, "hbm", lay.table_bytes), _alloc(c, "hbm", lay.state_bytes)
        try:
            run = Runner(ta, sa, lay, p)
            run.step(1, ids, cs.steps[0][1], torch.int32)
            pg, m, v, _ = run.tables()
            check_rows((pg, m, v), cs, f"second round k={k}", RATIOS)
        finally:
            ta.free()
            sa.free()


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_out_of_range_ids_are_skipped_and_counted(mesh_factory, index_dtype):
    dim = 260  # two tiles a row: a skipped row is counted once
    bad = [-1, TABLE_ROWS, 2 ** 31 - 1] + ([2 ** 40] if index_dtype == torch.int64 else [])
    valid = [4, 36, 0, 19, 7]
    ids = [valid[0], bad[0], valid[1], bad[1], valid[2], valid[3], bad[2]] + bad[3:] + [valid[4]]
    p, gs = make_table(TABLE_ROWS, dim, 91, steps=2)
    g_rows = torch.randn(len(ids), dim, generator=torch.Generator().manual_seed(1))
    keep = [i for i, x in enumerate(ids) if x in valid]
    steps = [(tuple(valid), g_rows[keep]), (tuple(valid), g_rows[keep])]
    want, t32 = rows_oracle(p, steps, HP), rows_torch(p, steps, HP)
    lay = Layout(TABLE_ROWS, dim, False, False)
    with _client(mesh_factory, "striped") as c:
        ta, sa = _alloc(c, "striped", lay.table_bytes), _alloc(c, "striped", lay.state_bytes)
        try:
            run = Runner(ta, sa, lay, p)
            run.step(1, ids, g_rows, index_dtype, valid=valid)
            assert int(run.counter.item()) == len(bad)
            run.step(2, ids, g_rows, index_dtype, valid=valid, count=False)  # a null skipped pointer: runs clean
            assert int(run.counter.item()) == len(bad)
            pg, m, v, _ = run.tables()
            mask = torch.zeros(TABLE_ROWS, dim, dtype=torch.bool)
            mask[valid] = True
            err, terr = errors((pg, m, v), want[-1], HP.lr, mask), errors(t32[-1], want[-1], HP.lr, mask)
            for q in QUANTITIES:
                print(f"adam-rows-ratio out-of-range {q}: error {err[q]:.3e} torch {terr[q]:.3e}")
                assert err[q] <= bound(terr)[q], (q, err[q], terr[q])
            # every valid row moved
            assert bool((m[valid] != 0).any(dim=1).all())
        finally:
            ta.free()
            sa.free()


def test_gscale(mesh_factory):
    dim = 260
    cs = case(dim)
    third = [(ids, scaled(g, 1.0 / 3.0)) for ids, g in cs.steps]
    want, t32 = rows_oracle(cs.p, third, HP)[-1], rows_torch(cs.p, third, HP)[-1]
    lay = Layout(TABLE_ROWS, dim, False, False)
    with _client(mesh_factory, "hbm") as c:
        ta, sa = _alloc(c, "hbm", lay.table_bytes), _alloc(c, "hbm", lay.state_bytes)
        try:
            res = {}
            for name, gscale in (("none", None), ("one", 1.0), ("third", 1.0 / 3.0)):
                run = Runner(ta, sa, lay, cs.p)
                for t, (ids, g) in enumerate(cs.steps, 1):
                    run.step(t, ids, g, gscale=gscale)
                res[name] = run.tables()[:3]
            for a, b in zip(res["none"], res["one"]):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "gscale = 1 changes bits"
            err, terr = errors(res["third"], want, HP.lr, cs.picked), errors(t32, want, HP.lr, cs.picked)
            for q in QUANTITIES:
                print(f"adam-rows-ratio gscale=1/3 {q}: error {err[q]:.3e} torch {terr[q]:.3e}")
                assert err[q] <= bound(terr)[q], (q, err[q], terr[q])
            with pytest.raises(api.OcmError, match="gscale"):
                run.step(5, [1], torch.ones(1, dim), gscale=math.inf, valid=[])
        finally:
            ta.free()
            sa.free()


def test_special_gradient_values(mesh_factory):
    """0, +-inf, NaN, a denormal and 1e30 in one row: NaN and inf where the fp32 yardstick has them, the
    neighbours finite and within the bound (test_gpu_adam.test_special_values' check, on one row)."""
    dim = 64
    special = {1: 0.0, 5: math.inf, 9: -math.inf, 13: math.nan, 17: 1e-40, 21: 1e30}
    p, gs = make_table(TABLE_ROWS, dim, 55, steps=2)
    ids = [9, 30]
    steps = []
    for g in gs:
        rows = g[ids].clone()
        for at, val in special.items():
            rows[0, at] = val
        steps.append((tuple(ids), rows))
    want, t32 = rows_oracle(p, steps, HP)[-1], rows_torch(p, steps, HP)[-1]
    lay = Layout(TABLE_ROWS, dim, False, False)
    with _client(mesh_factory, "hbm") as c:
        ta, sa = _alloc(c, "hbm", lay.table_bytes), _alloc(c, "hbm", lay.state_bytes)
        try:
            run = Runner(ta, sa, lay, p)
            for t, (i, g) in enumerate(steps, 1):
                run.step(t, i, g)
            got = run.tables()[:3]
        finally:
            ta.free()
            sa.free()
    for q, g, t in zip("pmv", got, t32):
        assert torch.equal(torch.isnan(g), torch.isnan(t)), f"NaN positions of {q}"
        inf = torch.isinf(t)
        assert torch.equal(torch.isinf(g), inf) and torch.equal(g[inf], t[inf]), f"inf positions of {q}"
    finite = torch.isfinite(t32[0]) & torch.isfinite(t32[1]) & torch.isfinite(t32[2])
    ordinary = torch.zeros(TABLE_ROWS, dim, dtype=torch.bool)
    ordinary[ids] = True
    ordinary[9, list(special)] = False
    assert bool(finite[ordinary].all()) and all(bool(torch.isfinite(g[ordinary]).all()) for g in got)
    wantf = Step(*[torch.where(finite, x, torch.zeros_like(x)) for x in want])
    in_rows = torch.zeros(TABLE_ROWS, dim, dtype=torch.bool)
    in_rows[ids] = True
    mask = finite & in_rows
    terr, err = errors(t32, wantf, HP.lr, mask), errors(got, wantf, HP.lr, mask)
    for q in "pmv":
        print(f"adam-rows-ratio special {q}: error {err[q]:.3e} torch {terr[q]:.3e}")
        assert err[q] <= KERNEL_OVER_TORCH * max(terr[q], FLOOR), (q, err[q], terr[q])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_end_to_end(mesh_factory, dtype):
    """RemoteEmbeddingAdam.step with duplicate ids equals the step with the hand-coalesced gradient, bit
    for bit; lookup() right after step(), with no sync between, returns the updated rows."""
    rows, dim = 300, 64
    gen = torch.Generator().manual_seed(8)
    w0 = torch.randn(rows, dim, generator=gen).to(dtype)
    ids = torch.tensor([5, 17, 5, 299, 0, 17, 5], dtype=torch.int64)
    g = torch.randn(len(ids), dim, generator=gen).to(dtype)
    uniq, inv = torch.unique(ids, return_inverse=True)
    hand = torch.zeros(len(uniq), dim).index_add_(0, inv, g.float()).to(dtype)
    with _client(mesh_factory, "striped") as c:
        got = []
        for dup in (True, False):
            emb = RemoteEmbedding(c, rows, dim, dtype=dtype, max_ids=64, stripe_unit=UNIT)
            emb.load(w0.to(DEV))
            opt = RemoteEmbeddingAdam(emb, lr=1e-2)
            if dtype == torch.bfloat16:
                assert torch.equal(opt.master(uniq.to(DEV)).cpu(), w0[uniq].float())
            assert not opt.moments(uniq.to(DEV))[0].any()
            before = emb.lookup(uniq.to(DEV)).clone()
            for _ in range(2):
                if dup:
                    opt.step(ids.to(DEV), g.to(DEV))
                else:
                    opt.step(uniq.to(DEV).int(), hand.to(DEV))
            after = emb.lookup(uniq.to(DEV)).clone()  # no sync since step(): lookup's stream_wait orders it
            m, v = opt.moments(uniq.to(DEV))
            torch.cuda.synchronize()
            assert opt.skipped() == 0 and opt.t == 2
            assert bool((after != before).any(dim=1).all())
            rest = torch.tensor([i for i in range(64) if i not in uniq.tolist()], device=DEV)
            assert torch.equal(emb.lookup(rest).cpu(), w0[rest.cpu()])
            got.append((after.cpu(), m.cpu(), v.cpu()))
            opt.step(torch.tensor([rows, 3], device=DEV), g[:2].to(DEV))
            assert opt.skipped() == 1
            opt.close()
            emb.close()
        for a, b in zip(*got):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        # the update is the oracle's, on the coalesced gradient
        steps = [(tuple(uniq.tolist()), hand.float())] * 2
        hp = type(HP)(1e-2, 0.9, 0.999, 1e-8, 0.0)
        want, t32 = rows_oracle(w0.float(), steps, hp)[-1], rows_torch(w0.float(), steps, hp)[-1]
        mask = torch.zeros(rows, dim, dtype=torch.bool)
        mask[uniq] = True
        terr = errors(t32, want, hp.lr, mask)
        full = [torch.zeros(rows, dim) for _ in range(2)]
        for x, part in zip(full, got[0][1:]):
            x[uniq] = part
        e = errors((want.p.float(), full[0], full[1]), want, hp.lr, mask)  # p: fp32 rows are checked below
        assert e["m"] <= bound(terr)["m"] and e["v"] <= bound(terr)["v"], (e, terr)
        if dtype == torch.float32:
            pf = w0.clone()
            pf[uniq] = got[0][0]
            e = errors((pf, full[0], full[1]), want, hp.lr, mask)
            assert e["p"] <= bound(terr)["p"], (e, terr)


def test_refusals_write_nothing(mesh_factory):
    dim = 8
    p, gs = make_table(TABLE_ROWS, dim, 3, steps=1)
    lay = Layout(TABLE_ROWS, dim, False, True)
    tab, m, v = lay.tabs["table"], lay.tabs["m"], lay.tabs["v"]
    with _client(mesh_factory, "hbm") as c:
        a = _alloc(c, "hbm", lay.state_bytes)
        try:
            run = Runner(a, a, lay, p)
            ids = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
            g8, g6 = torch.ones(2, 8, device=DEV), torch.ones(2, 6, device=DEV)
            hp = kernel_hp_rows(HP, 1)
            cases = [
                ("dim 6", dict(grad=g6), "multiple of 4"),
                ("a misaligned offset", dict(exp_avg=(m.off + 8, m.stride)), "not a multiple of 16"),
                ("L2 weight decay", dict(hp=hp[:3] + (0.01,) + hp[4:]), "weight decay"),
                ("decoupled weight decay", dict(hp=hp + (0.999,)), "weight decay"),
                ("exp_avg on exp_avg_sq", dict(exp_avg=v.at), "overlaps"),
                ("exp_avg inside the table", dict(exp_avg=(tab.off + 16, m.stride)), "overlaps"),
                ("a table past the half", dict(table=(lay.state_bytes - tab.stride, tab.stride)), "exceeds"),
            ]
            for what, change, msg in cases:
                kw = dict(grad=g8, table=tab.at, exp_avg=m.at, exp_avg_sq=v.at, hp=hp)
                kw.update(change)
                with pytest.raises(api.OcmError, match=msg):
                    a.adam_rows(a, ids, kw["grad"], kw["table"], kw["exp_avg"], kw["exp_avg_sq"], kw["hp"], TABLE_ROWS,
                                skipped=run.counter)
                torch.cuda.synchronize()
                run.verify_untouched([])
            assert int(run.counter.item()) == 0
            # the accepted neighbour of them all
            a.adam_rows(a, ids, g8, tab.at, m.at, v.at, hp, TABLE_ROWS, skipped=run.counter)
            torch.cuda.synchronize()
            run.verify_untouched([1, 2])
            assert bool((run.tables()[1][[1, 2]] != 0).all())
        finally:
            a.free()
