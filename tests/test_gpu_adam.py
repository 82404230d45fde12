"""The fused Adam kernel (csrc/src/kernels/optim.hip, adam_multi_kernel) through
Allocation.adam (one tensor: the count = 1 case) and Allocation.adam_multi, every variant
against the fp64 oracle of tests/adam_cases.py:

  <fp32 | bf16, generic>  HBM and striped state
  <fp32 | bf16, host>     host-tier state in one extent

with lengths from one tail element to a second grid-stride pass, state offsets that are
16-byte but not 256-byte aligned, stripe-unit boundaries inside the arrays, both orders of the
arrays, guard words around everything the kernels must leave alone, special values, and the
bf16 rounding bit for bit.

Every case prints the ratio of the kernel's error to torch-fp32's before it asserts
("adam-ratio", "adam-worst"; read with -s); the measured ones stand next to the bound,
adam_cases.KERNEL_OVER_TORCH.

The > 2^32 stripe-unit branch of state_ptr() needs 64 GiB of state and is not run here."""
import math

import pytest
import torch

from adam_cases import (FLOOR, KERNEL_OVER_TORCH, Step, adam_oracle, assert_bf16_rounding, bf16_table, check, errors,
                        hyper, kernel_hp, make_inputs, reference, torch_adam)
from oncilla_amd import api
from quant_cases import read_remote, write_remote

pytestmark = pytest.mark.gpu

UNIT = 4096           # stripe unit of the striped state
EXTENTS = 3           # the layout is made for three owners whatever the state is
GUARD_ELEMS = 64      # at least this many guard words before, between and after the arrays
GUARD32 = 0xFFA5C3E1 - (1 << 32)  # a NaN with a payload: arithmetic on it shows, and no kernel writes it
GUARD16 = 0xFFA5 - (1 << 16)
DEV = "cuda:0"
SMALL = [1, 3, 4, 5, 1023, 1027]  # tail only; one vector; vector + tail; a partly filled workgroup
TINY = [1, 3, 4, 5, 63, 64, 65]
RATIOS = []


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    reference.cache_clear()


def _client(mesh_factory, state):
    if state == "striped":
        m = mesh_factory(4, gpus=[0] * 4, policy="stripe")
    else:
        m = mesh_factory(2, gpus=[0, 0])
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _alloc(c, state, nbytes):
    kw = {"hbm": {}, "host": {"flags": api.OCM_ALLOC_HOST_TIER},
          "striped": {"flags": api.OCM_ALLOC_STRIPE, "stripe_unit": UNIT}}[state]
    a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=nbytes, remote_bytes=nbytes, **kw)
    ext = a.remote_info()["extents"]
    if state == "striped":
        assert len(ext) == EXTENTS
    else:
        assert len(ext) == 1 and (ext[0]["tier"] == api.OCM_TIER_HOST) == (state == "host")
    return a


def second_pass_length(host_kernel):
    """A length that reaches the grid-stride loop's second pass and ends on a 3-element tail:
    in that pass some of a lane's four vectors are live and some are past the end. The host
    variants (adam_multi_kernel<.., true>) run 128 workgroups, the generic ones two per CU."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_pass = 128 * 4096 if host_kernel else 2 * cus * 4096
    return per_pass + 4 * (256 + 17) + 3


def _place(lo, n):
    """The first byte offset >= lo that is 16-byte and not 256-byte aligned and, where the
    array is long enough, puts a stripe-unit boundary inside it and its tail (n % 4 elements)
    in another extent than element 0."""
    for off in range((lo + 15) // 16 * 16, lo + 2 * UNIT + 16, 16):
        if off % 256 == 0:
            continue
        first, last, tail = off // UNIT, (off + 4 * (n - 1)) // UNIT, (off + 4 * (n & ~3)) // UNIT
        if n >= 5 and first == last:
            continue
        if n >= 5 and n % 4 and tail % EXTENTS == first % EXTENTS:
            continue
        return off
    raise AssertionError(f"no place for {n} elements after {lo}")


class Layout:
    """Where the fp32 state arrays of tensors of `sizes` lie in the remote half: per tensor the
    arrays of `order` ('m', 'v' and for bf16 'w'), guard words around each."""

    def __init__(self, sizes, order):
        self.sizes, self.order, self.off, cur = sizes, order, [], 0
        for n in sizes:
            d = {}
            for name in order:
                d[name] = _place(cur + 4 * GUARD_ELEMS, n)
                cur = d[name] + 4 * n
            self.off.append(d)
        self.nbytes = (cur + 4 * GUARD_ELEMS + EXTENTS * UNIT - 1) // (EXTENTS * UNIT) * (EXTENTS * UNIT)
        for n, d in zip(sizes, self.off):
            assert all(o % 16 == 0 and o % 256 for o in d.values())
            if order[0] == "v":
                assert d["m"] > d["v"] and ("w" not in d or d["v"] < d["w"] < d["m"])

    def image(self):
        """The remote half before the first step, as int32 words: guards everywhere."""
        return torch.full((self.nbytes // 4,), GUARD32, dtype=torch.int32)

    def words(self, i, name):
        o = self.off[i][name] // 4
        return slice(o, o + self.sizes[i])


def _pack(tensors, dtype):
    """1-D CPU tensors -> one buffer of `dtype` with 64 guard elements around each, and their
    starts. fp32 slices are 16-byte aligned; bf16 slices 8-byte and not 16-byte aligned."""
    starts, pos = [], GUARD_ELEMS
    for t in tensors:
        if dtype == torch.bfloat16:
            pos += (4 - pos) % 8
        else:
            pos += -pos % 4
        starts.append(pos)
        pos += t.numel() + GUARD_ELEMS
    if dtype == torch.bfloat16:
        buf = torch.full((pos,), GUARD16, dtype=torch.int16).view(dtype)
    else:
        buf = torch.full((pos,), GUARD32, dtype=torch.int32).view(dtype)
    for t, s in zip(tensors, starts):
        buf[s:s + t.numel()] = t.to(dtype)
    return buf, starts


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _views(buf, starts, sizes, bf16):
    out = [buf[s:s + n] for s, n in zip(starts, sizes)]
    for v in out:
        assert v.data_ptr() % 16 == (8 if bf16 else 0)
    return out


def run_steps(a, lay, p0, g_steps, hps, bf16, multi, skip=(), m0=None, v0=None, p_start=None):
    """Write the state, run one fused update per entry of `hps` (kernel hp tuples) and read
    everything back. p0 / g_steps[t]: per-tensor fp32 CPU tensors (bf16-valued for bf16).
    Checks what must not change: every guard word of the remote half and of the p buffer, all
    of the gradients, and p / m / v of the tensors in `skip` (left out of the calls). Returns
    per tensor (p, m, v, master): p in its own dtype, master None for fp32. bf16: p0 is the
    master; the parameters start as its rounding, or as p_start."""
    sizes, k = lay.sizes, len(lay.sizes)
    dtype = torch.bfloat16 if bf16 else torch.float32
    img = lay.image()
    touched = torch.zeros(img.numel(), dtype=torch.bool)
    for i in range(k):
        img[lay.words(i, "m")] = (m0[i] if m0 else torch.zeros(sizes[i])).view(torch.int32)
        img[lay.words(i, "v")] = (v0[i] if v0 else torch.zeros(sizes[i])).view(torch.int32)
        if bf16:
            img[lay.words(i, "w")] = p0[i].view(torch.int32)
        if i not in skip:
            for name in lay.order:
                touched[lay.words(i, name)] = True
    write_remote(a, 0, 0, img)
    pbuf, pst = _pack(p_start or p0, dtype)
    pdev = pbuf.to(DEV)
    pv = _views(pdev, pst, sizes, bf16)
    gbufs, gdevs, gvs = [], [], []
    for gs in g_steps:
        gb, gst = _pack(gs, dtype)
        gbufs.append(gb)
        gdevs.append(gb.to(DEV))
        gvs.append(_views(gdevs[-1], gst, sizes, bf16))
    live = [i for i in range(k) if i not in skip]
    for t, hp in enumerate(hps):
        if multi:
            a.adam_multi([pv[i] for i in live], [gvs[t][i] for i in live], [lay.off[i]["m"] for i in live],
                         [lay.off[i]["v"] for i in live], hp, w_offs=[lay.off[i]["w"] for i in live] if bf16 else None)
        else:
            for i in live:
                a.adam(pv[i], gvs[t][i], lay.off[i]["m"], lay.off[i]["v"], hp, w_off=lay.off[i]["w"] if bf16 else None)
    torch.cuda.synchronize()
    got = read_remote(a, 0, 0, lay.nbytes).view(torch.int32)
    pgot = pdev.cpu()
    # what the kernels must not touch
    same = got == img
    assert bool(same[~touched].all()), f"remote word {int((~same & ~touched).nonzero()[0])} outside the live arrays changed"
    ptouched = torch.zeros(pbuf.numel(), dtype=torch.bool)
    for i in live:
        ptouched[pst[i]:pst[i] + sizes[i]] = True
    psame = _bits(pgot) == _bits(pbuf)
    assert bool(psame[~ptouched].all()), f"p buffer element {int((~psame & ~ptouched).nonzero()[0])} outside the live tensors changed"
    for gb, gd in zip(gbufs, gdevs):
        assert torch.equal(_bits(gd.cpu()), _bits(gb)), "a gradient buffer changed"
    out = []
    for i in range(k):
        f = lambda name: got[lay.words(i, name)].view(torch.float32)  # noqa: E731
        out.append((pgot[pst[i]:pst[i] + sizes[i]], f("m"), f("v"), f("w") if bf16 else None))
    return out


def run_case(a, what, sizes, hp_name, bf16, multi, order, skip=()):
    """STEPS steps from zero moments on tensors of `sizes` (tensor i's inputs: reference(n,
    n + 13 i)), then p / master, m and v of every live tensor within the bound of the oracle;
    bf16 p must be the rounding of the master that the kernel itself wrote."""
    hp, adamw = hyper(hp_name)
    refs = [reference(n, n + 13 * i, hp_name, bf16) for i, n in enumerate(sizes)]
    lay = Layout(sizes, order)
    steps = len(refs[0].g_list)
    rnd = [torch.randn(n, generator=torch.Generator().manual_seed(i)) for i, n in enumerate(sizes)]
    res = run_steps(a, lay, [r.p for r in refs], [[r.g_list[t] for r in refs] for t in range(steps)],
                    [kernel_hp(hp, adamw, t + 1) for t in range(steps)], bf16, multi, skip,
                    m0=[x if i in skip else torch.zeros_like(x) for i, x in enumerate(rnd)],
                    v0=[x.abs() if i in skip else torch.zeros_like(x) for i, x in enumerate(rnd)])
    for i, (p, m, v, w) in enumerate(res):
        if i in skip:
            continue
        label = f"{what} n={sizes[i]}"
        if bf16:
            assert_bf16_rounding(p, w, label)
        check((w if bf16 else p, m, v), refs[i], hp_name, label, RATIOS)


def _multi_sizes(first):
    """37 tensors, `first` among tiny ones; four have no gradient, so 33 go into the call:
    two launches (32 descriptors each)."""
    sizes = [first] + [TINY[i % len(TINY)] for i in range(36)]
    skip = (2, 3, 20, 36)
    assert len(sizes) - len(skip) == 33 and {sizes[i] for i in skip} == {3, 4, 64, 1} and first not in TINY
    return sizes, skip


def _record(path):
    """Print the largest ratio per quantity of the cases run so far on `path` (read with -s)."""
    worst = {}
    for what, q, r in RATIOS:
        if what.startswith(path):
            worst[q] = max(worst.get(q, 0.0), r)
    print(f"adam-worst {path}: " + " ".join(f"{q}={r:.2f}" for q, r in sorted(worst.items())))


@pytest.mark.parametrize("state", ["hbm", "host", "striped"])
def test_every_path_against_the_oracle(mesh_factory, state):
    big = second_pass_length(state == "host")  # fp32 and bf16 alike: both have a host variant
    msizes, mskip = _multi_sizes(big)
    with _client(mesh_factory, state) as c:
        a = _alloc(c, state, max(Layout(s, "mvw").nbytes for s in (msizes, [big] + SMALL)))
        try:
            for bf16 in (False, True):
                kind = "bf16" if bf16 else "fp32"
                # the long tensor: L2 Adam for fp32, AdamW for bf16; the short ones the other way
                # round as well, with exp_avg behind exp_avg_sq (bf16: the master between them)
                long_set, short_set = ("adamw", "fast_l2") if bf16 else ("default_l2", "adamw")
                fwd, rev = ("mvw", "vwm") if bf16 else ("mv", "vm")
                run_case(a, f"single-{kind}/{state}", [big] + SMALL, long_set, bf16, False, fwd)
                run_case(a, f"single-{kind}/{state}", SMALL, short_set, bf16, False, rev)
                # multi: the long tensor gets (nearly) the whole grid, gx = min(want, tuned grid *
                # biggest / total), and is longer than one pass of it
                cus = torch.cuda.get_device_properties(0).multi_processor_count
                grid = 128 if state == "host" else 2 * cus
                first = [n for i, n in enumerate(msizes) if i not in mskip][:32]  # the first launch
                gx = int(grid * big / sum(first) + 0.999)
                assert max(first) == big and big > gx * 4096
                run_case(a, f"multi-{kind}/{state}", msizes, long_set, bf16, True, fwd, mskip)
                run_case(a, f"multi-{kind}/{state}", [1027] + msizes[1:], short_set, bf16, True, rev, mskip)
                _record(f"single-{kind}/{state}")
                _record(f"multi-{kind}/{state}")
        finally:
            a.free()


def test_one_minus_beta_is_rounded_once(mesh_factory):
    """b2 = 0.9999: 1.f - float(b2) is 1.7e-4 off 1 - b2, and exp_avg_sq with it, 500 times
    torch's own error; the kernel gets fp32(1 - b2) from the host instead. The remaining
    hyper-parameter sets (no decay; lr * wd == 1) run here as well."""
    with _client(mesh_factory, "hbm") as c:
        a = _alloc(c, "hbm", 1 << 20)
        try:
            run_case(a, "single-fp32/hbm", [1027], "slow_b2", False, False, "mv")
            for hp_name in ("slow_b2", "default", "adamw_full_decay"):
                run_case(a, "single-fp32/hbm", [1027, 5], hp_name, False, False, "mv")
                run_case(a, "multi-fp32/hbm", [1027, 5], hp_name, False, True, "vm")
                run_case(a, "multi-bf16/hbm", [1027, 5], hp_name, True, True, "mvw")
            _record("single-fp32/hbm")
        finally:
            a.free()


# ---- special values ----

INF, NAN = math.inf, math.nan
# 1e19: g * g is 1e38, short of overflow, so every quantity stays finite; 1e30 (not in the
# fp64 oracle's reach: fp32 exp_avg_sq is inf, the update 0) is compared with torch alone.
SPECIAL = [0.0, INF, -INF, NAN, 1e-40, 1e19, -0.0, 1e30]
SPECIAL_AT = [1, 5, 9, 13, 17, 21, 25, 29]  # in the vector part, ordinary elements between them
SPECIAL_TAILS = [(0.0, INF, NAN), (-INF, 1e-40, 1e19), (-0.0, 1e30, 0.0)]  # elements 64 .. 66 of three tensors
N_SPECIAL = 67


def _special_inputs(k):
    p, gs = make_inputs(N_SPECIAL, 300 + k)
    for g in gs:
        g[SPECIAL_AT] = torch.tensor(SPECIAL, dtype=torch.float32)
        g[64:] = torch.tensor(SPECIAL_TAILS[k], dtype=torch.float32)
    return p, gs


def _check_special(got, p, gs, hp_name, what):
    hp, adamw = hyper(hp_name)
    want = adam_oracle(p, gs, hp, adamw)[-1]
    t32 = torch_adam(p, gs, hp, adamw)[-1]
    for q, g, t in zip("pmv", got, t32):
        assert torch.equal(torch.isnan(g), torch.isnan(t)), f"{what}: NaN positions of {q}"
        inf = torch.isinf(t)
        assert torch.equal(torch.isinf(g), inf) and torch.equal(g[inf], t[inf]), f"{what}: inf positions of {q}"
    finite = torch.isfinite(t32[0]) & torch.isfinite(t32[1]) & torch.isfinite(t32[2])
    ordinary = torch.ones(N_SPECIAL, dtype=torch.bool)
    ordinary[SPECIAL_AT] = False
    ordinary[64:] = False
    # the neighbours of the special elements: finite in the kernel's result (and in torch's, so
    # the bound below covers them)
    assert bool(finite[ordinary].all()) and all(bool(torch.isfinite(g[ordinary]).all()) for g in got), what
    want = Step(*[torch.where(finite, x, torch.zeros_like(x)) for x in want])
    terr = errors(t32, want, hp.lr, finite)
    err = errors(got, want, hp.lr, finite)
    for q in "pmv":
        print(f"adam-ratio {what} special {hp_name} {q}: error {err[q]:.3e} torch {terr[q]:.3e}")
        assert err[q] <= KERNEL_OVER_TORCH * max(terr[q], FLOOR), (what, q, err[q], terr[q])
    # exp_avg_sq overflowed in fp32 (g = 1e30): exp_avg and the parameter are finite and take
    # no step; the same operations as torch's, so the same values to rounding
    over = torch.isinf(t32[2]) & torch.isfinite(t32[0])
    assert int(over.sum()) >= 1
    for g, t in zip(got[:2], t32[:2]):
        assert bool(((g[over] - t[over]).abs() <= KERNEL_OVER_TORCH * FLOOR * t[over].abs()).all()), what


def test_special_values(mesh_factory):
    """g = 0 on zero moments (the denominator is eps), +-inf, NaN, a denormal, 1e19, -0.0 and
    1e30 at fixed places of the vector part and of the tail, fp32 single and multi, HBM and host
    state: NaN and inf where torch's fp32 Adam has them, everything else within the bound."""
    ins = [_special_inputs(k) for k in range(3)]
    sizes = [N_SPECIAL] * 3
    with _client(mesh_factory, "hbm") as c:
        for state in ("hbm", "host"):
            a = _alloc(c, state, 1 << 16)
            try:
                for hp_name in ("default", "adamw"):  # no L2 term: g = 0 stays 0
                    hp, adamw = hyper(hp_name)
                    for multi in (False, True):
                        lay = Layout(sizes, "mv")
                        res = run_steps(a, lay, [p for p, _ in ins], [[gs[t] for _, gs in ins] for t in range(4)],
                                        [kernel_hp(hp, adamw, t + 1) for t in range(4)], False, multi)
                        for k, (p, m, v, _) in enumerate(res):
                            _check_special((p, m, v), *ins[k], hp_name, f"{'multi' if multi else 'single'}/{state} tensor {k}")
            finally:
                a.free()


# ---- bf16 rounding, bit for bit ----

def test_bf16_parameter_is_the_nearest_even_rounding_of_the_master(mesh_factory):
    """step_size = 0, g = 0, no decay: the rule leaves the master as it is, and the bf16
    parameter must be its round-to-nearest-even (ties, overflow to inf, denormals, +-0, NaN):
    71 elements: 0 .. 67 go through the vector code, 68 .. 70 through the scalar tail. The table
    as it is keeps every crafted entry in the vector part; two copies swap crafted entries into
    the tail."""
    bits = bf16_table()
    masters = [bits.view(torch.float32)]
    # a tie that rounds up, the overflow to inf, a NaN whose payload is in the dropped half;
    # a tie that rounds down, -0, a denormal tie that rounds up
    for tail in ((0x3F818000, 0x7F7FFFFF, 0x7F800001), (0xBF808000, 0x80000000, 0x00018000)):
        t, words = bits.clone(), [int(x) & 0xFFFFFFFF for x in bits]
        for dst, w in zip((68, 69, 70), tail):
            src = words.index(w)
            assert src < 68  # a crafted entry of the vector part
            t[dst], t[src] = bits[src], bits[dst]
        assert [int(x) & 0xFFFFFFFF for x in t[68:]] == list(tail)
        masters.append(t.view(torch.float32))
    k = len(masters)
    hp = (0.9, 0.999, 1e-8, 0.0, 0.0, 1.0)
    zeros = [torch.zeros(71)] * k
    with _client(mesh_factory, "hbm") as c:
        for state in ("hbm", "host"):
            a = _alloc(c, state, 1 << 16)
            try:
                for multi in (False, True):
                    lay = Layout([71] * k, "mvw")
                    # the parameters start as 1.0: what is read back is what the kernel wrote
                    res = run_steps(a, lay, masters, [zeros], [hp], True, multi, p_start=[torch.ones(71)] * k)
                    for i, (p, m, v, w) in enumerate(res):
                        what = f"{'multi' if multi else 'single'}/{state} table {i}"
                        assert_bf16_rounding(p, masters[i], what)
                        nan = torch.isnan(masters[i])
                        assert torch.isnan(w[nan]).all()
                        assert torch.equal(w[~nan].view(torch.int32), masters[i][~nan].view(torch.int32)), what
                        assert not m.view(torch.int32).any() and not v.view(torch.int32).any(), what
            finally:
                a.free()
