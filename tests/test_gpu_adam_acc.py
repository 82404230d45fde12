"""The fused Adam kernel with its gradient read from remote fp32 accumulators
(adam_multi_kernel<.., kAcc = true>, ocm_x_adam_multi_acc) through Allocation.adam_multi_acc and
OffloadedAdam.step(accumulator=...): every variant against the fp64 oracle of tests/adam_cases.py
for every placement of the two spaces, what the pass zeroes and what it must leave alone,
bit-for-bit agreement with the local-gradient path, the scale rounded on its own, special
values, refusals before any launch, and the training workload.

The layout is test_gpu_adam.py's: offsets 16-byte but not 256-byte aligned, guard words (a NaN
with a payload) around every array of both remote halves, stripe-unit boundaries inside the
arrays. Every oracle case prints the kernel's error over torch-fp32's before it asserts
("adam-ratio"; read with -s); the bound is adam_cases.KERNEL_OVER_TORCH, unchanged."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from adam_acc_cases import TABLE_B1, scaled, unfused_table
from adam_cases import (Hyper, Reference, adam_oracle, assert_bf16_rounding, bound, check, errors, hyper, kernel_hp,
                        make_inputs, torch_adam)
from oncilla_amd import api
from oncilla_amd.models import OffloadedAdam, OffloadedGradAccumulator
from quant_cases import read_remote, write_remote
from test_gpu_adam import (DEV, SMALL, Layout, _alloc, _bits, _check_special, _client, _multi_sizes, _pack,
                           _special_inputs, _views, second_pass_length)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 4
THIRD = 1.0 / 3.0


@functools.lru_cache(maxsize=None)
def acc_reference(n, seed, hp_name, bf16, gscale):
    """(Reference, accumulator values per step) for one tensor: p as adam_cases makes it (bf16-valued
    for bf16 parameters), accumulators fp32 and not bf16-representable; the oracle and torch's fp32
    Adam are fed fl32(gscale * acc). Computed once and shared; callers leave the tensors unchanged."""
    hp, adamw = hyper(hp_name)
    p = make_inputs(n, seed, bf16)[0]
    accs = make_inputs(n, seed)[1]
    if n >= 4:
        assert not torch.equal(accs[0], accs[0].to(torch.bfloat16).float())
    gs = [scaled(a, gscale) for a in accs]
    last = adam_oracle(p, gs, hp, adamw)[-1]
    t32 = torch_adam(p, gs, hp, adamw)[-1]
    return Reference(p, tuple(gs), last, t32, errors(t32, last, hp.lr)), tuple(accs)


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    acc_reference.cache_clear()


def run_acc(sa, ga, slay, glay, p0, accs, hps, bf16, gscale=1.0, zero=True, skip=(), m0=None, v0=None):
    """Write the state, then per entry of `hps`: write that step's accumulators (accs[t][i], all
    tensors), run one fused update of the tensors not in `skip` and read the accumulator half back.
    sa / ga: the state and the gradient allocation, laid out by slay / glay (array 'g'); the same
    allocation and the same Layout when the accumulators share the state's half.

    Checked after every step: with `zero` every accumulator word of every live tensor is 0x00000000,
    without it the image is bit for bit what was written; every guard word of the gradient half and
    the accumulators of the skipped tensors are intact. Checked at the end: every guard word of the
    state half, the state of the skipped tensors, the guards of the p buffer.
    Returns per tensor (p, m, v, master)."""
    same = ga is sa
    assert same == (glay is slay)
    sizes, k = slay.sizes, len(slay.sizes)
    dtype = torch.bfloat16 if bf16 else torch.float32
    simg = slay.image()
    state_live = torch.zeros(simg.numel(), dtype=torch.bool)
    for i in range(k):
        simg[slay.words(i, "m")] = (m0[i] if m0 else torch.zeros(sizes[i])).view(torch.int32)
        simg[slay.words(i, "v")] = (v0[i] if v0 else torch.zeros(sizes[i])).view(torch.int32)
        if bf16:
            simg[slay.words(i, "w")] = p0[i].view(torch.int32)
        if i not in skip:
            for name in ("mvw" if bf16 else "mv"):
                state_live[slay.words(i, name)] = True
    if not same:
        write_remote(sa, 0, 0, simg)
    gimg = simg.clone() if same else glay.image()
    others = ~state_live if same else torch.ones(gimg.numel(), dtype=torch.bool)  # all but the live state arrays
    pbuf, pst = _pack(p0, dtype)
    pdev = pbuf.to(DEV)
    pv = _views(pdev, pst, sizes, bf16)
    live = [i for i in range(k) if i not in skip]
    for t, hp in enumerate(hps):
        for i in range(k):
            gimg[glay.words(i, "g")] = accs[t][i].view(torch.int32)
        write_remote(ga, 0, 0, gimg)
        sa.adam_multi_acc([pv[i] for i in live], ga, [glay.off[i]["g"] for i in live], [slay.off[i]["m"] for i in live],
                          [slay.off[i]["v"] for i in live], hp, gscale=gscale, zero=zero,
                          w_offs=[slay.off[i]["w"] for i in live] if bf16 else None)
        torch.cuda.synchronize()
        got = read_remote(ga, 0, 0, glay.nbytes).view(torch.int32)
        want = gimg.clone()
        if zero:
            for i in live:
                want[glay.words(i, "g")] = 0
        diff = (got != want) & others
        assert not bool(diff.any()), (f"step {t + 1}: word {int(diff.nonzero()[0])} of the gradient half is "
                                      f"0x{int(got[diff][0]) & 0xffffffff:08x}, expected 0x{int(want[diff][0]) & 0xffffffff:08x}")
        if same:
            gimg = got.clone()  # the state as the step left it goes back with the next accumulators
    sgot = got if same else read_remote(sa, 0, 0, slay.nbytes).view(torch.int32)
    if not same:
        sdiff = (sgot != simg) & ~state_live
        assert not bool(sdiff.any()), f"state word {int(sdiff.nonzero()[0])} outside the live arrays changed"
    pgot = pdev.cpu()
    ptouched = torch.zeros(pbuf.numel(), dtype=torch.bool)
    for i in live:
        ptouched[pst[i]:pst[i] + sizes[i]] = True
    psame = _bits(pgot) == _bits(pbuf)
    assert bool(psame[~ptouched].all()), f"p buffer element {int((~psame & ~ptouched).nonzero()[0])} outside the live tensors changed"
    out = []
    for i in range(k):
        f = lambda name: sgot[slay.words(i, name)].view(torch.float32)  # noqa: E731
        out.append((pgot[pst[i]:pst[i] + sizes[i]], f("m"), f("v"), f("w") if bf16 else None))
    return out


def run_oracle_case(sa, ga, what, sizes, hp_name, bf16, gscale, zero, skip=()):
    """STEPS steps from zero moments on tensors of `sizes` with tensor i's inputs
    acc_reference(n, n + 13 i): p / master, m and v of every live tensor within the bound."""
    hp, adamw = hyper(hp_name)
    refs = [acc_reference(n, n + 13 * i, hp_name, bf16, gscale) for i, n in enumerate(sizes)]
    order = "mvw" if bf16 else "vm"
    same = ga is sa
    slay = Layout(sizes, order + "g" if same else order)
    glay = slay if same else Layout(sizes, "g")
    rnd = [torch.randn(n, generator=torch.Generator().manual_seed(i)) for i, n in enumerate(sizes)]
    res = run_acc(sa, ga, slay, glay, [r.p for r, _ in refs], [[a[t] for _, a in refs] for t in range(STEPS)],
                  [kernel_hp(hp, adamw, t + 1) for t in range(STEPS)], bf16, gscale, zero, skip,
                  m0=[x if i in skip else torch.zeros_like(x) for i, x in enumerate(rnd)],
                  v0=[x.abs() if i in skip else torch.zeros_like(x) for i, x in enumerate(rnd)])
    for i, (p, m, v, w) in enumerate(res):
        label = f"{what} n={sizes[i]}"
        if i in skip:  # left out of the call: p, m and v as they were
            assert torch.equal(_bits(p), _bits(refs[i][0].p.to(p.dtype))), label
            assert torch.equal(m, rnd[i]) and torch.equal(v, rnd[i].abs()), label
            continue
        if bf16:
            assert_bf16_rounding(p, w, label)
        check((w if bf16 else p, m, v), refs[i][0], hp_name, label)


def _nbytes(lists, order):
    return max(Layout(s, order).nbytes for s in lists)


LONG_AMONG_TINY = 70003  # 18 workgroups for it, of which the tiny tensors' all but one exit at once

# (state, accumulators): "same" puts the accumulators into the state's own remote half
PAIRS = [("host", "host"), ("hbm", "hbm"), ("striped", "striped"), ("hbm", "host"), ("host", "hbm"),
         ("hbm", "same"), ("host", "same"), ("striped", "same")]


@pytest.mark.parametrize("state,grads", PAIRS)
def test_every_variant_against_the_oracle(mesh_factory, state, grads):
    """host/host and host/same take the PCIe variant (two buffer resources), every other pair the
    generic one. Per pair, fp32 and bf16: the short lengths and one that reaches the second
    grid-stride pass and ends on a 3-element tail in one launch; then 33 of 37 tensors, one long,
    in two launches, the other four left out. zero=False on the bf16 list, zero=True elsewhere."""
    host_kernel = state == "host" and grads in ("host", "same")
    big = second_pass_length(host_kernel)
    one_launch = SMALL + [big]
    msizes, mskip = _multi_sizes(LONG_AMONG_TINY)
    with _client(mesh_factory, state) as c:
        same = grads == "same"
        sa = _alloc(c, state, _nbytes((one_launch, msizes), "mvwg" if same else "mvw"))
        ga = sa if same else _alloc(c, grads, _nbytes((one_launch, msizes), "g"))
        try:
            for bf16 in (False, True):
                kind = "bf16" if bf16 else "fp32"
                run_oracle_case(sa, ga, f"acc-{kind}/{state}/{grads}", one_launch, "adamw" if bf16 else "default_l2", bf16,
                                THIRD if bf16 else 0.25, True)
                run_oracle_case(sa, ga, f"acc-multi-{kind}/{state}/{grads}", msizes, "fast_l2" if bf16 else "adamw", bf16,
                                1.0 if bf16 else THIRD, not bf16, mskip)
        finally:
            if not same:
                ga.free()
            sa.free()


# ---- agreement with the local-gradient path ----

AGREE_SIZES = [1027, 5, 4099, 1, 64]


def _run_local(a, lay, p0, g_steps, hps, bf16):
    """The existing path on the same layout: adam_multi with the gradients as local tensors."""
    sizes, k = lay.sizes, len(lay.sizes)
    dtype = torch.bfloat16 if bf16 else torch.float32
    img = lay.image()
    for i in range(k):
        img[lay.words(i, "m")] = 0
        img[lay.words(i, "v")] = 0
        if bf16:
            img[lay.words(i, "w")] = p0[i].view(torch.int32)
    write_remote(a, 0, 0, img)
    pbuf, pst = _pack(p0, dtype)
    pdev = pbuf.to(DEV)
    pv = _views(pdev, pst, sizes, bf16)
    for gs, hp in zip(g_steps, hps):
        gb, gst = _pack(gs, dtype)
        gdev = gb.to(DEV)
        a.adam_multi(pv, _views(gdev, gst, sizes, bf16), [d["m"] for d in lay.off], [d["v"] for d in lay.off], hp,
                     w_offs=[d["w"] for d in lay.off] if bf16 else None)
        torch.cuda.synchronize()
    got = read_remote(a, 0, 0, lay.nbytes).view(torch.int32)
    pgot = pdev.cpu()
    return [(pgot[pst[i]:pst[i] + sizes[i]],) + tuple(got[lay.words(i, name)].view(torch.float32)
                                                       for name in ("mvw" if bf16 else "mv")) for i in range(k)]


@pytest.mark.parametrize("state", ["hbm", "host", "striped"])
def test_agrees_bit_for_bit_with_the_local_gradient_path(mesh_factory, state):
    """fp32 with gscale 1 and 0.25, bf16 with bf16-representable accumulators: p, the master and the
    moments after four steps are those of adam_multi on a twin allocation fed fl32(gscale * acc) as
    local tensors. Both instantiations inline the one adam1."""
    hp, adamw = hyper("default_l2")
    hps = [kernel_hp(hp, adamw, t + 1) for t in range(STEPS)]
    order = "mvw"
    with _client(mesh_factory, state) as c:
        nbytes = Layout(AGREE_SIZES, order).nbytes
        sa, twin = _alloc(c, state, nbytes), _alloc(c, state, nbytes)
        ga = _alloc(c, state, Layout(AGREE_SIZES, "g").nbytes)
        try:
            for bf16, gscale in ((False, 1.0), (False, 0.25), (True, 1.0), (True, 0.25)):
                ins = [make_inputs(n, 500 + n, bf16) for n in AGREE_SIZES]
                p0 = [p for p, _ in ins]
                accs = [[gs[t] for _, gs in ins] for t in range(STEPS)]
                g_steps = [[scaled(a, gscale) for a in step] for step in accs]
                if bf16:  # what the bf16 path can be handed exactly
                    assert all(torch.equal(g, g.to(torch.bfloat16).float()) for step in g_steps for g in step)
                slay, glay = Layout(AGREE_SIZES, order[:3 if bf16 else 2]), Layout(AGREE_SIZES, "g")
                got = run_acc(sa, ga, slay, glay, p0, accs, hps, bf16, gscale, True)
                want = _run_local(twin, slay, p0, g_steps, hps, bf16)
                for i, (g, w) in enumerate(zip(got, want)):
                    mine = (g[0], g[1], g[2]) + ((g[3],) if bf16 else ())
                    for name, x, y in zip("pmvw", mine, w):
                        ne = _bits(x) != _bits(y)
                        assert not bool(ne.any()), (f"{state} bf16={bf16} gscale={gscale} tensor {i} {name}: element "
                                                    f"{int(ne.nonzero()[0])}: {x[ne][0].item()!r} vs {y[ne][0].item()!r}")
        finally:
            for a in (ga, twin, sa):
                a.free()


# ---- the scale is rounded on its own ----

@pytest.mark.parametrize("state", ["hbm", "host"])
def test_scale_is_rounded_on_its_own(mesh_factory, state):
    """gscale = 1/3 on the crafted table (adam_acc_cases.unfused_table): exp_avg after one step is
    m + 0.75 (fl(gscale * acc) - m), not the fused fma(gscale, acc, -m) in its place. 515 elements:
    the last three go through the scalar tail."""
    acc, m, want_a, want_b, differs = unfused_table(515, seed=48)  # this seed: two telling elements in the tail
    assert int(differs.sum()) >= 16 and int(differs[512:].sum()) == 2
    hp = (TABLE_B1, 0.999, 1e-8, 0.0, 1e-3, 1.0)  # L2 Adam without decay: g reaches exp_avg as it is
    p0 = make_inputs(515, 3)[0]
    with _client(mesh_factory, state) as c:
        slay, glay = Layout([515], "mv"), Layout([515], "g")
        sa, ga = _alloc(c, state, slay.nbytes), _alloc(c, state, glay.nbytes)
        try:
            (_, got_m, _, _), = run_acc(sa, ga, slay, glay, [p0], [[acc]], [hp], False, THIRD, True, m0=[m])
        finally:
            ga.free()
            sa.free()
    ok = (_bits(got_m) == _bits(want_a)) | (_bits(got_m) == _bits(want_b))
    bad = ~ok & differs
    print(f"unfused table/{state}: {int(differs.sum())} telling elements, {int(bad.sum())} off; "
          f"{int((~ok).sum())} off over all {ok.numel()}")
    assert not bool(bad.any()), f"element {int(bad.nonzero()[0])}: exp_avg {got_m[bad][0].item()!r}, " \
                                f"unfused {want_a[bad][0].item()!r} / {want_b[bad][0].item()!r}"
    assert bool(ok.all())  # and on the rest, where both forms give the same


# ---- special values ----

def test_special_accumulator_values(mesh_factory):
    """+-0, +-inf, NaN, 1e-40, 1e19 and 1e30 in the accumulators (gscale 1: the gradient is the
    accumulator's bits), in the vector part and in the tail, HBM and host spaces: NaN and inf where
    torch's fp32 Adam has them, everything else within the bound (test_gpu_adam.py's check)."""
    ins = [_special_inputs(k) for k in range(3)]
    sizes = [p.numel() for p, _ in ins]
    with _client(mesh_factory, "hbm") as c:
        for state in ("hbm", "host"):
            slay, glay = Layout(sizes, "mv"), Layout(sizes, "g")
            sa, ga = _alloc(c, state, slay.nbytes), _alloc(c, state, glay.nbytes)
            try:
                for hp_name in ("default", "adamw"):  # no L2 term: g = 0 stays 0
                    hp, adamw = hyper(hp_name)
                    res = run_acc(sa, ga, slay, glay, [p for p, _ in ins], [[gs[t] for _, gs in ins] for t in range(4)],
                                  [kernel_hp(hp, adamw, t + 1) for t in range(4)], False, 1.0, True)
                    for k, (p, m, v, _) in enumerate(res):
                        _check_special((p, m, v), *ins[k], hp_name, f"acc/{state} tensor {k}")
            finally:
                ga.free()
                sa.free()


# ---- refusals before any launch ----

def test_refusals_change_nothing(mesh_factory):
    """A list whose last tensor's accumulator range leaves the half, a misaligned g_off, a
    non-finite gscale and an overlap in the shared allocation: OcmError each, and p, the state
    and the accumulators of every tensor (the earlier ones of the list too) stay bit for bit."""
    sizes = [1027, 64, 5]
    hp = kernel_hp(*hyper("default"), 1)
    ins = [make_inputs(n, 40 + n) for n in sizes]
    with _client(mesh_factory, "hbm") as c:
        slay, glay = Layout(sizes, "mvg"), Layout(sizes, "g")
        sa, ga = _alloc(c, "hbm", slay.nbytes), _alloc(c, "hbm", glay.nbytes)
        try:
            simg, gimg = slay.image(), glay.image()
            for i, (p, gs) in enumerate(ins):
                simg[slay.words(i, "m")] = gs[1].view(torch.int32)
                simg[slay.words(i, "v")] = gs[2].abs().view(torch.int32)
                simg[slay.words(i, "g")] = gs[0].view(torch.int32)
                gimg[glay.words(i, "g")] = gs[0].view(torch.int32)
            write_remote(sa, 0, 0, simg)
            write_remote(ga, 0, 0, gimg)
            pbuf, pst = _pack([p for p, _ in ins], torch.float32)
            pdev = pbuf.to(DEV)
            pv = _views(pdev, pst, sizes, False)
            mo, vo = [d["m"] for d in slay.off], [d["v"] for d in slay.off]
            own, shared = [d["g"] for d in glay.off], [d["g"] for d in slay.off]
            end = ga.remote_size()
            assert (end - 4 * sizes[-1]) % 16 != 0
            cases = {
                "range": (ga, own[:2] + [(end - 4 * sizes[-1]) // 16 * 16 + 16], 1.0),  # its last word is past the end
                "misaligned": (ga, own[:2] + [own[2] + 8], 1.0),
                "inf scale": (ga, own, float("inf")),
                "nan scale": (ga, own, float("nan")),
                "overlap": (sa, shared[:2] + [mo[2]], 1.0),
                "overlap by one vector": (sa, shared[:2] + [vo[2] + 16], 1.0),
            }
            for what, (grads, g_offs, gscale) in cases.items():
                with pytest.raises(api.OcmError):
                    sa.adam_multi_acc(pv, grads, g_offs, mo, vo, hp, gscale=gscale)
                torch.cuda.synchronize()
                assert torch.equal(read_remote(sa, 0, 0, slay.nbytes).view(torch.int32), simg), what
                assert torch.equal(read_remote(ga, 0, 0, glay.nbytes).view(torch.int32), gimg), what
                assert torch.equal(_bits(pdev.cpu()), _bits(pbuf)), what
            # the same lists, put right, run: in the shared half and in the other allocation
            sa.adam_multi_acc(pv, sa, shared, mo, vo, hp)
            sa.adam_multi_acc(pv, ga, own, mo, vo, hp, zero=False)
            torch.cuda.synchronize()
            after = read_remote(sa, 0, 0, slay.nbytes).view(torch.int32)
            assert not after[slay.words(0, "g")].any() and not torch.equal(after[slay.words(0, "m")], simg[slay.words(0, "m")])
        finally:
            ga.free()
            sa.free()


# ---- the workload ----

def _mlp(dtype):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(24, 50), torch.nn.GELU(), torch.nn.Linear(50, 3)).to(DEV, dtype)


@pytest.mark.parametrize("bf16", [False, True])
def test_training_step_reads_the_accumulators_in_place(mesh_factory, bf16):
    """A small MLP, accum = 4, three steps: OffloadedGradAccumulator(readback=False),
    add(scale = 1/4) and opt.step(accumulator=acc), beside a twin that runs the earlier sequence
    (read(), the copy into .grad, step(), zero()) on the same micro-batch gradients. fp32:
    parameters and moments equal bit for bit. bf16: the twin rounds the mean gradient to bf16 and
    the new path does not; its masters are within the bound of an fp64 replay fed the fp32
    accumulator values. After the run every accumulator is +0."""
    dtype = torch.bfloat16 if bf16 else torch.float32
    lr, accum, steps = 3e-3, 4, 3
    model, twin = _mlp(dtype), _mlp(dtype)
    params, tparams = list(model.parameters()), list(twin.parameters())
    start = [p.detach().float().cpu().reshape(-1) for p in params]
    m = mesh_factory(4, gpus=[0] * 4, policy="stripe")
    with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
        opt, topt = OffloadedAdam(params, c, lr=lr), OffloadedAdam(tparams, c, lr=lr)
        acc = OffloadedGradAccumulator(params, c, readback=False)
        tacc = OffloadedGradAccumulator(tparams, c)
        assert acc.alloc.local_tensor(torch.uint8).numel() == acc.grad_bytes + min(4 * acc.total_elems, 4 << 20)
        fed = []  # per step: the fp32 accumulator values of every parameter
        gen = torch.Generator().manual_seed(1)
        for _ in range(steps):
            tacc.zero()
            for _ in range(accum):
                x = torch.randn(32, 24, generator=gen).to(DEV, dtype)
                y = torch.randn(32, 3, generator=gen).to(DEV)
                acc.zero_grads()
                tacc.zero_grads()
                torch.nn.functional.mse_loss(model(x).float(), y).backward()
                for p, q in zip(params, tparams):
                    q.grad.copy_(p.grad)  # the twin accumulates the same micro-batch gradients
                acc.add(scale=1.0 / accum)
                tacc.add(scale=1.0 / accum)
            sums = tacc.read()
            fed.append([g.detach().float().cpu().reshape(-1).clone() for g in sums])
            with torch.no_grad():
                for q, g in zip(tparams, sums):
                    q.grad.copy_(g)
            topt.step()
            for p in params:
                p.grad = None  # not consulted
            opt.step(accumulator=acc)  # the next zero_grads() reinstalls the views
        opt.synchronize()
        topt.synchronize()
        hp = Hyper(lr, 0.9, 0.999, 1e-8, 0.0)
        for i, p in enumerate(params):
            what = f"mlp {'bf16' if bf16 else 'fp32'} parameter {i}"
            mine, theirs = opt.moments(i), topt.moments(i)
            if not bf16:
                assert torch.equal(_bits(p.detach().cpu()), _bits(tparams[i].detach().cpu())), what
                assert torch.equal(_bits(mine[0]), _bits(theirs[0])) and torch.equal(_bits(mine[1]), _bits(theirs[1])), what
                continue
            gs = [step[i] for step in fed]
            last = adam_oracle(start[i], gs, hp, False)[-1]
            t32 = torch_adam(start[i], gs, hp, False)[-1]
            terr = errors(t32, last, lr)
            master = opt.master(i).reshape(-1)
            err, limit = errors((master, mine[0].reshape(-1), mine[1].reshape(-1)), last, lr), bound(terr)
            for q in "pmv":
                print(f"adam-ratio {what} {q}: error {err[q]:.3e} torch {terr[q]:.3e}")
                assert err[q] <= limit[q], (what, q, err[q], limit[q])
            assert_bf16_rounding(p.detach().cpu().reshape(-1), master, what)
        # every accumulator is +0 (the local half is scratch from here on)
        acc.wait()
        left = read_remote(acc.alloc, 0, 0, 4 * acc.total_elems).view(torch.int32)
        assert not left.any()
        for o in (acc, tacc, opt, topt):
            o.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_train_offload_example_in_place(native, bf16):
    env = {k: v for k, v in os.environ.items() if k != "OCM_NO_GPU"}
    args = [sys.executable, os.path.join(REPO, "examples", "train_offload.py"), "--gpu", "0", "--steps", "60",
            "--accum", "4", "--accum-in-place"] + (["--bf16"] if bf16 else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd="/tmp", env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]  # the example exits non-zero unless its loss halves
    assert "mode=fused" in r.stdout and "60 steps" in r.stdout
