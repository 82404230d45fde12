"""Cases shared by the fused-Adam tests (test_adam_cpu.py, test_gpu_adam.py): the fp64
oracle, the fp32 replay of the kernel's rule, the inputs, the error measures and their
bound, the hyper-parameter sets and the crafted bf16 rounding table.

The bound is not a fixed tolerance. Every comparison also runs torch's own fp32
single-tensor Adam / AdamW on the CPU on the same inputs and measures its error against the
same fp64 oracle; the code under test may be at most KERNEL_OVER_TORCH times as far off
(each error taken as the maximum over the tensor, with a floor of 2^-22)."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

Hyper = namedtuple("Hyper", "lr b1 b2 eps wd")
Step = namedtuple("Step", "p m v gmax")  # after one step; gmax: largest |effective g| so far, per element

STEPS = 4
HP_SETS = {  # name -> (Hyper, adamw)
    "default": (Hyper(1e-3, 0.9, 0.999, 1e-8, 0.0), False),
    "default_l2": (Hyper(1e-3, 0.9, 0.999, 1e-8, 0.01), False),
    "fast_l2": (Hyper(1e-2, 0.8, 0.95, 1e-6, 0.01), False),
    "adamw": (Hyper(1e-3, 0.9, 0.999, 1e-8, 0.05), True),
    "slow_b2": (Hyper(1e-3, 0.9, 0.9999, 1e-8, 0.0), False),  # 1.f - float(b2) is 1.7e-4 off
    "adamw_full_decay": (Hyper(0.5, 0.9, 0.999, 1e-8, 2.0), True),  # lr * wd == 1: decay multiplier exactly 0
}

# The kernel may differ from torch's fp32 update by a reciprocal-multiply in the bias
# correction (sqrt(v) * (1/sqrt(bc2)) for sqrt(v) / sqrt(bc2)) and by FMA contraction, about
# one ulp each per step, so it gets 4 times torch's own error against the fp64 oracle.
# Measured kernel / torch ratios, largest over the cases of tests/test_gpu_adam.py on an MI355X
# (the same on HBM, host-tier and striped state): p 1.04, exp_avg 1.00, exp_avg_sq 1.00 for
# fp32 (single and multi); master 1.12, exp_avg 0.50, exp_avg_sq 1.00 for bf16. The fp32 replay
# below (adam_rule_fp32, no FMA) reaches 2.1 on the same cases. With the complements taken as
# 1.f - float(beta) the replay's exp_avg_sq is at 55x ("default") and 700x ("slow_b2"); the
# kernel that did so measured 521x on exp_avg_sq and 1008x on p ("slow_b2", n = 1027), 0.28 on
# exp_avg.
KERNEL_OVER_TORCH = 4.0
FLOOR = 2.0 ** -22  # a lucky exact torch result cannot make the bound zero
FLT_MIN = 2.0 ** -126
QUANTITIES = ("p", "m", "v")


def hyper(name):
    return HP_SETS[name]


def kernel_hp(hp, adamw, t):
    """The tuple Allocation.adam / adam_multi take for step t (1-based), from Python doubles."""
    return (hp.b1, hp.b2, hp.eps, hp.wd, hp.lr / (1 - hp.b1 ** t), 1 / math.sqrt(1 - hp.b2 ** t),
            (1 - hp.lr * hp.wd) if adamw else math.nan)


def make_inputs(n, seed, bf16=False, steps=STEPS):
    """(p, [g_1 .. g_steps]) as fp32 tensors: p ~ randn, every g randn times a per-element
    magnitude 10^k, k in {-3 .. 1}, that stays put over the steps (so 'the largest |g| so far'
    is a scale of the element). bf16: all values bf16-representable."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    mag = 10.0 ** torch.randint(-3, 2, (n,), generator=gen).float()
    gs = [torch.randn(n, generator=gen) * mag for _ in range(steps)]
    if bf16:
        p = p.to(torch.bfloat16).float()
        gs = [g.to(torch.bfloat16).float() for g in gs]
    return p, gs


def adam_oracle(p, g_list, hp, adamw, dtype=torch.float64):
    """The plain Adam / AdamW recurrence as in torch/optim/adam.py's single-tensor path, from
    zero moments, in `dtype` with Python-double hyper-parameters. Returns a Step per step. For
    bf16 parameters pass bf16-valued p and g: p is then the fp32-master recurrence's value and
    the parameter is its rounding to bf16."""
    p = p.to(dtype).clone()
    m, v, gmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, g in enumerate(g_list, 1):
        g = g.to(dtype)
        if adamw:
            p = p * (1 - hp.lr * hp.wd)
        elif hp.wd != 0:
            g = g + hp.wd * p
        m = m + (1 - hp.b1) * (g - m)
        v = hp.b2 * v + (1 - hp.b2) * g * g
        denom = v.sqrt() / math.sqrt(1 - hp.b2 ** t) + hp.eps
        p = p - hp.lr / (1 - hp.b1 ** t) * (m / denom)
        gmax = torch.maximum(gmax, g.abs())
        out.append(Step(p.clone(), m.clone(), v.clone(), gmax.clone()))
    return out


def torch_adam(p, g_list, hp, adamw, dtype=torch.float32):
    """torch.optim.Adam / AdamW itself (single-tensor path, CPU) in `dtype`: (p, m, v) per step."""
    q = p.to(dtype).clone().requires_grad_()
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    opt = cls([q], lr=hp.lr, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd, foreach=False)
    out = []
    for g in g_list:
        q.grad = g.to(dtype).clone()
        opt.step()
        st = opt.state[q]
        out.append((q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


MUTATIONS = ("eps_in_sqrt", "no_bc2", "l2_after_moments", "adamw_decay_in_grad", "swap_betas")


def adam_rule_fp32(p, g_list, hp, adamw, one_minus_b1, one_minus_b2, mutation=None):
    """adam1() of csrc/src/kernels/optim.hip in numpy fp32, one rounding per operation in the
    kernel's order: the CPU stand-in for the kernel. Not bit-exact with the GPU (hipcc contracts
    to FMA). The complements are parameters: np.float32(1 - b) is the kernel's, np.float32(1) -
    np.float32(b) its predecessor's. `mutation`: one of MUTATIONS, a deliberately wrong rule.
    Returns (p, m, v) as fp32 tensors per step."""
    f = np.float32
    b1, b2 = (hp.b2, hp.b1) if mutation == "swap_betas" else (hp.b1, hp.b2)
    omb1, omb2 = (one_minus_b2, one_minus_b1) if mutation == "swap_betas" else (one_minus_b1, one_minus_b2)
    omb1, omb2, fb2, eps, wd = f(omb1), f(omb2), f(b2), f(hp.eps), f(hp.wd)
    p = p.numpy().astype(f).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    with np.errstate(all="ignore"):
        for t, g in enumerate(g_list, 1):
            g = g.numpy().astype(f)
            step_size = f(hp.lr / (1 - b1 ** t))
            inv_sqrt_bc2 = f(1.0) if mutation == "no_bc2" else f(1 / math.sqrt(1 - b2 ** t))
            if adamw and mutation == "adamw_decay_in_grad":
                g = g + wd * p
            elif adamw:
                p = p * f(1 - hp.lr * hp.wd)
            elif wd != 0 and mutation != "l2_after_moments":
                g = g + wd * p
            m = m + omb1 * (g - m)
            v = fb2 * v + omb2 * g * g
            if mutation == "eps_in_sqrt":
                denom = np.sqrt(v + eps) * inv_sqrt_bc2
            else:
                denom = np.sqrt(v) * inv_sqrt_bc2 + eps
            upd = m / denom
            if mutation == "l2_after_moments" and not adamw:
                upd = upd + wd * p  # the decay joins the step, past the moments
            p = p - step_size * upd
            assert p.dtype == m.dtype == v.dtype == f
            out.append((torch.from_numpy(p.copy()), torch.from_numpy(m.copy()), torch.from_numpy(v.copy())))
    return out


def errors(got, want, lr, mask=None):
    """Largest per-element error of (p, m, v) `got` against the oracle Step `want`:
    v relative (a sum of non-negatives: no cancellation); m absolute over the element's largest
    |effective g| so far; p absolute over max(|p|, lr). Scales below the smallest normal fp32
    count as that, so a denormal's fixed spacing is not taken for a relative error. `mask`:
    the elements to look at (default all)."""
    d = torch.float64
    scale = {"p": want.p.abs().clamp_min(lr), "m": want.gmax.clamp_min(FLT_MIN), "v": want.v.clamp_min(FLT_MIN)}
    out = {}
    for q, g in zip(QUANTITIES, got):
        e = (g.to(d) - getattr(want, q)).abs() / scale[q]
        if mask is not None:
            e = e[mask]
        e = torch.nan_to_num(e, nan=math.inf)  # a NaN where the oracle is finite is an error of any size
        out[q] = float(e.max()) if e.numel() else 0.0
    return out


def bound(torch_err):
    return {q: KERNEL_OVER_TORCH * max(torch_err[q], FLOOR) for q in QUANTITIES}


def ratios(err, torch_err):
    return {q: err[q] / max(torch_err[q], FLOOR) for q in QUANTITIES}


Reference = namedtuple("Reference", "p g_list last torch_last torch_err")


@functools.lru_cache(maxsize=None)
def reference(n, seed, hp_name, bf16=False):
    """Inputs, the oracle's last Step, torch's fp32 (p, m, v) after the last step and torch's
    errors against the oracle, computed once per (n, seed, set, bf16) and shared; callers must
    leave the tensors unchanged."""
    hp, adamw = HP_SETS[hp_name]
    p, gs = make_inputs(n, seed, bf16)
    last = adam_oracle(p, gs, hp, adamw)[-1]
    t32 = torch_adam(p, gs, hp, adamw)[-1]
    return Reference(p, tuple(gs), last, t32, errors(t32, last, hp.lr))


def check(got, ref, hp_name, what, log=None):
    """(p, m, v) after the last step against ref's oracle, within the bound. Prints every ratio
    before it asserts; appends (what, quantity, ratio) to `log`."""
    hp, _ = HP_SETS[hp_name]
    err = errors(got, ref.last, hp.lr)
    r, b = ratios(err, ref.torch_err), bound(ref.torch_err)
    for q in QUANTITIES:
        print(f"adam-ratio {what} {hp_name} {q}: error {err[q]:.3e} torch {ref.torch_err[q]:.3e} ratio {r[q]:.2f}")
        if log is not None:
            log.append((what, q, r[q]))
    for q in QUANTITIES:
        assert err[q] <= b[q], f"{what} {hp_name}: {q} error {err[q]:.3e} > {b[q]:.3e} = {KERNEL_OVER_TORCH} x torch's {ref.torch_err[q]:.3e}"


# ---- bf16 round-to-nearest-even ----

def bf16_table(n=71, seed=5):
    """n fp32 bit patterns (int32 tensor): the crafted ones first, seeded normal values after."""
    crafted = [
        0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to the even neighbour, down and up
        0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,  # just above and just below a tie
        0xBF808001, 0xBF807FFF,
        0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,  # the largest finite values: to inf, or not
        0x7F800000, 0xFF800000, 0x00000000, 0x80000000,  # +-inf, +-0
        0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x80018000,  # denormals
        0x7FC00000, 0x7F800001, 0xFFC00001, 0x7F80FFFF,  # NaNs, two with the payload in the dropped half only
    ]
    assert len(crafted) <= n
    g = torch.Generator().manual_seed(seed)
    fill = (torch.randn(n - len(crafted), generator=g) * 100.0).view(torch.int32)
    t = torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in crafted], dtype=torch.int32)
    return torch.cat([t, fill])


def f32_to_bf16_np(bits):
    """f32_to_bf16() of optim.hip on uint32 bit patterns (numpy): uint16 patterns."""
    u = np.asarray(bits).astype(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def assert_bf16_rounding(p_bf16, master_f32, what=""):
    """p (bf16 tensor) is master.to(bfloat16) bit for bit; where the master is NaN, some NaN."""
    want = master_f32.to(torch.bfloat16)
    nan = torch.isnan(master_f32)
    assert torch.isnan(p_bf16[nan].float()).all(), (what, "NaN expected")
    g, w = p_bf16[~nan].view(torch.int16), want[~nan].view(torch.int16)
    if not torch.equal(g, w):
        i = int((g != w).nonzero()[0])
        raise AssertionError(f"{what}: element {i} of the non-NaN ones: 0x{int(g[i]) & 0xffff:04x}, expected 0x{int(w[i]) & 0xffff:04x}")
