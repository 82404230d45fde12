"""Cases shared by the row-sparse fused-Adam tests (test_adam_rows_cpu.py, test_gpu_adam_rows.py):
the fp64 oracle, the fp32 yardstick, the numpy replay of the kernel's rule, the inputs and the
bound.

The oracle is adam_cases.adam_oracle's recurrence applied to the rows picked at each step, with the
global step in the bias corrections ("lazy" Adam: a row's moments do not move while it is not
picked). The yardstick is the same recurrence in fp32 with torch CPU ops, in torch/optim/adam.py's
single-tensor order (lerp_, mul_().addcmul_(), sqrt() / bias_correction2_sqrt + eps, addcdiv_); it
is not the code under test. The bound is adam_cases': the code under test may be at most
KERNEL_OVER_TORCH times as far from the oracle as the yardstick is, with adam_cases' FLOOR and
errors()'s scales, taken over the rows picked so far.

Largest kernel / yardstick ratios measured on an MI355X over the cases of
tests/test_gpu_adam_rows.py (the same on HBM, host-tier and striped placement, int32 and int64 ids,
the table in the state's pair or in its own): p 0.66, exp_avg 0.08, exp_avg_sq 1.00 for fp32 tables;
master 0.67, exp_avg 0.10, exp_avg_sq 1.00 for bf16 (exp_avg's yardstick error is below FLOOR, which
then is the denominator). The dense cross-check measured p 0.87, the second-round case p 0.41."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from adam_cases import FLOOR, KERNEL_OVER_TORCH, QUANTITIES, Step, bound, errors, hyper, make_inputs, ratios

TABLE_ROWS = 37
DIMS = (4, 8, 252, 256, 260, 1028)  # one vector; a part-filled wave; a full tile less a vector; a full tile;
#                                     a tile and one vector; rows of 4112 bytes (they straddle a 4096-byte unit)
HP_NAME = "default"                 # no weight decay: the row-sparse step refuses it

# The ids of the four steps on a table of 37 rows: a single id; five scattered ids; a permutation of
# all 37; a subset that repeats rows 36 and 17, picked two steps earlier (the bias corrections have
# moved on by two steps since, the rows' moments by one).
_PERM = [int(i) for i in torch.randperm(TABLE_ROWS, generator=torch.Generator().manual_seed(37))]
ID_STEPS = ([11], [3, 36, 0, 17, 24], _PERM, [36, 5, 17, 30])

Case = namedtuple("Case", "p g_tables steps last torch_last torch_err picked")


def kernel_hp_rows(hp, t):
    """The tuple Allocation.adam_rows takes for global step t (1-based): adam_cases.kernel_hp without decay."""
    return (hp.b1, hp.b2, hp.eps, 0.0, hp.lr / (1 - hp.b1 ** t), 1 / math.sqrt(1 - hp.b2 ** t))


def make_table(rows, dim, seed, bf16=False, steps=4):
    """(p, [G_1 .. G_steps]): a rows x dim table and a full gradient table per step, adam_cases.make_inputs'
    values (every element keeps its gradient magnitude over the steps), reshaped."""
    p, gs = make_inputs(rows * dim, seed, bf16, steps)
    return p.view(rows, dim), [g.view(rows, dim) for g in gs]


def rows_oracle(p, steps, hp, dtype=torch.float64):
    """steps: [(ids, g_rows)] with unique ids per step; step t (1-based) updates rows ids of p, m, v from
    zero moments with bias corrections of t. Returns a Step of tables (gmax: the largest |g| a picked
    element has seen) per step."""
    p = p.to(dtype).clone()
    m, v, gmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, (ids, g) in enumerate(steps, 1):
        ids = torch.as_tensor(ids, dtype=torch.int64)
        g = g.to(dtype)
        mi = m[ids] + (1 - hp.b1) * (g - m[ids])
        vi = hp.b2 * v[ids] + (1 - hp.b2) * g * g
        denom = vi.sqrt() / math.sqrt(1 - hp.b2 ** t) + hp.eps
        p[ids] = p[ids] - hp.lr / (1 - hp.b1 ** t) * (mi / denom)
        m[ids], v[ids] = mi, vi
        gmax[ids] = torch.maximum(gmax[ids], g.abs())
        out.append(Step(p.clone(), m.clone(), v.clone(), gmax.clone()))
    return out


def rows_torch(p, steps, hp):
    """The yardstick: torch/optim/adam.py's single-tensor update in fp32 with torch CPU ops, on the picked
    rows. (p, m, v) tables per step."""
    p = p.to(torch.float32).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, (ids, g) in enumerate(steps, 1):
        ids = torch.as_tensor(ids, dtype=torch.int64)
        param, exp_avg, exp_avg_sq, grad = p[ids], m[ids], v[ids], g.to(torch.float32)
        exp_avg.lerp_(grad, 1 - hp.b1)
        exp_avg_sq.mul_(hp.b2).addcmul_(grad, grad, value=1 - hp.b2)
        step_size = hp.lr / (1 - hp.b1 ** t)
        bias_correction2_sqrt = math.sqrt(1 - hp.b2 ** t)
        denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(hp.eps)
        param.addcdiv_(exp_avg, denom, value=-step_size)
        p[ids], m[ids], v[ids] = param, exp_avg, exp_avg_sq
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def rows_rule_fp32(p, steps, hp, gscale=1.0):
    """adam1() of csrc/src/kernels/adam_rule.h on the picked rows in numpy fp32, one rounding per operation
    in the kernel's order, the gradient fl32(gscale * g) first: adam_cases.adam_rule_fp32's approach, by
    rows. Not bit-exact with the GPU (hipcc contracts to FMA). (p, m, v) tables per step."""
    f = np.float32
    omb1, omb2, fb2, eps = f(1 - hp.b1), f(1 - hp.b2), f(hp.b2), f(hp.eps)
    p = p.numpy().astype(f).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    with np.errstate(all="ignore"):
        for t, (ids, g) in enumerate(steps, 1):
            ids = np.asarray(ids, dtype=np.int64)
            g = f(gscale) * g.numpy().astype(f)
            step_size, inv_sqrt_bc2 = f(hp.lr / (1 - hp.b1 ** t)), f(1 / math.sqrt(1 - hp.b2 ** t))
            mi = m[ids] + omb1 * (g - m[ids])
            vi = fb2 * v[ids] + omb2 * g * g
            denom = np.sqrt(vi) * inv_sqrt_bc2 + eps
            p[ids] = p[ids] - step_size * (mi / denom)
            m[ids], v[ids] = mi, vi
            assert p.dtype == m.dtype == v.dtype == f
            out.append(tuple(torch.from_numpy(x.copy()) for x in (p, m, v)))
    return out


def picked_mask(rows, dim, steps):
    mask = torch.zeros(rows, dim, dtype=torch.bool)
    for ids, _ in steps:
        mask[torch.as_tensor(ids, dtype=torch.int64)] = True
    return mask


def build_case(p, g_tables, id_steps):
    """The inputs, the oracle's and the yardstick's last step and the yardstick's error, for tables p /
    g_tables and the ids of each step."""
    hp, _ = hyper(HP_NAME)
    steps = tuple((tuple(ids), g_tables[s][torch.as_tensor(ids, dtype=torch.int64)]) for s, ids in enumerate(id_steps))
    picked = picked_mask(p.shape[0], p.shape[1], steps)
    last, t32 = rows_oracle(p, steps, hp)[-1], rows_torch(p, steps, hp)[-1]
    return Case(p, tuple(g_tables), steps, last, t32, errors(t32, last, hp.lr, picked), picked)


@functools.lru_cache(maxsize=None)
def case(dim, bf16=False, rows=TABLE_ROWS, n_steps=4):
    """The four-step case on a `rows` x dim table (ID_STEPS), computed once and shared; callers leave
    the tensors unchanged."""
    p, gs = make_table(rows, dim, 1000 + dim, bf16)
    return build_case(p, gs, ID_STEPS[:n_steps])


def check_rows(got, c, what, log=None):
    """(p, m, v) tables after the last step against the case's oracle on the picked rows, within the
    bound. Prints every ratio before it asserts; appends (what, quantity, ratio) to `log`."""
    hp, _ = hyper(HP_NAME)
    err = errors(got, c.last, hp.lr, c.picked)
    r, b = ratios(err, c.torch_err), bound(c.torch_err)
    for q in QUANTITIES:
        print(f"adam-rows-ratio {what} {q}: error {err[q]:.3e} torch {c.torch_err[q]:.3e} ratio {r[q]:.2f}")
        if log is not None:
            log.append((what, q, r[q]))
    for q in QUANTITIES:
        assert err[q] <= b[q], (f"{what}: {q} error {err[q]:.3e} > {b[q]:.3e} = {KERNEL_OVER_TORCH} x max(yardstick's "
                                f"{c.torch_err[q]:.3e}, {FLOOR:.3e})")
