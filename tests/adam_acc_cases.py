"""Cases shared by the tests of the fused Adam that reads its gradient from remote fp32
accumulators (test_adam_acc_cpu.py, test_gpu_adam_acc.py): the scale as one fp32 rounding of
its own, and a crafted table on which that differs from a fused multiply-subtract."""
import numpy as np
import torch

SCALES = (1.0, 0.25, 1.0 / 3.0)
TABLE_B1 = 0.25  # 1 - b1 = 0.75: exact in fp32, and large enough to carry half an ulp of g - m into exp_avg


def scaled(acc, gscale):
    """fl32(gscale * acc): one IEEE fp32 multiply by the fp32 value of gscale, rounded to
    nearest even, subnormals kept (numpy on the CPU). What adam1 is then fed."""
    with np.errstate(all="ignore"):
        return torch.from_numpy(acc.numpy().astype(np.float32) * np.float32(gscale))


def unfused_table(n=512, seed=21, gscale=1.0 / 3.0):
    """acc and exp_avg values on which rounding the scale on its own shows in the next exp_avg.

    m is fl(gscale * acc) moved by a few ulps, so g - m cancels down to a few ulps: the rule's
    d = fl(fl(gscale * acc) - m) is exact, the fused fma(gscale, acc, -m) keeps the product's
    rounding error, up to half an ulp more or less. exp_avg' = m + 0.75 d carries three quarters
    of that. The kernel may or may not contract exp_avg's own m + omb1 * d (adam_cases:
    'hipcc contracts to FMA'), so each d gives two candidates, with one rounding and with two.
    All of it in float64, where products of fp32 values and these sums are exact.

    Returns (acc, m, want_a, want_b, differs): fp32 tensors; want_a / want_b are the two
    candidates from the unfused d; `differs` marks the elements where neither equals either
    candidate from the fused d (at least 16)."""
    gen = torch.Generator().manual_seed(seed)
    a = ((torch.rand(n, generator=gen) + 1.0) * 3.0).numpy()
    s32, omb1 = np.float32(gscale), np.float32(1 - TABLE_B1)
    g = a * s32                                          # fp32: rounded on its own
    ulps = torch.randint(-4, 5, (n,), generator=gen).numpy().astype(np.int32)
    m = (g.view(np.int32) + ulps).view(np.float32)
    f64 = np.float64

    def candidates(d32):
        once = (m.astype(f64) + f64(omb1) * d32.astype(f64)).astype(np.float32)   # fma(omb1, d, m)
        twice = m + (omb1 * d32)                                                  # fp32 product, fp32 sum
        return once, twice

    d_rule = g - m                                                                # exact: a few ulps
    d_fused = (a.astype(f64) * f64(s32) - m.astype(f64)).astype(np.float32)
    (ra, rb), (fa, fb) = candidates(d_rule), candidates(d_fused)
    differs = (ra != fa) & (ra != fb) & (rb != fa) & (rb != fb)
    assert int(differs.sum()) >= 16, int(differs.sum())
    t = torch.from_numpy
    return t(a.copy()), t(m.copy()), t(ra.copy()), t(rb.copy()), t(differs)
