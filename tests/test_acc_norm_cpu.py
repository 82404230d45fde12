"""Gradient clipping over remote accumulators, checked without a GPU: api.clip_scale against the
coefficient torch.nn.utils.clip_grad_norm_ applies to CPU tensors, and the refusals that need no
kernel. What runs the reduction is tests/test_gpu_acc_norm.py."""
import math

import numpy as np
import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import OffloadedAdam, OffloadedGradAccumulator


def _torch_coefficient(grads, max_norm):
    """What clip_grad_norm_ multiplies the gradients by, read off an element it leaves nonzero."""
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    flat, after = torch.cat([g.reshape(-1) for g in grads]), torch.cat([p.grad.reshape(-1) for p in ps])
    i = int(flat.abs().argmax())
    return float(after[i]) / float(flat[i]), float(norm), after, flat


@pytest.mark.parametrize("max_norm", [1e-3, 0.5, 1.0, 7.0, 1e9])
@pytest.mark.parametrize("seed", [0, 1])
def test_clip_scale_is_torchs_coefficient(seed, max_norm):
    """The same clamp (exactly 1 where torch does not clip) and, where it clips, the double-computed
    coefficient within fp32 rounding of torch's: torch sums n squares in fp32 (n * 2^-24 relative on
    the sum of squares, half of that on the norm), rounds max_norm, the sum with 1e-6 and the
    quotient (2^-24 each), and the product read back here (2^-24)."""
    gen = torch.Generator().manual_seed(seed)
    grads = [torch.randn(n, generator=gen) * 3.0 for n in (1027, 5, 64)]
    n = sum(g.numel() for g in grads)
    sumsq = math.fsum(float(x) ** 2 for g in grads for x in g.double())
    coef, tnorm, after, flat = _torch_coefficient(grads, max_norm)
    mine = api.clip_scale(sumsq, 1.0, max_norm)
    assert abs(tnorm - math.sqrt(sumsq)) <= n * 2.0 ** -24 * math.sqrt(sumsq)
    if math.sqrt(sumsq) + 1e-6 <= max_norm * (1 - n * 2.0 ** -24):  # clearly below: both leave the gradient alone
        assert mine == 1.0 and torch.equal(after, flat)
    else:
        assert mine < 1.0 and coef < 1.0
        assert abs(mine - coef) <= (n / 2 + 4) * 2.0 ** -24 * mine, (mine, coef)
    # a scale in front: the norm is of scale * acc, and the result carries the scale
    assert api.clip_scale(sumsq, 0.25, max_norm) == 0.25 * min(1.0, max_norm / (0.25 * math.sqrt(sumsq) + 1e-6))
    assert api.clip_scale(sumsq, -0.25, max_norm) == -api.clip_scale(sumsq, 0.25, max_norm)


def test_clip_scale_edges():
    assert api.clip_scale(0.0, 0.5, 1.0) == 0.5                      # zero norm
    assert api.clip_scale(25.0, 1.0, 5.0) == 5.0 / (5.0 + 1e-6)      # torch's 1e-6 clips a norm equal to max_norm
    assert api.clip_scale(25.0, 1.0, 5.000001) == 1.0
    assert api.clip_scale(float("inf"), 1.0, 1.0) == 0.0
    assert math.isnan(api.clip_scale(float("nan"), 1.0, 1.0))
    # rounded to fp32 once, where it becomes gscale: the double result is not an fp32 value
    x = api.clip_scale(25.0, 1.0, 1.0)
    assert float(np.float32(x)) != x


@pytest.fixture
def client(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(4, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        yield c


def test_acc_sumsq_needs_a_gpu(client):
    params = [torch.nn.Parameter(torch.randn(64)), torch.nn.Parameter(torch.randn(5))]
    acc = OffloadedGradAccumulator(params, client, readback=False)
    with pytest.raises(api.OcmError):
        acc.alloc.acc_sumsq([0, 256], [64, 5])
    with pytest.raises(api.OcmError):
        acc.sumsq()
    with pytest.raises(api.OcmError):
        acc.grad_norm()
    # the hook itself refuses too, whatever it is handed, before it looks at the outputs
    out = (torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.int64), torch.zeros(1 << 16, dtype=torch.uint8))
    with pytest.raises(api.OcmError, match="needs a GPU"):
        acc.alloc._acc_sumsq_into([0, 256], [64, 5], *out, stream=0)
    assert client.lib.ocm_x_acc_sumsq_work_bytes(2) == 0
    acc.close()


def test_clipping_needs_an_accumulator(client):
    params = [torch.nn.Parameter(torch.randn(64))]
    opt = OffloadedAdam(params, client, mode="staged")
    params[0].grad = torch.randn(64)
    for kw in ({"max_norm": 1.0}, {"skip_nonfinite": True}, {"max_norm": 1.0, "skip_nonfinite": True}):
        with pytest.raises(ValueError):
            opt.step(**kw)
    assert opt.t == 0
    assert opt.step() is None and opt.t == 1  # neither argument: today's path, today's return value
    opt.close()
