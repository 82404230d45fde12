"""The fused Adam that reads its gradient from remote fp32 accumulators, checked without a GPU:
the rule (g = fl32(gscale * acc), then the unchanged update) inside adam_cases' bound of the fp64
oracle, the descriptor arithmetic of OffloadedAdam.step(accumulator=...) with the native call
stubbed, and OffloadedGradAccumulator(readback=False) on a CPU mesh. What runs the kernel is
tests/test_gpu_adam_acc.py."""
import numpy as np
import pytest
import torch

from adam_acc_cases import SCALES, TABLE_B1, scaled, unfused_table
from adam_cases import QUANTITIES, STEPS, adam_oracle, adam_rule_fp32, bound, errors, hyper, make_inputs, torch_adam
from oncilla_amd import api
from oncilla_amd.models import OffloadedAdam, OffloadedGradAccumulator
from quant_cases import read_remote

N, SEED = 4099, 11


@pytest.mark.parametrize("gscale", SCALES)
@pytest.mark.parametrize("hp_name", ["default_l2", "adamw"])
def test_rule_within_the_bound(gscale, hp_name):
    """fl(gscale * acc), then adam_cases.adam_rule_fp32. The oracle and torch's fp32 Adam are fed
    the same rounded gradient, so the bound measures the update, not the scale."""
    hp, adamw = hyper(hp_name)
    p, accs = make_inputs(N, SEED)
    gs = [scaled(a, gscale) for a in accs]
    if gscale == 1.0:
        assert all(torch.equal(g.view(torch.int32), a.view(torch.int32)) for g, a in zip(gs, accs))
    orc, t32 = adam_oracle(p, gs, hp, adamw), torch_adam(p, gs, hp, adamw)
    got = adam_rule_fp32(p, gs, hp, adamw, np.float32(1 - hp.b1), np.float32(1 - hp.b2))
    for s in range(STEPS):
        b, e = bound(errors(t32[s], orc[s], hp.lr)), errors(got[s], orc[s], hp.lr)
        for q in QUANTITIES:
            assert e[q] <= b[q], (gscale, hp_name, s, q, e[q], b[q])


def test_scale_keeps_subnormals_and_rounds_once():
    acc = torch.tensor([1e-40, -1e-40, 3.0, 1e-38], dtype=torch.float32)
    assert torch.equal(scaled(acc, 1.0).view(torch.int32), acc.view(torch.int32))
    third = scaled(acc, 1.0 / 3.0)
    assert float(third[0]) != 0.0 and float(third[3]) < 2.0 ** -126  # a subnormal result is kept
    assert float(third[2]) == float(np.float32(3.0) * np.float32(1.0 / 3.0))


def test_unfused_table():
    acc, m, want_a, want_b, differs = unfused_table()
    assert int(differs.sum()) >= 16 and acc.dtype == m.dtype == want_a.dtype == torch.float32
    # exp_avg of the fp32 replay (two roundings in the lerp) is the second candidate
    g = scaled(acc, 1.0 / 3.0).numpy()
    assert np.array_equal(m.numpy() + np.float32(1 - TABLE_B1) * (g - m.numpy()), want_b.numpy())


# ---- OffloadedAdam.step(accumulator=...) with the native call stubbed ----

class _FakeAlloc:
    def __init__(self, local_bytes):
        self.buf = torch.zeros(local_bytes, dtype=torch.uint8)
        self.calls = []

    def local_tensor(self, dtype=None):
        return self.buf.view(dtype) if dtype else self.buf

    def put(self, *a, **kw):
        pass

    def adam_multi_acc(self, ps, grads_alloc, g_offs, m_offs, v_offs, hp, gscale=1.0, zero=True, w_offs=None, stream=None):
        self.calls.append(dict(ps=ps, grads=grads_alloc, g=list(g_offs), m=list(m_offs), v=list(v_offs), hp=hp,
                               gscale=gscale, zero=zero, w=w_offs))

    def adam_multi(self, *a, **kw):
        raise AssertionError("the local-gradient path ran")


class _FakeGpuClient:
    device = 0

    def alloc(self, kind, local_bytes, remote_bytes, **kw):
        self.made = _FakeAlloc(local_bytes)
        return self.made


@pytest.fixture
def client(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(4, policy="stripe")
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        yield c


class _NoStream:
    def synchronize(self):
        pass


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_descriptors(client, monkeypatch, dtype):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **kw: _NoStream())
    sizes = [5, 64, 1030, 3]
    params = [torch.nn.Parameter(torch.randn(n).to(dtype)) for n in sizes]
    acc = OffloadedGradAccumulator(params, client, readback=False)
    fake = _FakeGpuClient()
    opt = OffloadedAdam(params, fake, lr=1e-3, mode="fused")
    for p in params:
        p.grad = None  # not consulted
    opt.step(accumulator=acc, scale=0.25, zero=False)
    opt.step(accumulator=acc)
    first, second = fake.made.calls
    # accumulator slots: every tensor padded to 4 elements
    assert first["g"] == [0, 4 * 8, 4 * (8 + 64), 4 * (8 + 64 + 1032)] == [4 * s[1] for s in acc._slots]
    pad = opt.padded
    assert pad == 64 + 64 + 1088 + 64 and opt.starts == [0, 64, 128, 1216]
    assert first["m"] == [4 * s for s in opt.starts] and first["v"] == [4 * (pad + s) for s in opt.starts]
    assert first["w"] == ([4 * (2 * pad + s) for s in opt.starts] if dtype == torch.bfloat16 else None)
    assert first["grads"] is acc.alloc and [p.data_ptr() for p in first["ps"]] == [p.data_ptr() for p in params]
    assert (first["gscale"], first["zero"], second["gscale"], second["zero"]) == (0.25, False, 1.0, True)
    # the bias corrections follow the step count
    assert opt.t == 2 and first["hp"][4] == 1e-3 / (1 - 0.9) and second["hp"][4] == 1e-3 / (1 - 0.9 ** 2)
    # another order, another list: refused before the step counts
    other = OffloadedGradAccumulator(params[::-1], client, readback=False)
    fewer = OffloadedGradAccumulator(params[:3], client, readback=False)
    for bad in (other, fewer):
        with pytest.raises(ValueError):
            opt.step(accumulator=bad)
    assert opt.t == 2 and len(fake.made.calls) == 2
    for a in (acc, other, fewer):
        a.close()


def test_staged_mode_is_refused(client):
    params = [torch.nn.Parameter(torch.randn(64))]
    acc = OffloadedGradAccumulator(params, client, readback=False)
    opt = OffloadedAdam(params, client, mode="staged")
    with pytest.raises(ValueError):
        opt.step(accumulator=acc)
    assert opt.t == 0
    opt.close()
    acc.close()


# ---- OffloadedGradAccumulator(readback=False) ----

@pytest.mark.parametrize("chunk", [None, 1024])
def test_accumulator_without_readback(client, monkeypatch, chunk):
    """chunk None: the zero chunk covers all accumulators (one put). 1024: five puts, the last
    one short (4416 bytes of accumulators)."""
    if chunk:
        monkeypatch.setattr(OffloadedGradAccumulator, "_ZERO_CHUNK", chunk)
    sizes = [5, 64, 1030]
    params = [torch.nn.Parameter(torch.randn(n)) for n in sizes]
    acc = OffloadedGradAccumulator(params, client, readback=False)
    total = 8 + 64 + 1032
    assert acc.total_elems == total and acc.grad_bytes == 4 * total
    assert acc.local_bytes == acc.grad_bytes + min(4 * total, chunk or (4 << 20))
    assert acc.alloc.local_tensor(torch.uint8).numel() == acc.local_bytes and acc.alloc.remote_size() == 4 * total
    with_region = OffloadedGradAccumulator([torch.nn.Parameter(torch.randn(n)) for n in sizes], client)
    assert with_region.local_bytes == with_region.grad_bytes + 4 * total  # the default is as it was
    with_region.close()
    with pytest.raises(RuntimeError):
        acc.read()
    for p in params:
        p.grad.fill_(-1.5)
    acc.add(scale=2.0, async_=False)
    words = read_remote(acc.alloc, 0, 0, 4 * total).view(torch.float32)
    assert float(words[0]) == -3.0 and float(words[total - 3]) == -3.0
    acc.zero()
    words = read_remote(acc.alloc, 0, 0, 4 * total).view(torch.int32)
    assert not words.any()  # +0: every bit clear
    acc.close()
