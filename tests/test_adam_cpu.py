"""The fused-Adam oracle and bound (tests/adam_cases.py) checked on the CPU: the fp64 oracle
against torch in float64, the fp32 replay of the kernel's rule inside the bound for every
hyper-parameter set, six wrong rules outside it, and the bf16 rounding port on the crafted
table; and what every optimizer hook says to a handle that is no live allocation. No GPU: what
runs the kernels themselves is tests/test_gpu_adam.py."""
import ctypes

import numpy as np
import pytest
import torch

from oncilla_amd import api

from adam_cases import (HP_SETS, MUTATIONS, QUANTITIES, STEPS, adam_oracle, adam_rule_fp32, bf16_table, bound, errors,
                        f32_to_bf16_np, hyper, kernel_hp, make_inputs, reference, torch_adam)

N, SEED = 4099, 11


def _worst_ratio(hp_name, one_minus=None, mutation=None, bf16=False):
    """Largest error / bound over the steps, per quantity, of the fp32 replay on one set.
    one_minus: (hp -> (1 - b1, 1 - b2) as fp32); default: rounded once from double."""
    hp, adamw = hyper(hp_name)
    p, gs = make_inputs(N, SEED, bf16)
    orc, t32 = adam_oracle(p, gs, hp, adamw), torch_adam(p, gs, hp, adamw)
    o1, o2 = one_minus(hp) if one_minus else (np.float32(1 - hp.b1), np.float32(1 - hp.b2))
    got = adam_rule_fp32(p, gs, hp, adamw, o1, o2, mutation)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for s in range(STEPS):
        b, e = bound(errors(t32[s], orc[s], hp.lr)), errors(got[s], orc[s], hp.lr)
        for q in QUANTITIES:
            worst[q] = max(worst[q], e[q] / b[q])
    return worst


def _parent_complements(hp):
    return np.float32(1) - np.float32(hp.b1), np.float32(1) - np.float32(hp.b2)


@pytest.mark.parametrize("hp_name", list(HP_SETS))
def test_oracle_is_torch_in_float64(hp_name):
    hp, adamw = hyper(hp_name)
    p, gs = make_inputs(N, SEED)
    for mine, (tp, tm, tv) in zip(adam_oracle(p, gs, hp, adamw), torch_adam(p, gs, hp, adamw, dtype=torch.float64)):
        torch.testing.assert_close(mine.p, tp, rtol=1e-12, atol=0)
        torch.testing.assert_close(mine.m, tm, rtol=1e-12, atol=0)
        torch.testing.assert_close(mine.v, tv, rtol=1e-12, atol=0)
    assert float(mine.gmax.min()) > 0


def test_inputs_and_hp_tuple():
    p, gs = make_inputs(N, SEED)
    assert len(gs) == STEPS and p.dtype == gs[0].dtype == torch.float32
    pb, gb = make_inputs(N, SEED, bf16=True)
    assert torch.equal(pb, pb.to(torch.bfloat16).float()) and torch.equal(gb[2], gb[2].to(torch.bfloat16).float())
    hp, _ = hyper("adamw_full_decay")
    assert kernel_hp(hp, True, 1)[6] == 0.0  # lr * wd == 1: the weights are fully decayed
    assert np.isnan(kernel_hp(hp, False, 1)[6])
    assert reference(N, SEED, "default") is reference(N, SEED, "default")  # computed once, shared


def test_api_hands_the_kernel_complements_rounded_once():
    from oncilla_amd.api import _adam_hp

    hp, _ = hyper("slow_b2")
    h6, h7 = _adam_hp(kernel_hp(hp, False, 3)[:6]), _adam_hp(kernel_hp(hp, True, 3))
    assert len(h6) == len(h7) == 9 and np.isnan(h6[6]) and h7[6] == 1 - hp.lr * hp.wd
    for h in (h6, h7):
        assert h[7] == 1 - hp.b1 and h[8] == 1 - hp.b2
        assert np.float32(h[8]) != np.float32(1) - np.float32(hp.b2)  # what the kernel used to compute
    with pytest.raises(ValueError):
        _adam_hp((0.9, 0.999, 1e-8))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("hp_name", list(HP_SETS))
def test_kernel_rule_in_fp32_is_within_the_bound(hp_name, bf16):
    worst = _worst_ratio(hp_name, bf16=bf16)
    print(f"adam_rule_fp32 {hp_name} bf16={bf16}: error / bound {worst}")
    assert all(worst[q] <= 1.0 for q in QUANTITIES), worst


# mutation -> (hyper-parameter set, quantity) that must leave the bound; the other sets and
# quantities may or may not notice.
CAUGHT_BY = {
    "parent_complements": ("slow_b2", "v"),
    "eps_in_sqrt": ("default", "p"),
    "no_bc2": ("default", "p"),
    "l2_after_moments": ("default_l2", "m"),
    "adamw_decay_in_grad": ("adamw", "m"),
    "swap_betas": ("fast_l2", "v"),
}


@pytest.mark.parametrize("mutation", list(CAUGHT_BY))
def test_mutations_leave_the_bound(mutation):
    hp_name, q = CAUGHT_BY[mutation]
    if mutation == "parent_complements":
        worst = _worst_ratio(hp_name, one_minus=_parent_complements)
    else:
        assert mutation in MUTATIONS
        worst = _worst_ratio(hp_name, mutation=mutation)
    print(f"{mutation} on {hp_name}: error / bound {worst}")
    assert worst[q] > 1.0, f"{mutation} not caught on {q} of {hp_name}: {worst}"


def test_parent_complements_are_caught_on_the_default_betas_too():
    # 1.f - float(0.999): exp_avg_sq 1.3e-5 off at every step, some 30 times torch's own error
    worst = _worst_ratio("default", one_minus=_parent_complements)
    assert worst["v"] > 1.0 and worst["m"] <= 1.0, worst


def test_every_mutation_is_listed():
    assert set(CAUGHT_BY) == set(MUTATIONS) | {"parent_complements"}


def test_bf16_rounding_port_on_the_crafted_table():
    t = bf16_table()
    assert t.numel() == 71 and t.dtype == torch.int32
    f = t.view(torch.float32)
    got = torch.from_numpy(f32_to_bf16_np(t.numpy().view(np.uint32)).view(np.int16))
    want = f.to(torch.bfloat16).view(torch.int16)
    nan = torch.isnan(f)
    assert int(nan.sum()) == 4
    assert torch.equal(got[~nan], want[~nan])
    assert torch.isnan(got[nan].view(torch.bfloat16).float()).all()  # payloads differ; NaN stays NaN
    # the table holds what it says: ties both ways, overflow to inf, denormals to zero and up
    u = lambda x: x - (1 << 16) if x >= (1 << 15) else x  # noqa: E731
    pairs = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3F808001: 0x3F81, 0x3F817FFF: 0x3F81, 0x7F7FFFFF: 0x7F80,
             0xFF7FFFFF: 0xFF80, 0x7F7F7FFF: 0x7F7F, 0x80000000: 0x8000, 0x00008000: 0x0000, 0x00018000: 0x0002,
             0x007FFFFF: 0x0080}
    bits = [int(x) & 0xFFFFFFFF for x in t]
    for src, dst in pairs.items():
        assert int(got[bits.index(src)]) == u(dst), hex(src)


def test_optimizer_hooks_refuse_a_freed_handle(mesh_factory, monkeypatch):
    """A handle that is not a live allocation is refused by name before anything of it is read,
    as the list calls refuse it; a live one gets as far as the GPU check."""
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(2)
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        live = c.alloc(api.OCM_REMOTE_GPU, local_bytes=1 << 16, remote_bytes=1 << 16)
        gone = c.alloc(api.OCM_REMOTE_GPU, local_bytes=1 << 16, remote_bytes=1 << 16)
        stale = ctypes.c_void_p(gone.handle.value)
        gone.free()
        lib = api.load()
        hp, rows = (ctypes.c_float * 9)(), api.OcmAdamRows()
        buf = (ctypes.c_double * 8)()  # stands for every device pointer: no hook gets as far as reading one
        ptr = ctypes.cast(buf, ctypes.c_void_p)
        try:
            for handle, said in ((stale, "unknown allocation"), (live.handle, "needs a GPU")):
                calls = {
                    "ocm_x_adam": lambda: lib.ocm_x_adam(handle, ptr, ptr, 8, 0, 64, hp, None),
                    "ocm_x_acc_sumsq": lambda: lib.ocm_x_acc_sumsq(handle, 0, None, None, ptr, ptr, None, 0, None),
                    "ocm_x_adam_rows": lambda: lib.ocm_x_adam_rows(handle, handle, ctypes.byref(rows), None, None, hp, 1.0,
                                                                    None, None),
                }
                for name, call in calls.items():
                    assert call() == -1, name
                    assert api.last_error().endswith(said) and name in api.last_error(), (name, api.last_error())
            # either of two handles: the live one does not vouch for the stale one
            for table, state in ((live.handle, stale), (stale, live.handle)):
                assert lib.ocm_x_adam_rows(table, state, ctypes.byref(rows), None, None, hp, 1.0, None, None) == -1
                assert api.last_error().endswith("unknown allocation"), api.last_error()
        finally:
            live.free()
