"""The gradient-norm reduction over remote fp32 accumulators (acc_norm_kernel and its finishing
kernel, ocm_x_acc_sumsq) through Allocation.acc_sumsq, OffloadedGradAccumulator.sumsq / grad_norm
and OffloadedAdam.step(max_norm=..., skip_nonfinite=...).

The layout is test_gpu_adam.py's: offsets 16-byte but not 256-byte aligned, guard words (a NaN
with a payload) around every array, stripe-unit boundaries inside the arrays. A single over-read
into a guard word turns a sum into NaN and its count non-zero, so the guards need no check of
their own.

The oracle is math.fsum of the float64 squares: the square of an fp32 value is exact in fp64, so
that is the exact sum, and any order of fp64 additions of n non-negative terms is within
n * 2^-53 relative of it. That bound is asserted everywhere; nothing here is measured."""
import math
import os
import subprocess
import sys

import pytest
import torch

from oncilla_amd import api
from oncilla_amd.models import OffloadedAdam, OffloadedGradAccumulator
from quant_cases import read_remote, write_remote
from test_gpu_adam import DEV, SMALL, Layout, _alloc, _bits, _client, _multi_sizes, second_pass_length

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = sorted(set(SMALL + [64, 4099]))  # tail only; one vector; vector + tail; partly filled and more than one workgroup
assert SHORT == [1, 3, 4, 5, 64, 1023, 1027, 4099]
LONG_AMONG_TINY = 70003
EPS = 2.0 ** -53
SENTINEL = -12345


def exact_sumsq(t):
    """The exact sum of squares of an fp32 tensor, rounded once: each float64 square is exact."""
    return math.fsum((t.double().numpy() ** 2).tolist())


def values(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * 3.0


def load(a, lay, arrays):
    """Guards everywhere, tensor i's words at its 'g' offset; returns the image written."""
    img = lay.image()
    for i, t in enumerate(arrays):
        img[lay.words(i, "g")] = t.view(torch.int32)
    write_remote(a, 0, 0, img)
    return img


def sumsq_of(a, lay):
    s, b = a.acc_sumsq([d["g"] for d in lay.off], lay.sizes)
    torch.cuda.synchronize()
    assert s.dtype == torch.float64 and b.dtype == torch.int64 and s.is_cuda and b.is_cuda
    assert s.numel() == b.numel() == len(lay.sizes) + 1
    return s.cpu(), b.cpu()


def check_exact(what, s, b, arrays):
    """Every tensor and the total within n * 2^-53 of the exact sum (printed first; read with -s),
    every count 0."""
    exact = [exact_sumsq(t) for t in arrays]
    total, n_total = math.fsum(exact), sum(t.numel() for t in arrays)
    worst = 0.0
    for i, (t, e) in enumerate(zip(arrays, exact)):
        got = float(s[i])
        worst = max(worst, abs(got - e) / (t.numel() * EPS * e) if e else 0.0)
        assert abs(got - e) <= t.numel() * EPS * e, (what, i, t.numel(), got, e)
    print(f"acc-norm {what}: worst error / bound {worst:.3f}; total off by "
          f"{abs(float(s[-1]) - total) / (n_total * EPS * total):.3f} of its bound")
    assert abs(float(s[-1]) - total) <= n_total * EPS * total, (what, float(s[-1]), total)
    assert not b.any(), (what, b.tolist())


@pytest.mark.parametrize("state", ["hbm", "host", "striped"])
def test_against_the_exact_sum(mesh_factory, state):
    """One launch: the short lengths and one that reaches the second grid-stride pass of the
    variant in use (host: the buffer-resource kernel on the host grid) and ends on a 3-element
    tail. Then 37 tensors, one long among tiny ones, in two launches with the totals formed once.
    Each call is made twice, with identical bits in both outputs, and leaves the whole remote half
    bit for bit the image written."""
    big = second_pass_length(state == "host")
    assert big % 4 == 3
    lists = {"one launch": SHORT + [big], "two launches": _multi_sizes(LONG_AMONG_TINY)[0]}
    assert len(lists["one launch"]) <= 32 < len(lists["two launches"]) == 37
    with _client(mesh_factory, state) as c:
        a = _alloc(c, state, max(Layout(s, "g").nbytes for s in lists.values()))
        try:
            for what, sizes in lists.items():
                lay = Layout(sizes, "g")
                arrays = [values(n, 7 * n + i) for i, n in enumerate(sizes)]
                img = load(a, lay, arrays)
                s, b = sumsq_of(a, lay)
                check_exact(f"{what}/{state}", s, b, arrays)
                s2, b2 = sumsq_of(a, lay)  # reproducible: the order of additions is the launch shape's
                assert torch.equal(s.view(torch.int64), s2.view(torch.int64)) and torch.equal(b, b2), what
                after = read_remote(a, 0, 0, lay.nbytes).view(torch.int32)  # read-only
                assert torch.equal(after, img), f"{what}/{state}: word {int((after != img).nonzero()[0])} changed"
        finally:
            a.free()


def test_empty_lists(mesh_factory):
    """No tensors: zero totals. Empty tensors among others: +0 and 0 for them, wherever they point."""
    with _client(mesh_factory, "hbm") as c:
        lay = Layout([5, 64], "g")
        a = _alloc(c, "hbm", lay.nbytes)
        try:
            arrays = [values(5, 1), values(64, 2)]
            load(a, lay, arrays)
            s, b = a.acc_sumsq([], [])
            torch.cuda.synchronize()
            assert s.tolist() == [0.0] and b.tolist() == [0]
            s, b = a.acc_sumsq([0, lay.off[0]["g"], a.remote_size(), lay.off[1]["g"]], [0, 5, 0, 64])
            torch.cuda.synchronize()
            assert float(s[0]) == 0.0 and float(s[2]) == 0.0 and b.tolist() == [0] * 5
            check_exact("with empty tensors", s[[1, 3, 4]].cpu(), b[[1, 3, 4]].cpu(), arrays)
            s, b = a.acc_sumsq([0, 16], [0, 0])  # nothing to read: the finishing kernel alone
            torch.cuda.synchronize()
            assert s.tolist() == [0.0] * 3 and b.tolist() == [0] * 3
        finally:
            a.free()


@pytest.mark.parametrize("state", ["hbm", "host"])
def test_not_fp32_inside(mesh_factory, state):
    """Squares past FLT_MAX (1e19 and 1e30 values: an fp32 sum of squares is inf), and 4099 ones
    beside one 2^-10, whose square 2^-20 an fp32 sum of 4099 cannot hold (its ulp there is 2^-11).
    Both finite and within n * 2^-53 of the exact sum."""
    large = torch.tensor([1e19, 1e30] * 513 + [1e30], dtype=torch.float32)  # 1027 words
    ones = torch.ones(4100)
    ones[2049] = 2.0 ** -10
    assert exact_sumsq(ones) == 4099 + 2.0 ** -20 and math.isinf(float((large * large).sum()))
    assert float((ones * ones).sum()) == 4099.0
    with _client(mesh_factory, state) as c:
        lay = Layout([1027, 4100], "g")
        a = _alloc(c, state, lay.nbytes)
        try:
            load(a, lay, [large, ones])
            s, b = sumsq_of(a, lay)
            assert torch.isfinite(s).all()
            check_exact(f"wide/{state}", s, b, [large, ones])
        finally:
            a.free()


INF, NAN = math.inf, math.nan


def test_special_values(mesh_factory):
    """+-0 and 1e-40 count as finite; +-inf and NaN in the vector part and in the tail of separate
    tensors, HBM and host spaces: nonfinite exact per tensor and in the total, sumsq inf where only
    infinities occur and NaN where a NaN occurs, the other tensors of the launch unaffected."""
    def tensor(seed, at=(), tail=()):
        t = values(67, seed)  # 64 words of vectors, 3 of tail
        t[[1, 5, 9]] = torch.tensor([0.0, -0.0, 1e-40])
        for i, x in at:
            t[i] = x
        for i, x in enumerate(tail):
            t[64 + i] = x
        return t

    arrays = [tensor(0), tensor(1, at=[(13, INF), (40, -INF)]), tensor(2, at=[(17, NAN), (21, INF)]),
              tensor(3, tail=(1.0, INF, -0.0)), tensor(4, tail=(NAN, 1e-40, 2.0)), tensor(5, tail=(-INF, INF, 0.0)),
              tensor(6)]
    counts = [0, 2, 2, 1, 1, 2, 0]
    kinds = ["finite", "inf", "nan", "inf", "nan", "inf", "finite"]
    lay = Layout([67] * len(arrays), "g")
    with _client(mesh_factory, "hbm") as c:
        for state in ("hbm", "host"):
            a = _alloc(c, state, lay.nbytes)
            try:
                load(a, lay, arrays)
                s, b = sumsq_of(a, lay)
                assert b.tolist() == counts + [sum(counts)], (state, b.tolist())
                for i, kind in enumerate(kinds):
                    got = float(s[i])
                    if kind == "finite":
                        e = exact_sumsq(arrays[i])
                        assert abs(got - e) <= 67 * EPS * e, (state, i, got, e)
                    else:
                        assert (got == INF) if kind == "inf" else math.isnan(got), (state, i, got)
                assert math.isnan(float(s[-1])), state
            finally:
                a.free()


def test_runs_behind_an_async_accumulate(mesh_factory):
    """accumulate_batch(async_=True) and acc_sumsq at once, no host wait between: the sums are
    those of the accumulated values."""
    n = 1 << 18
    x = values(n, 99)
    with _client(mesh_factory, "hbm") as c:
        a = _alloc(c, "hbm", 4 * n + 4096)
        try:
            write_remote(a, 0, 0, torch.zeros(n + 1024, dtype=torch.float32))
            a.local_tensor(torch.float32)[:n].copy_(x)
            torch.cuda.synchronize()
            a.accumulate_batch([[0, 256, n]], dtype=torch.float32, scale=2.0, async_=True)
            s, b = a.acc_sumsq([256], [n])
            torch.cuda.synchronize()
            a.wait()
            check_exact("behind an accumulate", s.cpu(), b.cpu(), [2.0 * x])
        finally:
            a.free()


def test_refusals_change_nothing(mesh_factory):
    """A misaligned g_off, a last word past the end of the half, list lengths that do not match:
    OcmError each, and the sentinel-filled outputs are as they were after a synchronise. (The mesh
    fixture places every remote half of a GPU client where the GPU can address it, so the net-tier
    refusal is not run here.)"""
    sizes = [1027, 64, 5]
    with _client(mesh_factory, "hbm") as c:
        lay = Layout(sizes, "g")
        a = _alloc(c, "hbm", lay.nbytes)
        try:
            img = load(a, lay, [values(n, n) for n in sizes])
            offs, end = [d["g"] for d in lay.off], a.remote_size()
            assert (end - 4 * sizes[-1]) % 16 != 0
            s = torch.full((4,), float(SENTINEL), dtype=torch.float64, device=DEV)
            b = torch.full((4,), SENTINEL, dtype=torch.int64, device=DEV)
            work = torch.empty(int(c.lib.ocm_x_acc_sumsq_work_bytes(3)), dtype=torch.uint8, device=DEV)
            cases = {
                "misaligned": (offs[:2] + [offs[2] + 8], sizes, work),
                "range": (offs[:2] + [(end - 4 * sizes[-1]) // 16 * 16 + 16], sizes, work),  # its last word is past the end
                "lengths": (offs, sizes[:2], work),
                "short workspace": (offs, sizes, work[:-16]),
            }
            for what, (g_offs, ns, w) in cases.items():
                with pytest.raises(api.OcmError):
                    a._acc_sumsq_into(g_offs, ns, s, b, w)
                torch.cuda.synchronize()
                assert (s == SENTINEL).all() and (b == SENTINEL).all(), what
            with pytest.raises(api.OcmError):
                a.acc_sumsq(offs, sizes[:2])
            assert torch.equal(read_remote(a, 0, 0, lay.nbytes).view(torch.int32), img)
            a._acc_sumsq_into(offs, sizes, s, b, work)  # the same list, put right, runs
            torch.cuda.synchronize()
            assert not (s == SENTINEL).any() and b.tolist() == [0] * 4
        finally:
            a.free()


# ---- the workload ----

def _mlp(dtype):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(24, 50), torch.nn.GELU(), torch.nn.Linear(50, 3)).to(DEV, dtype)


class _Twin:
    """The small MLP of test_gpu_adam_acc.py with its optimizer and accumulator."""

    def __init__(self, c, dtype, readback=False):
        self.model = _mlp(dtype)
        self.params = list(self.model.parameters())
        self.opt = OffloadedAdam(self.params, c, lr=3e-3)
        self.acc = OffloadedGradAccumulator(self.params, c, readback=readback)

    def backward(self, x, y):
        self.acc.zero_grads()
        torch.nn.functional.mse_loss(self.model(x).float(), y).backward()

    def follow(self, other):
        """Take the other's micro-batch gradients instead of running a backward."""
        self.acc.zero_grads()
        for q, p in zip(self.params, other.params):
            q.grad.copy_(p.grad)

    def state(self):
        self.opt.synchronize()
        out = []
        for i, p in enumerate(self.params):
            m, v = self.opt.moments(i)
            out += [_bits(p.detach().cpu()), _bits(m), _bits(v)]
            if self.opt.bf16:
                out.append(_bits(self.opt.master(i)))
        return out

    def accumulators(self):
        self.acc.wait()
        return read_remote(self.acc.alloc, 0, 0, 4 * self.acc.total_elems).view(torch.int32)

    def close(self):
        self.acc.close()
        self.opt.close()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.state(), b.state()))


@pytest.mark.parametrize("bf16", [False, True])
def test_training_step_clips_in_place(mesh_factory, bf16):
    """accum = 4, three steps. max_norm = 1e9 never clips: parameters, moments and masters are bit
    for bit those of a twin stepping with no max_norm. max_norm = 1e-3 always clips: the returned
    norm is within n * 2^-53 relative of the float64 norm of a readback=True twin's read() and
    within n * 2^-24 of what torch's clip_grad_norm_ returns on those values (the worst case of its
    fp32 sum of n non-negative terms; n the parameter count); parameters and state are bit for bit
    those of that twin stepping with scale = api.clip_scale(...) made from the returned norm
    (sqrt(fl(x * x)) == x in binary floating point, so the norm gives the sum of squares' root back);
    every accumulator is +0 at the end."""
    dtype = torch.bfloat16 if bf16 else torch.float32
    accum, steps = 4, 3
    m = mesh_factory(4, gpus=[0] * 4, policy="stripe")
    with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
        loose, plain, tight = _Twin(c, dtype), _Twin(c, dtype), _Twin(c, dtype)
        scaled = _Twin(c, dtype, readback=True)
        n = sum(p.numel() for p in tight.params)
        gen = torch.Generator().manual_seed(1)
        for _ in range(steps):
            for _ in range(accum):
                x = torch.randn(32, 24, generator=gen).to(DEV, dtype)
                y = torch.randn(32, 3, generator=gen).to(DEV)
                loose.backward(x, y)
                plain.follow(loose)
                tight.backward(x, y)
                scaled.follow(tight)
                for t in (loose, plain, tight, scaled):
                    t.acc.add(scale=1.0 / accum)
            assert loose.opt.step(accumulator=loose.acc, max_norm=1e9) > 0.0
            assert plain.opt.step(accumulator=plain.acc) is None
            sums = [g.detach().cpu().clone() for g in scaled.acc.read()]
            want = math.sqrt(math.fsum(exact_sumsq(g.reshape(-1)) for g in sums))
            shadow = [torch.nn.Parameter(torch.zeros_like(g)) for g in sums]
            for q, g in zip(shadow, sums):
                q.grad = g.clone()
            theirs = float(torch.nn.utils.clip_grad_norm_(shadow, 1e-3))
            norm = tight.opt.step(accumulator=tight.acc, max_norm=1e-3)
            print(f"acc-norm workload {dtype}: norm {norm!r}, float64 {want!r} (off by {abs(norm - want) / want:.2e}), "
                  f"torch {theirs!r} (off by {abs(norm - theirs) / theirs:.2e})")
            assert isinstance(norm, float) and norm > 1e-3
            assert abs(norm - want) <= n * EPS * want
            assert abs(norm - theirs) <= n * 2.0 ** -24 * theirs
            assert scaled.acc.grad_norm() == (norm, 0)  # readback either way: the same pass, the same bits
            scaled.opt.step(accumulator=scaled.acc, scale=api.clip_scale(norm * norm, 1.0, 1e-3))
        assert loose.opt.t == plain.opt.t == tight.opt.t == scaled.opt.t == steps
        assert _same(loose, plain), "max_norm = 1e9 changed the step"
        assert _same(tight, scaled), "max_norm = 1e-3 is not the step with clip_scale's scale"
        assert not _same(tight, loose)
        assert not tight.accumulators().any() and not loose.accumulators().any()
        for t in (loose, plain, tight, scaled):
            t.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_nonfinite_step_is_skipped(mesh_factory, bf16):
    """One inf reaches one accumulator word (through the last micro-batch's gradient):
    step(skip_nonfinite=True) returns a non-finite norm, t, parameters, moments and masters are
    unchanged bit for bit and every accumulator is +0. The next step, on clean gradients, matches a
    twin that never saw the bad one."""
    dtype = torch.bfloat16 if bf16 else torch.float32
    accum = 4
    m = mesh_factory(4, gpus=[0] * 4, policy="stripe")
    with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
        mine, twin = _Twin(c, dtype), _Twin(c, dtype)
        gen = torch.Generator().manual_seed(2)

        def micro_batches(poison=False):
            for k in range(accum):
                x = torch.randn(32, 24, generator=gen).to(DEV, dtype)
                y = torch.randn(32, 3, generator=gen).to(DEV)
                mine.backward(x, y)
                if not poison:
                    twin.follow(mine)
                    twin.acc.add(scale=1.0 / accum)
                elif k == accum - 1:
                    mine.params[1].grad.view(-1)[7] = INF
                mine.acc.add(scale=1.0 / accum)

        micro_batches()
        norm = mine.opt.step(accumulator=mine.acc, skip_nonfinite=True)
        assert math.isfinite(norm) and norm > 0.0 and twin.opt.step(accumulator=twin.acc) is None
        before = mine.state()
        micro_batches(poison=True)
        assert mine.acc.grad_norm()[1] == 1
        norm = mine.opt.step(accumulator=mine.acc, skip_nonfinite=True, max_norm=1.0)
        assert isinstance(norm, float) and not math.isfinite(norm)
        assert mine.opt.t == 1 and all(torch.equal(x, y) for x, y in zip(before, mine.state()))
        assert not mine.accumulators().any()
        micro_batches()
        assert math.isfinite(mine.opt.step(accumulator=mine.acc, skip_nonfinite=True))
        twin.opt.step(accumulator=twin.acc)
        assert mine.opt.t == twin.opt.t == 2 and _same(mine, twin)
        for t in (mine, twin):
            t.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_train_offload_example_clips(native, bf16):
    env = {k: v for k, v in os.environ.items() if k != "OCM_NO_GPU"}
    args = [sys.executable, os.path.join(REPO, "examples", "train_offload.py"), "--gpu", "0", "--steps", "60",
            "--accum", "4", "--accum-in-place", "--clip-norm", "1.0"] + (["--bf16"] if bf16 else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd="/tmp", env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]  # the example exits non-zero unless its loss halves
    assert "mode=fused" in r.stdout and "60 steps" in r.stdout
    assert "clip-norm 1: last gradient norm" in r.stdout and "of 60 steps clipped" in r.stdout
