"""Cases shared by the accumulate tests (test_acc_cpu.py, test_gpu_acc.py): the edge
vectors, the 60-op list and the gradient-accumulator exercise. Every comparison is bit
for bit (int32 views) with the torch oracle (oncilla_amd.ops.accumulate_reference);
elements whose oracle result is NaN are checked for NaN-ness only."""
import random

import numpy as np
import torch

from oncilla_amd import api
from oncilla_amd.ops import accumulate_reference
from quant_cases import read_local, read_remote, write_local, write_remote

UNIT = 4096  # stripe unit of every pool here
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
EDGE_ELEMS = 64
FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")


def assert_bits(got, want, what=""):
    """fp32 tensors equal bit for bit; where the oracle gives NaN, some NaN."""
    got, want = got.reshape(-1), want.reshape(-1)
    nan = torch.isnan(want)
    assert torch.isnan(got[nan]).all(), (what, "NaN expected")
    g, w = got[~nan].view(torch.int32), want[~nan].view(torch.int32)
    if not torch.equal(g, w):
        i = int((g != w).nonzero()[0])
        raise AssertionError(f"{what}: element {i}: 0x{int(g[i]) & 0xffffffff:08x}, expected 0x{int(w[i]) & 0xffffffff:08x}")


def _vec(dtype, head, seed):
    """64 elements of `dtype`: `head`, then seeded finite filler over a few binades."""
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(EDGE_ELEMS, generator=g) * torch.exp(torch.empty(EDGE_ELEMS).uniform_(-4.0, 4.0, generator=g))).to(dtype)
    t[: len(head)] = torch.tensor(head, dtype=torch.float64).to(dtype)
    return t


def _bits16(dtype, words):
    return torch.tensor([w - 0x10000 if w >= 0x8000 else w for w in words], dtype=torch.int16).view(dtype)


def edge_vectors(dtype):
    """name -> (acc fp32 [64], x `dtype` [64], scale): one op each."""
    f32, sig = torch.float32, {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}[dtype]
    v = {}
    v["signed_zeros"] = (_vec(f32, [0.0, -0.0, 0.0, -0.0], 1), _vec(dtype, [0.0, -0.0, -0.0, 0.0], 2), 1.0)
    v["signed_zeros_negative_scale"] = (_vec(f32, [0.0, -0.0, 0.0, -0.0], 3), _vec(dtype, [0.0, -0.0, -0.0, 0.0], 4), -1.0)
    # 2^-140 + 2^-141, the second as scale * x where the type cannot hold it
    if dtype == torch.float32:
        x, s = [2.0 ** -141, -(2.0 ** -141), 2.0 ** -149], 1.0
    elif dtype == torch.bfloat16:
        x, s = [2.0 ** -100, -(2.0 ** -100), 2.0 ** -108], 2.0 ** -41
    else:
        x, s = [2.0 ** -14, -(2.0 ** -14), 2.0 ** -22], 2.0 ** -127
    v["subnormal_f32_sum"] = (_vec(f32, [2.0 ** -140, 2.0 ** -140, 2.0 ** -140], 5), _vec(dtype, x, 6), s)
    # subnormal elements of the type itself: the smallest, the largest, a negative one
    xs = _vec(dtype, [], 7)
    if dtype == torch.float32:
        xs[:3] = torch.tensor([1, 0x007FFFFF, 0x80000400 - (1 << 32)], dtype=torch.int32).view(f32)
    elif dtype == torch.bfloat16:
        xs[:3] = _bits16(dtype, [0x0001, 0x007F, 0x8013])
    else:
        xs[:3] = _bits16(dtype, [0x0001, 0x03FF, 0x8213])
    v["subnormal_x"] = (_vec(f32, [0.0, float(xs[1]), 2.0 ** -126], 8), xs, 1.0)
    # scale = 1/3: the product itself rounds
    v["rounded_product"] = (_vec(f32, [1.0, 1.0, -2.0, 0.0], 9), _vec(dtype, [1.0, 3.0, 7.0, -5.0], 10), 1.0 / 3.0)
    # (1 + 2^-a)(1 + 2^-b) with a + b = 24 is 1 + 2^-a + 2^-b + 2^-24: the last term is half an
    # ulp, a tie that rounds to even, away; an fma keeps it. fp32: x = scale = 1 + 2^-12.
    a = {24: 12, 8: 7, 11: 10}[sig]
    xt, st = 1.0 + 2.0 ** -a, 1.0 + 2.0 ** -(24 - a)
    acc_t = -(1.0 + 2.0 ** -a + 2.0 ** -(24 - a))  # fp32: -(1 + 2^-11)
    v["fusion_telltale"] = (_vec(f32, [acc_t, -acc_t], 11), _vec(dtype, [xt, -xt], 12), st)
    acc, x, _ = v["fusion_telltale"]
    two = accumulate_reference(acc, x, st)
    fused = (acc.double() + x.double() * float(np.float32(st))).to(f32)  # one rounding
    assert float(two[0]) == 0.0 and float(fused[0]) == 2.0 ** -24, (two[0], fused[0])
    assert two[0].view(torch.int32) != fused[0].view(torch.int32)
    v["absorbed"] = (_vec(f32, [2.0 ** 24, 2.0 ** 24, -(2.0 ** 24)], 13), _vec(dtype, [1.0, 2.0, -1.0], 14), 1.0)
    v["cancellation"] = (_vec(f32, [1.5, -1.5, 0.375], 15), _vec(dtype, [-1.5, 1.5, -0.375], 16), 1.0)
    v["infinities"] = (_vec(f32, [INF, INF, -INF, 1.0, -INF], 17), _vec(dtype, [1.0, -INF, -INF, INF, INF], 18), 1.0)
    big = float(torch.finfo(dtype).max)
    v["largest_finite"] = (_vec(f32, [FLT_MAX, -FLT_MAX, FLT_MAX, big, -big], 19), _vec(dtype, [big, big, -big, big, big], 20), 1.0)
    for name, (acc, x, s) in v.items():
        assert acc.dtype == f32 and x.dtype == dtype and acc.numel() == x.numel() == EDGE_ELEMS, name
    return v


def run_edge_vectors(a, dtype, stage):
    """Every edge vector as one op on `a`: x at local 0, accumulators at a remote offset whose
    vectors cross a stripe-unit boundary. `stage`: local offset for raw reads and writes."""
    esize = torch.empty((), dtype=dtype).element_size()
    for k, (name, (acc, x, scale)) in enumerate(edge_vectors(dtype).items()):
        roff = UNIT - 32 + 4 * EDGE_ELEMS * k
        write_local(a, 0, x)
        write_remote(a, stage, roff, acc)
        a.accumulate_batch(np.array([[0, roff, EDGE_ELEMS]]), dtype, scale)
        got = read_remote(a, stage, roff, 4 * EDGE_ELEMS).view(torch.float32)
        assert_bits(got, accumulate_reference(acc, x, scale), f"{name} {dtype}")
        assert torch.equal(read_local(a, 0, esize * EDGE_ELEMS), x.view(torch.uint8)), name


def random_elems(n, dtype, seed):
    """n finite elements over some sixteen binades, zeros among them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp(torch.empty(n).uniform_(-6.0, 6.0, generator=g))
    x[::97] = 0.0
    return x.clamp(-60000.0, 60000.0).to(dtype)


SCALES = [1.0, -0.5, 1.0 / 3.0, 3.0, 2.0 ** -20, 0.1]
GUARD = 0xA5


class AccList:
    """60 ops on disjoint remote ranges (more ops than travel in the kernel arguments), dtypes
    and scales mixed per op, 4 to 4100 elements each, 16 to 48 guard bytes between the ranges.
    Op 0 starts at UNIT - 32 (its vectors cross a stripe-unit boundary) and op 1 ends exactly
    on one."""

    def __init__(self, seed=23):
        rng = random.Random(seed)
        sizes = [60, 1028, 4, 8, 1020, 1024, 2048, 4096 + 4] + [4 * rng.randint(1, 1024) for _ in range(52)]
        self.ops = []  # (local_offset, remote_offset, elems, torch dtype, scale)
        loff, roff = 0, 16
        for i, n in enumerate(sizes):
            dtype = DTYPES[i % 3] if i < 8 else rng.choice(DTYPES)
            scale = SCALES[i % len(SCALES)]
            if i == 0:
                roff = UNIT - 32
            elif i == 1:
                roff = (roff + 4 * n + UNIT - 1) // UNIT * UNIT - 4 * n
            self.ops.append((loff, roff, n, dtype, scale))
            loff += (n * torch.empty((), dtype=dtype).element_size() + 15) // 16 * 16
            roff += 4 * n + 16 * rng.randint(1, 3)
        assert len(self.ops) == 60 and self.ops[0][1] == UNIT - 32 and (self.ops[1][1] + 4 * self.ops[1][2]) % UNIT == 0
        assert all(r0 + 4 * n0 + 16 <= r1 for (_, r0, n0, _, _), (_, r1, _, _, _) in zip(self.ops, self.ops[1:]))
        self.elems = sum(o[2] for o in self.ops)
        self.remote_bytes = (roff + UNIT - 1) // UNIT * UNIT
        self.stage = (loff + 63) // 64 * 64  # local staging for raw reads and writes of the whole remote half
        self.local_bytes = self.stage + self.remote_bytes

    def array(self):
        return np.array([[lo, ro, n, api.acc_dtype(dt), s] for lo, ro, n, dt, s in self.ops], dtype=np.float64)

    def run(self, a, async_=False, after=None):
        """Prepare, run the list on `a`, and compare the WHOLE remote half with a model, guards
        included; the local half must be unchanged."""
        model = torch.full((self.remote_bytes,), GUARD, dtype=torch.uint8)
        want = model.clone()
        for i, (lo, ro, n, dt, s) in enumerate(self.ops):
            x = random_elems(n, dt, seed=2000 + i)
            acc = random_elems(n, torch.float32, seed=3000 + i)
            write_local(a, lo, x)
            model[ro:ro + 4 * n] = acc.view(torch.uint8)
            r = accumulate_reference(acc, x, s)
            assert not torch.isnan(r).any()
            want[ro:ro + 4 * n] = r.view(torch.uint8)
        write_remote(a, self.stage, 0, model)
        local_before = read_local(a, 0, self.stage)
        a.accumulate_batch(self.array(), async_=async_)
        if after:
            after()
        elif async_:
            a.wait()
        got = read_remote(a, self.stage, 0, self.remote_bytes)
        if not torch.equal(got, want):
            bad = int((got != want).nonzero()[0])
            op = [i for i, (_, ro, n, _, _) in enumerate(self.ops) if ro <= bad < ro + 4 * n]
            raise AssertionError(f"remote byte {bad} differs (op {op or 'none: a guard byte'})")
        assert torch.equal(read_local(a, 0, self.stage), local_before), "the local half changed"


def exercise_grad_accumulator(acc, params, grads, scales):
    """`grads[m][k]`: micro-batch m's gradient of parameter k, written into the installed .grad
    views; after every add the oracle is replayed on the CPU. Returns nothing; asserts."""
    want = [torch.zeros(p.shape, dtype=torch.float32) for p in params]
    for m, scale in enumerate(scales):
        acc.zero_grads()
        for p, g in zip(params, grads[m]):
            p.grad.copy_(g.to(p.device))
        n = acc.add(scale=scale, async_=bool(m % 2))
        assert n == 1 + sum(p.dtype != q.dtype for p, q in zip(params, params[1:]))  # one op per run of a dtype
        want = [accumulate_reference(w, g, scale) for w, g in zip(want, grads[m])]
    got = acc.read()
    assert len(got) == len(params)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.float32 and g.shape == params[k].shape
        assert_bits(g.cpu(), w, f"parameter {k}")
    acc.zero()
    for g in acc.read():
        assert not g.cpu().view(torch.int32).any()
