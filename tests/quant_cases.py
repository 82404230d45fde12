"""Cases shared by the converting-transfer tests (test_quant_cpu.py, test_gpu_quant.py):
the edge groups, the 60-op list, and helpers that move raw bytes through an allocation.
Everything is compared byte for byte with the torch oracle (oncilla_amd.ops.quant)."""
import random

import numpy as np
import torch

from oncilla_amd import api
from oncilla_amd.ops import mx8_decode_reference, mx8_encode_reference, mx8_record_reference

UNIT = 4096  # stripe unit of every pool here


def _bits(dtype, words):
    """A 32-element group from 16-bit patterns (the rest +0)."""
    t = torch.zeros(32, dtype=torch.int16)
    for i, w in enumerate(words):
        t[i] = w - 0x10000 if w >= 0x8000 else w
    return t.view(dtype)


def _vals(dtype, vals):
    t = torch.zeros(32, dtype=dtype)
    for i, v in enumerate(vals):
        t[i] = v
    return t


def edge_groups(dtype):
    """name -> one group of 32 elements of `dtype`."""
    g = {}
    g["zero_with_neg_zero"] = _bits(dtype, [0, 0x8000, 0, 0x8000])
    m875 = torch.tensor(3.5, dtype=dtype)  # 0.875 * 2^2: m == 0.875 exactly
    g["m_0875"] = _vals(dtype, [3.5, 1.0, -0.5, 3.25, -3.5])
    nxt = (m875.view(torch.int16) + 1).view(dtype)  # the next representable value above it
    assert float(nxt) > 3.5
    g["m_0875_next"] = _vals(dtype, [float(nxt), 1.0, -0.5, 3.25, -3.5])
    # amax 448 (e = 0): the small members land in fp8 subnormals (multiples of 2^-9), ties included
    g["fp8_subnormals"] = _vals(dtype, [448.0, 2.0 ** -9, 3 * 2.0 ** -9, -(2.0 ** -10), 1.5 * 2.0 ** -10, 2.0 ** -11,
                                        7.5 * 2.0 ** -9, -7 * 2.0 ** -9, 2.0 ** -6, 5.5 * 2.0 ** -9])
    # ties where e4m3fn steps by 2 ([16, 32)), by 4 ([32, 64)) and by 32 ([256, 448])
    g["rne_ties"] = _vals(dtype, [448.0, 17.0, 19.0, 21.0, -17.0, 23.0, 34.0, 38.0, -42.0, 272.0, 304.0, -432.0, 1.0625, 1.1875])
    if dtype == torch.bfloat16:
        g["smallest_subnormal_amax"] = _bits(dtype, [0x0001, 0x8001, 0])  # e = -141, clamped to -127
        g["subnormal_mixed"] = _bits(dtype, [0x007f, 0x8040, 0x0001, 0x0013])
        g["largest"] = _bits(dtype, [0x7f7f, 0xff7f, 0x7f00, 0x4000])  # decodes past bf16's range: infinity
    else:
        g["smallest_subnormal_amax"] = _bits(dtype, [0x0001, 0x8001, 0])
        g["subnormal_mixed"] = _bits(dtype, [0x03ff, 0x8200, 0x0001, 0x0013])
        g["largest"] = _bits(dtype, [0x7bff, 0xfbff, 0x63d0, 0x4000])
    return g


def random_elems(n, dtype, seed):
    """n finite elements over some sixteen binades."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp(torch.empty(n).uniform_(-6.0, 6.0, generator=g))
    x[::97] = 0.0
    return x.clamp(-60000.0, 60000.0).to(dtype)


def roundtrip(x):
    """Oracle decode of the oracle encode, in x's shape."""
    c, s = mx8_encode_reference(x)
    return mx8_decode_reference(c, s, x.dtype).view(x.shape)


# ---- raw bytes through an allocation ----

def _sync(t):
    if t.is_cuda:
        torch.cuda.synchronize()


def write_local(a, off, t):
    lt = a.local_tensor(torch.uint8)
    b = t.contiguous().view(torch.uint8).reshape(-1)
    lt[off:off + b.numel()].copy_(b)
    _sync(lt)


def read_local(a, off, n):
    lt = a.local_tensor(torch.uint8)
    _sync(lt)
    return lt[off:off + n].cpu().clone()


def write_remote(a, stage, roff, t):
    """Raw bytes into the remote half with a plain put, staged at local offset `stage`."""
    write_local(a, stage, t)
    a.put(stage, roff, t.numel() * t.element_size())


def read_remote(a, stage, roff, n):
    a.get(stage, roff, n)
    return read_local(a, stage, n)


# ---- the 60-op list ----

class OpList:
    """60 mixed puts and gets on disjoint ranges, 32 to 4096 elements each (more ops than
    travel in the kernel arguments). Record 0's codes cross a stripe-unit boundary
    (remote_offset = 4096 * 2 - 64, 128 elements), record 1's scale bytes do (2048 elements
    whose 64 scale bytes start 32 bytes before a boundary), record 2 is a whole multi-tile op."""

    def __init__(self, seed=11):
        rng = random.Random(seed)
        sizes = [128, 2048, 4096] + [32 * rng.randint(1, 128) for _ in range(57)]
        sizes[3], sizes[4] = 32, 2048 + 32
        fixed = {0: UNIT * 2 - 64, 1: UNIT * 5 - 2080}
        self.ops = []  # (op_flag, local_offset, remote_offset, elems)
        loff, roff = 0, UNIT * 8
        for i, n in enumerate(sizes):
            flag = 1 if i in (0, 1) else (i % 3 != 0)  # gets: every third op
            if i in fixed:
                r = fixed[i]
            else:
                r, roff = roff, (roff + n + n // 32 + 31) // 32 * 32 + 32 * rng.randint(0, 3)
            self.ops.append((int(flag), loff, r, n))
            loff += 2 * n
        self.stage = (loff + 63) // 64 * 64     # local staging for raw reads and writes
        self.local_bytes = self.stage + 8192
        self.remote_bytes = (roff + UNIT) // UNIT * UNIT
        assert (fixed[1] + 2048) % UNIT == UNIT - 32
        assert len(self.ops) == 60

    def array(self):
        return np.asarray(self.ops, dtype=np.int64)

    def run(self, a, dtype, async_=False, after=None):
        """Prepare, run the list on `a`, and compare every record and every decoded range."""
        src = {}
        for i, (flag, lo, ro, n) in enumerate(self.ops):
            x = random_elems(n, dtype, seed=1000 + i)
            src[i] = x
            if flag:
                write_local(a, lo, x)
            else:
                write_remote(a, self.stage, ro, mx8_record_reference(x))
                write_local(a, lo, torch.full((n,), 0x5a5a, dtype=torch.int16))
        a.quant_batch(self.array(), dtype, async_=async_)
        if after:
            after()
        elif async_:
            a.wait()
        for i, (flag, lo, ro, n) in enumerate(self.ops):
            if flag:
                got = read_remote(a, self.stage, ro, api.quant_bytes(n))
                assert torch.equal(got, mx8_record_reference(src[i])), f"record of op {i} {self.ops[i]}"
            else:
                got = read_local(a, lo, 2 * n).view(dtype)
                want = roundtrip(src[i])
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"decoded op {i} {self.ops[i]}"


def exercise_kv(kv, rounds, seed, device):
    """The swap pattern of test_kv_offload.py on a compressed pool: what comes back is the
    oracle decode of the oracle encode of the block that was written."""
    rng = random.Random(seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    pool_model = {}
    for r in range(rounds):
        fresh = torch.randn((kv.num_gpu_blocks, *kv.block_shape), generator=g).to(kv.dtype)
        kv.gpu_cache.copy_(fresh.to(device))  # written by torch on its stream; swap_out must see it
        k = rng.randint(1, kv.num_gpu_blocks)
        gpu_ids = rng.sample(range(kv.num_gpu_blocks), k)
        pool_ids = rng.sample(range(kv.num_pool_blocks), k)
        if r % 2 == 0:  # consecutive runs: still one op per block
            base = rng.randrange(0, kv.num_pool_blocks - k + 1)
            pool_ids = list(range(base, base + k))
            gpu_ids = sorted(gpu_ids)
        assert kv.swap_out(list(zip(gpu_ids, pool_ids)), async_=bool(r % 3)) == k
        for gi, pi in zip(gpu_ids, pool_ids):
            pool_model[pi] = roundtrip(fresh[gi]).to(device)
        kv.gpu_cache.zero_()
        known = list(pool_model)
        back = rng.sample(known, min(len(known), kv.num_gpu_blocks))
        dst = rng.sample(range(kv.num_gpu_blocks), len(back))
        kv.swap_in(list(zip(back, dst)), async_=bool(r % 2))
        # torch reads on its stream right away: swap_in made it wait for the copies
        for pi, gi in zip(back, dst):
            assert torch.equal(kv.gpu_cache[gi].view(torch.int16), pool_model[pi].view(torch.int16)), (r, pi, gi)
    kv.wait()
