"""Cases shared by the MXFP4 tests (test_mx4_cpu.py, test_gpu_mx4.py): the edge groups, the
all-patterns sweep, the decode table, the mixed-format list and a strided layout. Everything is compared byte
for byte with the torch oracle (oncilla_amd.ops.mx4_*_reference). The byte movers are those
of quant_cases.py."""
import functools
import random

import numpy as np
import torch

from oncilla_amd import api
from oncilla_amd.ops import (mx4_decode_reference, mx4_encode_reference, mx4_record_reference, mx4_rows_reference,
                             mx8_record_reference)
from quant_cases import (UNIT, DecodeTable, _bits, _vals, all_patterns, random_elems, read_local, read_remote, write_local,
                         write_remote)
from quant_cases import roundtrip as roundtrip8

DTYPES = [torch.bfloat16, torch.float16]
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]  # the RNE ties of E2M1 after scaling


def _next_up(v, dtype):
    return float((torch.tensor(v, dtype=dtype).view(torch.int16) + 1).view(dtype))


def edge_groups(dtype):
    """name -> one group of 32 elements of `dtype`."""
    g = {}
    g["zero_with_neg_zero"] = _bits(dtype, [0, 0x8000, 0, 0x8000])
    # m == 0.75 exactly: 6 = 0.75 * 2^3 and 3 = 0.75 * 2^2; and the next representable value above each
    g["m_075_six"] = _vals(dtype, [6.0, 1.0, -0.5, 3.0, -6.0, 4.5, 2.25])
    g["m_075_three"] = _vals(dtype, [3.0, 1.0, -0.5, 0.375, -3.0, 2.25, 0.125])
    for name, v in (("m_075_six_next", 6.0), ("m_075_three_next", 3.0)):
        nxt = _next_up(v, dtype)
        assert nxt > v
        g[name] = _vals(dtype, [nxt, 1.0, -0.5, v, -v, 0.75 * v, 0.125])
    # every tie after scaling, both signs, in a group whose amax is 6 (e = 0) and in one scaled by 2^5
    g["rne_ties"] = _vals(dtype, [6.0] + TIES + [-t for t in TIES])
    g["rne_ties_scaled"] = _vals(dtype, [6.0 * 32] + [32 * t for t in TIES] + [-32 * t for t in TIES])
    # around the ties at 0.25 (to 0) and 0.75 (to 1): values that round to 0, keeping their sign, and to 0.5
    lo, hi = torch.tensor(0.25, dtype=dtype), torch.tensor(0.75, dtype=dtype)
    below = lambda t: float((t.view(torch.int16) - 1).view(dtype))  # noqa: E731
    g["to_zero_and_half"] = _vals(dtype, [6.0, 0.125, -0.125, below(lo), _next_up(0.25, dtype), 0.5, below(hi),
                                          _next_up(0.75, dtype), -below(lo), -_next_up(0.25, dtype), -below(hi), 2.0 ** -20])
    g["smallest_subnormal_amax"] = _bits(dtype, [0x0001, 0x8001, 0])  # bf16: e = -135 clamps to -127
    if dtype == torch.bfloat16:
        g["subnormal_mixed"] = _bits(dtype, [0x007f, 0x8040, 0x0001, 0x0013, 0x0060])
        g["largest"] = _bits(dtype, [0x7f7f, 0xff7f, 0x7f00, 0x7e80, 0x4000])  # decodes past bf16's range: infinity
    else:
        g["subnormal_mixed"] = _bits(dtype, [0x03ff, 0x8200, 0x0001, 0x0013, 0x0300])
        g["largest"] = _bits(dtype, [0x7bff, 0xfbff, 0x7800, 0x7400, 0x63d0, 0x4000])
    return g


@functools.lru_cache(maxsize=None)
def sweep(dtype):
    """Every finite 16-bit pattern of `dtype`, twice, 4096 groups: once in pattern order (a group
    holds 32 neighbouring values: codes near the top of the range) and once dealt out 2048 apart
    (a group spans every binade and both signs: most of it rounds to zero). Inf and NaN patterns
    are replaced by zero. Returns (elements, record, decoded) with the oracle's results, computed
    once per dtype and shared: treat them as read-only."""
    x = all_patterns(dtype)
    codes, scales = mx4_encode_reference(x)
    return x, torch.cat([codes, scales]), mx4_decode_reference(codes, scales, dtype)


@functools.lru_cache(maxsize=None)
def decode_table():
    """65280 code bytes, byte[i] = i & 255, under 4080 scale bytes, scale[g] = g // 16: every code
    byte (both nibbles, every pairing) meets every scale byte 0..254, 130560 elements. Scale
    byte 255 is E8M0's NaN: no encoder writes it and its decode is not specified."""
    codes = (torch.arange(255 * 256, dtype=torch.int32) & 255).to(torch.uint8)
    scales = (torch.arange(255 * 16, dtype=torch.int32) // 16).to(torch.uint8)
    assert int(scales.max()) == 254 and int(torch.bincount(scales.long()).min()) == 16
    return DecodeTable("mxfp4", codes, scales, mx4_decode_reference)


TABLE_ROWS = 30  # the table as rows of 4352 elements: two tiles and eight groups each


def roundtrip(x):
    """Oracle decode of the oracle encode, in x's shape."""
    c, s = mx4_encode_reference(x)
    return mx4_decode_reference(c, s, x.dtype).view(x.shape)


def up32(n):
    return (n + 31) // 32 * 32


FORMATS = {"mxfp8": (mx8_record_reference, roundtrip8), "mxfp4": (mx4_record_reference, roundtrip)}


class MixedList:
    """60 ops on disjoint ranges: puts and gets, MXFP8 and MXFP4, 32 to 4096 elements each, two
    empty ops among them (more ops than travel in the kernel arguments). Op 0's MXFP4 codes cross
    a stripe-unit boundary and op 1's scale bytes start 32 bytes before one."""

    def __init__(self, seed=17):
        rng = random.Random(seed)
        sizes = [256, 4096, 4096 + 32, 32, 2048 + 32] + [32 * rng.randint(1, 128) for _ in range(55)]
        sizes[7] = sizes[30] = 0
        fixed = {0: UNIT * 2 - 64, 1: UNIT * 5 - 2080}  # op 1: 2048 code bytes, then 128 scale bytes from UNIT * 5 - 32
        self.ops, self.formats = [], []
        loff, roff = 0, UNIT * 8
        for i, n in enumerate(sizes):
            fmt = "mxfp4" if i < 3 or i % 2 else "mxfp8"
            flag = 1 if i < 2 else int(i % 3 != 0)
            if i in fixed:
                r = fixed[i]
            else:
                r, roff = roff, up32(roff + api.quant_bytes(n, fmt)) + 32 * rng.randint(0, 3)
            self.ops.append((flag, loff, r, n))
            self.formats.append(fmt)
            loff += 2 * n
        self.stage = (loff + 63) // 64 * 64
        self.local_bytes = self.stage + 8192
        self.remote_bytes = (roff + UNIT) // UNIT * UNIT
        assert len(self.ops) == 60 and {(o[0], f) for o, f in zip(self.ops, self.formats)} == {
            (0, "mxfp8"), (1, "mxfp8"), (0, "mxfp4"), (1, "mxfp4")}

    def wire_bytes(self):
        return sum(api.quant_bytes(o[3], f) for o, f in zip(self.ops, self.formats))

    def run(self, a, dtype, async_=False):
        src = {}
        for i, ((flag, lo, ro, n), fmt) in enumerate(zip(self.ops, self.formats)):
            if not n:
                continue
            src[i] = x = random_elems(n, dtype, seed=2000 + i)
            if flag:
                write_local(a, lo, x)
            else:
                write_remote(a, self.stage, ro, FORMATS[fmt][0](x))
                write_local(a, lo, torch.full((n,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(api.quant_ops(np.asarray(self.ops, dtype=np.int64), dtype, self.formats), async_=async_)
        if async_:
            a.wait()
        for i, ((flag, lo, ro, n), fmt) in enumerate(zip(self.ops, self.formats)):
            if not n:
                continue
            record, back = FORMATS[fmt]
            if flag:
                got = read_remote(a, self.stage, ro, api.quant_bytes(n, fmt))
                assert torch.equal(got, record(src[i])), f"record of op {i} {self.ops[i]} {fmt}"
            else:
                got = read_local(a, lo, 2 * n).view(torch.int16)
                assert torch.equal(got, back(src[i]).view(torch.int16)), f"decoded op {i} {self.ops[i]} {fmt}"


def run_strided(a, dtype, rows, row_elems, extra_stride, seed, base=UNIT - 32):
    """One strided MXFP4 put of `rows` rows into a remote half filled with 0xA5, every byte of the
    touched range checked (records, and the fill between and behind them); a plain MXFP4 get of
    the last row; then a strided get of all rows into a local range filled with 0x5A, the gaps
    between the rows checked too. Needs local_bytes >= 2 * rows * local stride + the staging
    behind it and remote_bytes >= base + rows * remote stride."""
    rec = api.quant_bytes(row_elems, "mxfp4")
    rs, ls = up32(rec) + extra_stride, 2 * row_elems + 16
    x = random_elems(rows * row_elems, dtype, seed).view(rows, row_elems)
    span_l, span_r = rows * ls, rows * rs
    stage = 2 * span_l
    local = torch.full((span_l,), 0x5A, dtype=torch.uint8)
    for r in range(rows):
        local[r * ls:r * ls + 2 * row_elems] = x[r].contiguous().view(torch.uint8)
    write_local(a, 0, local)
    write_remote(a, stage, base, torch.full((span_r,), 0xA5, dtype=torch.uint8))
    a.quant_strided_batch(np.array([[1, 0, base, row_elems, rows, ls, rs]]), dtype, format="mxfp4")
    want = torch.full((span_r,), 0xA5, dtype=torch.uint8)
    recs = mx4_rows_reference(x)
    for r in range(rows):
        want[r * rs:r * rs + rec] = recs[r]
    got = read_remote(a, stage, base, span_r)
    assert torch.equal(got, want), (rows, row_elems, extra_stride, (got != want).nonzero()[:8].reshape(-1).tolist())
    # a plain converting get reads one row of it
    r = rows - 1
    write_local(a, span_l, torch.full((2 * row_elems,), 0x5A, dtype=torch.uint8))
    a.quant_batch(np.array([[0, span_l, base + r * rs, row_elems]]), dtype, format="mxfp4")
    assert torch.equal(read_local(a, span_l, 2 * row_elems).view(torch.int16), roundtrip(x[r]).view(torch.int16))
    # and the strided get, beside the source rows
    write_local(a, span_l, torch.full((span_l,), 0x5A, dtype=torch.uint8))
    a.quant_strided_batch(np.array([[0, span_l, base, row_elems, rows, ls, rs]]), dtype, format="mxfp4")
    want_l = torch.full((span_l,), 0x5A, dtype=torch.uint8)
    for r in range(rows):
        want_l[r * ls:r * ls + 2 * row_elems] = roundtrip(x[r]).view(torch.uint8)
    assert torch.equal(read_local(a, span_l, span_l), want_l), (rows, row_elems, extra_stride)
    return span_l, span_r


def exercise_kv(kv, rounds, seed, device):
    """Swap blocks out and in on an MXFP4 pool, whole blocks or layered: what comes back is the
    oracle round trip of what was written, per record (a block, or a layer of a block)."""
    rng = random.Random(seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    lead = (kv.layers,) if kv.layers else ()
    bdim = 1 if kv.layers else 0
    pool_model = {}
    for r in range(rounds):
        fresh = (torch.randn((*lead, kv.num_gpu_blocks, *kv.block_shape), generator=g) * 3).to(kv.dtype)
        kv.gpu_cache.copy_(fresh.to(device))
        k = rng.randint(1, kv.num_gpu_blocks)
        gpu_ids = rng.sample(range(kv.num_gpu_blocks), k)
        pool_ids = rng.sample(range(kv.num_pool_blocks), k)
        assert kv.swap_out(list(zip(gpu_ids, pool_ids)), async_=bool(r % 2)) == k
        for gi, pi in zip(gpu_ids, pool_ids):
            blk = fresh.select(bdim, gi)  # [layers, *block] or [*block]
            pool_model[pi] = roundtrip(blk.reshape(max(kv.layers, 1), -1)).view(blk.shape)
        kv.gpu_cache.zero_()
        back = rng.sample(list(pool_model), min(len(pool_model), kv.num_gpu_blocks))
        dst = rng.sample(range(kv.num_gpu_blocks), len(back))
        kv.swap_in(list(zip(back, dst)), async_=bool(r % 2))
        for pi, gi in zip(back, dst):
            got = kv.gpu_cache.select(bdim, gi).cpu()
            assert torch.equal(got.view(torch.int16), pool_model[pi].view(torch.int16)), (r, pi, gi)
    kv.wait()
