"""Cases shared by the converting-transfer tests (test_quant_cpu.py, test_gpu_quant.py):
the edge groups, the all-patterns sweep, the decode table (every code under every scale
byte), the non-finite groups, the 60-op list, and helpers that move raw bytes through an
allocation. Everything is compared byte for byte with the torch oracle
(oncilla_amd.ops.quant); the one allowance is the payload of a NaN that a NaN code decodes to."""
import functools
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


def _up(x, m):
    return (x + m - 1) // m * m


def mismatches(got, want, show=int, where=None):
    """(count, the first dozen (index, got, want)) of the elements that differ, of those that
    `where` selects if it is given."""
    bad = got != want
    if where is not None:
        bad &= where
    bad = bad.nonzero().reshape(-1)
    return bad.numel(), [(int(i), show(got[i]), show(want[i])) for i in bad[:12]]


def hex16(v):
    return hex(int(v) & 0xFFFF)


# ---- the all-patterns sweep ----

def all_patterns(dtype):
    """Every 16-bit pattern of `dtype`, twice, 131072 elements in 4096 groups: once in pattern
    order (a group holds 32 neighbouring values: codes near the top of the range) and once dealt
    out 2048 apart (a group spans every binade and both signs: most of it rounds to zero). Inf
    and NaN patterns are replaced by zero."""
    p = torch.arange(65536, dtype=torch.int32)
    both = torch.cat([p, p.view(32, 2048).t().reshape(-1)])
    exp_all_ones = (both & 0x7F80) == 0x7F80 if dtype == torch.bfloat16 else (both & 0x7C00) == 0x7C00
    both = torch.where(exp_all_ones, torch.zeros_like(both), both)
    x = both.to(torch.int16).view(dtype)
    assert torch.isfinite(x.float()).all()
    return x


@functools.lru_cache(maxsize=None)
def sweep(dtype):
    """all_patterns(dtype) with the oracle's MXFP8 results: (elements, record, decoded), computed
    once per dtype and shared: treat them as read-only."""
    x = all_patterns(dtype)
    codes, scales = mx8_encode_reference(x)
    return x, torch.cat([codes, scales]), mx8_decode_reference(codes, scales, dtype)


def run_sweep(a, dtype):
    """One put of the whole sweep at remote offset UNIT - 64 (codes and scale bytes cross stripe
    units), the record against the oracle's; one get back into a range filled with 0x5A5A, the
    elements against the oracle's decode. Needs sweep_bytes() in the pair."""
    x, record, decoded = sweep(dtype)
    n = x.numel()
    write_local(a, 0, x)
    a.quant_batch(np.array([[1, 0, UNIT - 64, n]]), dtype)
    got = read_remote(a, 2 * n, UNIT - 64, record.numel())
    count, first = mismatches(got, record)
    assert count == 0, ("record", count, first)
    write_local(a, 0, torch.full((n,), 0x5A5A, dtype=torch.int16))
    a.quant_batch(np.array([[0, 0, UNIT - 64, n]]), dtype)
    got = read_local(a, 0, 2 * n).view(torch.int16)
    count, first = mismatches(got, decoded.view(torch.int16), hex16)
    assert count == 0, ("decoded", count, first)


def sweep_bytes():
    """(local_bytes, remote_bytes) of the pair run_sweep needs: the elements and a staging range
    for the record behind them; the record from UNIT - 64."""
    n, rec = 131072, api.quant_bytes(131072)
    return 2 * n + _up(rec, UNIT), _up(UNIT + rec, UNIT)


# ---- decode tables: every code under every scale byte ----

class DecodeTable:
    """A record that no encoder wrote: `codes` and `scales` (uint8) as they are, 32 elements per
    scale byte, decoded by one converting get and compared bit for bit with `decode` (the
    oracle). `nan` marks the elements whose code is a NaN code, if the format has any: those
    decode to some NaN of the element type, the payload is not specified, and everything else
    is exact."""

    def __init__(self, fmt, codes, scales, decode, nan=None):
        self.fmt, self.codes, self.scales, self._decode, self.nan = fmt, codes, scales, decode, nan
        self.elems = 32 * scales.numel()
        assert api.quant_bytes(self.elems, fmt) == codes.numel() + scales.numel()
        self._want = {}

    def record(self):
        return torch.cat([self.codes, self.scales])

    def row_records(self, rows):
        """The table as `rows` records of elems / rows elements each: [rows, record bytes], row
        r holding its share of the codes, then its share of the scale bytes."""
        assert self.elems % (32 * rows) == 0
        return torch.cat([self.codes.view(rows, -1), self.scales.view(rows, -1)], dim=1)

    def want(self, dtype):
        """The oracle's decode as int16, computed once per dtype: treat it as read-only. Its rows
        are the decodes of row_records(), a row being whole groups."""
        if dtype not in self._want:
            self._want[dtype] = self._decode(self.codes, self.scales, dtype).view(torch.int16)
        return self._want[dtype]

    def check(self, got, dtype):
        """got: the decoded elements as int16."""
        want = self.want(dtype)
        exact = None
        if self.nan is not None:
            assert torch.isnan(want.view(dtype)[self.nan].float()).all()  # the oracle's are NaNs too
            not_nan = (~torch.isnan(got.view(dtype).float())) & self.nan
            assert not not_nan.any(), ("NaN codes that decoded to a number", int(not_nan.sum()),
                                       [(int(i), hex16(got[i])) for i in not_nan.nonzero().reshape(-1)[:12]])
            exact = ~self.nan
        count, first = mismatches(got, want, hex16, exact)
        assert count == 0, (self.fmt, count, first)

    def bytes(self, rows=1):
        """(local_bytes, remote_bytes) of the pair run() or run_strided(rows) needs."""
        ls, rs = self._strides(rows)
        return _up(rows * ls + rows * rs, UNIT), _up(UNIT + rows * rs, UNIT)

    def _strides(self, rows):
        if rows == 1:
            return 2 * self.elems, _up(self.codes.numel() + self.scales.numel(), 32)
        return 2 * self.elems // rows + 16, _up(api.quant_bytes(self.elems // rows, self.fmt), 32) + 32

    def run(self, a, dtype):
        """The record raw into the remote half at UNIT - 64 with a plain put, one converting get
        into a range filled with 0x5A5A."""
        n = self.elems
        write_remote(a, 2 * n, UNIT - 64, self.record())
        write_local(a, 0, torch.full((n,), 0x5A5A, dtype=torch.int16))
        a.quant_batch(np.array([[0, 0, UNIT - 64, n]]), dtype, format=self.fmt)
        self.check(read_local(a, 0, 2 * n).view(torch.int16), dtype)

    def run_strided(self, a, dtype, rows):
        """The same values through the strided op: the table as `rows` records, a remote stride
        of the rounded record plus 32 and a local one of the row plus 16, one strided converting
        get into a range filled with 0x5A; the bytes between the decoded rows keep the fill."""
        re = self.elems // rows
        ls, rs = self._strides(rows)
        recs = torch.full((rows, rs), 0xA5, dtype=torch.uint8)
        rr = self.row_records(rows)
        recs[:, :rr.shape[1]] = rr
        write_remote(a, rows * ls, UNIT - 64, recs)
        write_local(a, 0, torch.full((rows * ls,), 0x5A, dtype=torch.uint8))
        a.quant_strided_batch(np.array([[0, 0, UNIT - 64, re, rows, ls, rs]]), dtype, format=self.fmt)
        got = read_local(a, 0, rows * ls).view(rows, ls)
        assert (got[:, 2 * re:] == 0x5A).all(), "the bytes behind a decoded row"
        self.check(got[:, :2 * re].contiguous().view(torch.int16).reshape(-1), dtype)


@functools.lru_cache(maxsize=None)
def decode_table():
    """MXFP8: 65536 codes, code[i] = i & 255, under 2048 scale bytes, scale[g] = g // 8: every
    scale byte 0..255 meets every code, scale byte 255 (float(code) * 2^128: infinities, zero
    for the zero codes) and 0 (fp32 subnormal products) included. The 512 elements whose code
    is 0x7f or 0xff decode to some NaN."""
    codes = (torch.arange(65536, dtype=torch.int32) & 255).to(torch.uint8)
    scales = (torch.arange(2048, dtype=torch.int32) // 8).to(torch.uint8)
    nan = (codes & 0x7F) == 0x7F
    assert int(nan.sum()) == 512  # the NaN allowance covers these and nothing else
    return DecodeTable("mxfp8", codes, scales, mx8_decode_reference, nan)


TABLE_ROWS = 32  # the MXFP8 table as rows of 2048 elements: one tile each


# ---- non-finite groups ----

N_NONFINITE = 2048 + 64  # one tile and two groups: both MXFP8 rounds and a second tile take part
# (group, element of the group, value): group 3 is lanes 6 and 7 of the MXFP8 tile and the element
# sits in the odd lane, whose maximum reaches lane 6 by the shuffle; group 40 is in the second
# MXFP8 round; group 65 is the last one, in the second tile
NONFINITE = ((3, 21, float("inf")), (40, 5, float("nan")), (65, 31, float("-inf")))


def run_nonfinite_put(a, dtype, fmt, record_reference):
    """A put of random elements with an Inf, a NaN and a -Inf in three groups: every code and scale
    byte of every other group equals the oracle record of the same input with those three groups
    zeroed, and 32 sentinel bytes before and after the record are intact. The three groups' own
    bytes are not compared (their codes are unspecified). Needs 16384 local and 4 * UNIT remote bytes."""
    n, ng = N_NONFINITE, N_NONFINITE // 32
    x = random_elems(n, dtype, seed=77)
    clean = x.clone()
    for g, k, v in NONFINITE:
        x[32 * g + k] = v
        clean[32 * g:32 * g + 32] = 0
    assert int((~torch.isfinite(x.float())).sum()) == 3 and torch.isfinite(clean.float()).all()
    want = record_reference(clean)
    rb = api.quant_bytes(n, fmt)
    per = (rb - ng) // ng  # code bytes of a group
    compared = torch.ones(rb, dtype=torch.bool)
    for g, _, _ in NONFINITE:
        compared[per * g:per * g + per] = False
        compared[rb - ng + g] = False
    assert int(compared.sum()) == rb - 3 * (per + 1)
    stage, ro = 8192, UNIT - 64
    fill = torch.full((32,), 0xA5, dtype=torch.uint8)
    write_remote(a, stage, ro - 32, torch.full((rb + 64,), 0xA5, dtype=torch.uint8))
    write_local(a, 0, x)
    a.quant_batch(np.array([[1, 0, ro, n]]), dtype, format=fmt)
    got = read_remote(a, stage, ro - 32, rb + 64)
    assert torch.equal(got[:32], fill) and torch.equal(got[-32:], fill), "the bytes around the record"
    count, first = mismatches(got[32:-32], want, int, compared)
    assert count == 0, (fmt, count, first)


def run_nan_codes_get(a, dtype):
    """The get direction, MXFP8: the oracle record of a finite input with three codes overwritten
    by the NaN codes 0x7f / 0xff, in the groups of NONFINITE. Those three elements decode to a
    NaN; every other element equals the oracle decode exactly."""
    n = N_NONFINITE
    x = random_elems(n, dtype, seed=78)
    record = mx8_record_reference(x)
    want = roundtrip(x).view(torch.int16)
    at = torch.zeros(n, dtype=torch.bool)
    for (g, k, _), code in zip(NONFINITE, (0x7F, 0xFF, 0x7F)):
        record[32 * g + k] = code
        at[32 * g + k] = True
    stage, ro = 8192, UNIT - 64
    write_remote(a, stage, ro, record)
    write_local(a, 0, torch.full((n,), 0x5A5A, dtype=torch.int16))
    a.quant_batch(np.array([[0, 0, ro, n]]), dtype)
    got = read_local(a, 0, 2 * n).view(torch.int16)
    assert torch.isnan(got.view(dtype)[at].float()).all(), [hex16(v) for v in got[at]]
    count, first = mismatches(got, want, hex16, ~at)
    assert count == 0, (count, first)


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
