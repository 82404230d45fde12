"""Cases shared by the pooled-lookup tests (test_bag_cpu.py, test_gpu_bag.py): a numpy model of
ocm_copy_onesided_bag, its rule step by step in float32 (products and sums kept apart, in the order of
the ids), and a layout helper that never lets an op write what another op reads. Every byte of both
halves is compared with the model."""
from fractions import Fraction

import numpy as np
import torch

from quant_cases import UNIT, read_local, read_remote, write_local, write_remote  # noqa: F401  (re-exported)

NONE = (1 << 64) - 1
F32, BF16, FP16 = 1, 2, 3                 # enum ocm_acc_dtype
DTYPES = (F32, BF16, FP16)
ESIZE = {F32: 4, BF16: 2, FP16: 2}
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, FP16: torch.float16}
SUM, MEAN = 0, 1
NP_INDEX = {1: np.int32, 2: np.int64}
TORCH_INDEX = {1: torch.int32, 2: torch.int64}
IN_FLIGHT = 4                             # kBagInFlight of csrc/include/ocm/bag.h
TILE = 1024                               # kBagTileBytes
LENGTHS = (0, 1, 2, IN_FLIGHT, IN_FLIGHT + 1, 2 * IN_FLIGHT + 1, 37)
# columns of an op row: the fields of struct ocm_bag_params in order
LOFF, ROFF, RELEMS, BAGS, IDS, LSTRIDE, RSTRIDE, RROWS, IOFF, OOFF, WOFF = range(11)


def _up(x, m):
    return (x + m - 1) // m * m


# ---- element types ----
def widen(raw, dtype):
    """Raw row bytes (uint8) as float32 values, exactly."""
    if dtype == F32:
        return raw.view(np.float32).copy()
    h = raw.view(np.uint16)
    if dtype == BF16:
        return (h.astype(np.uint32) << 16).view(np.float32)
    return h.view(np.float16).astype(np.float32)


def narrow(acc, dtype):
    """float32 values as raw bytes of `dtype`, round to nearest even."""
    acc = np.asarray(acc, dtype=np.float32)
    if dtype == F32:
        return acc.view(np.uint8).copy()
    if dtype == FP16:
        with np.errstate(over="ignore"):
            return acc.astype(np.float16).view(np.uint8).copy()
    u = acc.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    r = np.where(nan, (u >> 16) | 0x40, r)
    return r.astype(np.uint16).view(np.uint8).copy()


def raw_rows(values, dtype):
    """A (rows, elems) array of values (each exactly representable in `dtype`) as (rows, row bytes) uint8."""
    v = np.asarray(values, dtype=np.float32)
    raw = narrow(v.reshape(-1), dtype).reshape(v.shape[0], -1)
    assert np.array_equal(widen(raw.reshape(-1), dtype).reshape(v.shape), v), "values must be exact in the table's type"
    return raw


# ---- the rule ----
def bag_sum(rows, weights=None):
    """fl32 sum of float32 rows in order: acc = fl32(acc + fl32(w * x)), two roundings."""
    acc = np.zeros(rows[0].shape if len(rows) else 0, dtype=np.float32)
    for j, x in enumerate(rows):
        p = x if weights is None else np.float32(weights[j]) * x  # float32 * float32: one rounding
        acc = acc + p                                              # and another
    return acc


def _round_f32(q):
    """The Fraction q rounded to float32, to nearest even."""
    c = np.float32(float(q))
    best = None
    for v in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        d = abs(Fraction(float(v)) - q)
        even = (int(np.float32(v).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, v)
    return np.float32(best[1])


def bag_sum_fma(rows, weights):
    """The same sum with every term fused: acc = fl32(acc + w * x), one rounding (what the rule forbids)."""
    acc = np.zeros(rows[0].shape, dtype=np.float32)
    for j, x in enumerate(rows):
        acc = np.array([_round_f32(Fraction(float(a)) + Fraction(float(weights[j])) * Fraction(float(e))) for a, e in zip(acc, x)],
                       dtype=np.float32)
    return acc


def _index(arr, off, itype, n):
    size = 4 * itype
    return [int(v) for v in np.frombuffer(arr[off:off + n * size].tobytes(), dtype=NP_INDEX[itype])]


def bag_range(off_b, off_b1, ids):
    """[lo, hi) of a bag from its two offsets as read (signed), compared as unsigned and clamped."""
    lo, hi = (min(v if v >= 0 else v + (1 << 64), ids) for v in (off_b, off_b1))
    return lo, max(hi, lo)


def model(local, remote, ops, modes, itype, dtype):
    """The local byte array after the ops, and the number of entries skipped. The arrays are read
    from `local` as it was; the remote half is only read."""
    out = np.array(local, dtype=np.uint8)
    skipped = 0
    es = ESIZE[dtype]
    for o, mode in zip(ops, modes):
        loff, roff, relems, bags, ids, ls, rs, rrows, ioff, ooff, woff = (int(v) for v in o)
        if bags == 0:
            continue
        rb = relems * es
        offs = _index(local, ooff, itype, bags + 1)
        idx = _index(local, ioff, itype, ids) if ids else []
        w = np.frombuffer(local[woff:woff + 4 * ids].tobytes(), dtype=np.float32) if ids and woff != NONE else None
        for b in range(bags):
            lo, hi = bag_range(offs[b], offs[b + 1], ids)
            rows, ws = [], []
            for j in range(lo, hi):
                if not 0 <= idx[j] < rrows:  # unsigned compare: negatives are out of range
                    skipped += 1
                    continue
                at = roff + idx[j] * rs
                rows.append(widen(remote[at:at + rb], dtype))
                ws.append(w[j] if w is not None else None)
            acc = bag_sum(rows, ws if w is not None else None) if rows else np.zeros(relems, dtype=np.float32)
            if mode == MEAN and hi > lo:
                acc = acc / np.float32(hi - lo)  # one float32 division; skipped entries count
            out[loff + b * ls: loff + b * ls + rb] = narrow(acc, dtype)
    return out, skipped


def nominal(ops, dtype):
    """(bags, ids, nominal bytes read) of the ops with bags."""
    live = [o for o in ops if int(o[BAGS])]
    return (sum(int(o[BAGS]) for o in live), sum(int(o[IDS]) for o in live),
            sum(int(o[IDS]) * int(o[RELEMS]) * ESIZE[dtype] for o in live))


# ---- layouts ----
class Layout:
    """Lays tables, arrays and outputs out in one pair so that no op writes what another reads: every
    output table takes a fresh range of the local half, every array a fresh range that no op writes,
    every table a fresh range of the remote half, which nothing writes."""

    def __init__(self, itype, dtype):
        self.itype, self.dtype = itype, dtype
        self.lpos, self.rpos = 0, 0
        self.ops, self.modes = [], []
        self.local_data, self.remote_data = [], []  # (offset, uint8 bytes)

    def table(self, values, gap=0, lead=16):
        """A remote table of the rows `values` (rows x elems), `gap` bytes between rows, `lead` bytes in."""
        raw = raw_rows(values, self.dtype)
        stride = raw.shape[1] + gap
        off = _up(self.rpos, 16) + lead
        assert off % 16 == 0 and stride % 16 == 0
        for r in range(raw.shape[0]):
            self.remote_data.append((off + r * stride, raw[r]))
        self.rpos = off + (raw.shape[0] - 1) * stride + raw.shape[1]
        return dict(off=off, stride=stride, rows=raw.shape[0], elems=np.asarray(values).shape[1])

    def array(self, values, np_dtype):
        vals = np.asarray(values, dtype=np_dtype)
        off = _up(self.lpos, 8)
        self.local_data.append((off, np.frombuffer(vals.tobytes(), dtype=np.uint8)))
        self.lpos = off + max(vals.nbytes, 1)
        return off

    def bag(self, table, ids, offsets, weights=None, mode=SUM, out_gap=0, n_ids=None, bags=None, rows=None, off=None):
        """An op over `table`: offsets has bags + 1 entries (any values: the rule clamps them). n_ids,
        bags, rows, off: what the op says instead of what the arrays and the table have."""
        bags = len(offsets) - 1 if bags is None else bags
        n_ids = len(ids) if n_ids is None else n_ids
        rb = table["elems"] * ESIZE[self.dtype]
        ioff = self.array(ids, NP_INDEX[self.itype])
        ooff = self.array(offsets, NP_INDEX[self.itype])
        woff = self.array(weights, np.float32) if weights is not None else NONE
        loff = _up(self.lpos, 16)
        ls = rb + out_gap
        assert ls % 16 == 0
        self.lpos = loff + max(bags, 1) * ls
        self.ops.append([loff, table["off"] if off is None else off, table["elems"], bags, n_ids, ls, table["stride"],
                         table["rows"] if rows is None else rows, ioff, ooff, woff])
        self.modes.append(mode)
        return self.ops[-1]

    @property
    def local_bytes(self):
        return _up(self.lpos + 64, 4096)

    @property
    def remote_bytes(self):
        return max(_up(self.rpos + 64, UNIT), 4 * UNIT)  # at least a unit on each of three owners

    def images(self, seed):
        """Both halves as the run starts: random bytes, the tables and the arrays."""
        rng = np.random.RandomState(seed)
        local = rng.randint(0, 256, self.local_bytes).astype(np.uint8)
        remote = rng.randint(0, 256, self.remote_bytes).astype(np.uint8)
        for img, data in ((local, self.local_data), (remote, self.remote_data)):
            for off, raw in data:
                img[off:off + len(raw)] = raw
        return local, remote


def fill(a, local, remote):
    """Writes both images into the pair (the remote one with plain puts staged in the local half)."""
    chunk = min(len(local), len(remote))
    for off in range(0, len(remote), chunk):
        write_remote(a, 0, off, torch.from_numpy(remote[off:off + chunk].copy()))
    write_local(a, 0, torch.from_numpy(local.copy()))


def remote_bytes_of(a, local_bytes, remote_bytes):
    """The whole remote half, read with plain gets through the local half (which is put back)."""
    keep = read_local(a, 0, local_bytes)
    chunk = min(local_bytes, remote_bytes)
    out = [read_remote(a, 0, off, min(chunk, remote_bytes - off)) for off in range(0, remote_bytes, chunk)]
    write_local(a, 0, keep)
    return torch.cat(out).numpy()


def run_layout(a, lay, seed=1, async_=False):
    """Runs the layout's ops as one list and compares every byte of both halves with the model. Returns
    the model's skip count and the error the call (or the wait) raised, for the caller to check."""
    local, remote = lay.images(seed)
    fill(a, local, remote)
    want, skipped = model(local, remote, lay.ops, lay.modes, lay.itype, lay.dtype)
    err = None
    try:
        a.bag_batch(lay.ops, lay.dtype, lay.itype, lay.modes, async_=async_)
        if async_:
            a.wait()
    except Exception as e:  # noqa: BLE001  (the caller sees it)
        err = e
    got = read_local(a, 0, lay.local_bytes).numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"local half: {bad.size} bad bytes, first {bad[:4]}, in ops {_ops_of(lay, bad[:4])}"
    assert np.array_equal(remote_bytes_of(a, lay.local_bytes, lay.remote_bytes), remote), "the remote half changed"
    return skipped, err


def _ops_of(lay, where):
    return [next((i for i, o in enumerate(lay.ops) if o[LOFF] <= w < o[LOFF] + max(o[BAGS], 1) * o[LSTRIDE]), None) for w in where]


def grid_values(rng, rows, elems):
    """Random multiples of 1/16 up to 8 in size: exact in every element type, sums of 37 exact in float32."""
    return rng.randint(-127, 128, (rows, elems)).astype(np.float32) / np.float32(16)


def bag_lengths(bags):
    """`bags` bag lengths out of LENGTHS in turn; with more than two bags the first and the last are empty."""
    lens = [LENGTHS[(i + 1) % len(LENGTHS)] for i in range(bags)]
    if bags <= 2:
        lens = [IN_FLIGHT + 1, 2 * IN_FLIGHT + 1][:bags]
    if bags > 2:
        lens[0] = lens[-1] = 0
        assert set(lens) == set(LENGTHS) or bags < len(LENGTHS) + 2
    return lens


def ids_for(rng, lens, table_rows):
    """Ids for bags of these lengths: random rows with a duplicate inside every bag of three or more,
    and one id repeated through the whole of every bag of 2 * IN_FLIGHT + 1; the offsets go with them."""
    ids, offsets = [], [0]
    for n in lens:
        bag = [int(v) for v in rng.randint(0, table_rows, n)]
        if n >= 3:
            bag[-1] = bag[0]
        if n == 2 * IN_FLIGHT + 1:
            bag = [bag[0]] * n
        ids += bag
        offsets.append(len(ids))
    return ids, offsets


def shapes_layout(itype, dtype, row_bytes, bags, seed, table_rows=19, gap=0):
    """One list over one table of rows of row_bytes: a sum, a weighted sum, a mean and an op without
    ids, each of `bags` bags whose lengths are bag_lengths(bags)."""
    rng = np.random.RandomState(seed)
    lay = Layout(itype, dtype)
    elems = row_bytes // ESIZE[dtype]
    t = lay.table(grid_values(rng, table_rows, elems), gap=gap)
    lens = bag_lengths(bags)
    for k, mode in enumerate((SUM, SUM, MEAN)):
        ids, offsets = ids_for(rng, lens, table_rows)
        w = None
        if k == 1:  # weights with a few bits each, so that products round
            w = rng.randint(-64, 65, len(ids)).astype(np.float32) / np.float32(48)
        lay.bag(t, ids, offsets, weights=w, mode=mode, out_gap=16 * (k % 2))
    lay.bag(t, [], [0] * (bags + 1))  # ids == 0: zeros to every bag
    return lay


def order_values(dtype):
    """Four values whose float32 sum depends on the order: big, small, -big, small."""
    big, small = (2.0 ** 15, 2.0 ** -10) if dtype == FP16 else (2.0 ** 25, 1.0)
    return [big, small, -big, small]


def tie_rows(dtype):
    """Rows of two elements whose two-row sums lie halfway between two values of the 16-bit type:
    1 + half an ulp (to even: down) and 1 + ulp + half an ulp (to even: up)."""
    ulp = 2.0 ** -7 if dtype == BF16 else 2.0 ** -10
    return [[1.0, 1.0 + ulp], [ulp / 2, ulp / 2]]


def fma_case(dtype):
    """(rows, weights) of a weighted bag of three one-element rows whose in-order two-rounding sum
    differs from the reversed order and from the fused sum, also after narrowing to `dtype`. With
    a = 1 + one ulp of the 16-bit type, b = 1 + 2^-23 and s = 2^20, the product (b s) * a has one bit
    more than float32 holds: P = fl32(b s a) drops s * 2^-30 (s * 2^-33 for float16). The terms are
    (-P) * 1, (b s) * a, 1 * 2^-8: in order, -P + P is 0 and the sum is 2^-8; fused, the second term
    leaves the dropped bit, 2^-10 (2^-13), and the sum is 2^-8 + 2^-10; reversed, 2^-8 is lost below
    P's ulp of 2^-3 and the sum is 0."""
    a = np.float32(1 + (2.0 ** -10 if dtype == FP16 else 2.0 ** -7))
    bs = np.float32((1 + 2.0 ** -23) * 2.0 ** 20)
    P = np.float32(bs * a)
    assert Fraction(float(P)) != Fraction(float(bs)) * Fraction(float(a))  # the product rounds
    x = np.array([[1.0], [a], [2.0 ** -8]], dtype=np.float32)
    w = np.array([-P, bs, 1.0], dtype=np.float32)
    return x, w


def order_layout(itype, dtype):
    """The cases that catch a wrong order, a fused multiply-add, a wrong divisor and a wrong rounding."""
    lay = Layout(itype, dtype)
    vals = order_values(dtype)
    elems = 16 // ESIZE[dtype]  # one vector
    # every element of row r holds vals[r] (times a power of two per element, which changes no rounding)
    scale = np.array([1.0, 0.5, 0.25, 1.0] * 2, dtype=np.float32)[:elems]
    t = lay.table(np.outer(np.array(vals, dtype=np.float32), scale))
    lay.bag(t, [0, 1, 2, 3, 3, 2, 1, 0], [0, 4, 8])  # the first bag in order (small), the second reversed (0)
    x, w = fma_case(dtype)
    tf = lay.table(np.repeat(x, elems, axis=1))
    lay.bag(tf, [0, 1, 2, 2, 1, 0], [0, 3, 6], weights=np.concatenate([w, w[::-1]]))
    rng = np.random.RandomState(5)
    tm = lay.table(grid_values(rng, 9, elems))
    lay.bag(tm, [int(v) for v in rng.randint(0, 9, 10)], [0, 3, 10], mode=MEAN)  # bags of 3 and 7
    if dtype != F32:
        tt = lay.table(np.repeat(np.array(tie_rows(dtype), dtype=np.float32), 4, axis=1))
        lay.bag(tt, [0, 1], [0, 2])
    return lay


def clamp_layout(itype, dtype):
    """Offsets that the rule clamps: an entry above ids, a decreasing pair, a negative entry."""
    rng = np.random.RandomState(8)
    lay = Layout(itype, dtype)
    t = lay.table(grid_values(rng, 11, 8))
    ids = [int(v) for v in rng.randint(0, 11, 12)]
    lay.bag(t, ids, [0, 5, 3, 9, 40, 7, 12])       # [0,5) [5,5) [3,9) [9,12) [12,12) [7,12)
    lay.bag(t, ids, [2, -1, 4, 1 << 30, 12])       # [2,12) [12,12) [4,12) [12,12)
    return lay


def mixed_layout(itype, dtype, n_ops, seed=11):
    """n_ops mixed ops (sums, weighted sums, means; rows of 16 bytes to over two tiles; 1 to 5 bags)
    with ops without bags first, in the middle and last."""
    rng = np.random.RandomState(seed)
    lay = Layout(itype, dtype)
    tables = [lay.table(grid_values(rng, 7, rb // ESIZE[dtype]), gap=16 * i) for i, rb in enumerate((16, 48, 1024, 1040, 2064))]
    for i in range(n_ops):
        t = tables[int(rng.randint(0, len(tables)))]
        lens = [int(v) for v in rng.choice(LENGTHS[:-1], int(rng.randint(1, 6)))]
        ids, offsets = ids_for(rng, lens, t["rows"])
        kind = i % 3
        w = rng.randint(-64, 65, len(ids)).astype(np.float32) / np.float32(48) if kind == 1 else None
        empty = i in (0, n_ops // 2, n_ops // 2 + 1, n_ops - 1)
        lay.bag(t, ids, offsets, weights=w, mode=MEAN if kind == 2 else SUM, out_gap=16 * (i % 2), bags=0 if empty else None)
    return lay


def window_layout(itype, dtype):
    """Out-of-range ids that even a broken check keeps inside the pair: the table is a window of 8 rows
    that starts 4 rows into a region of 64 rows of the remote half, and the bad ids are only -4 .. -1
    and 8 .. 40. Rows of three tiles: an entry is still counted once. Returns the layout and the count."""
    rng = np.random.RandomState(4)
    lay = Layout(itype, dtype)
    region = lay.table(grid_values(rng, 64, 2064 // ESIZE[dtype]), gap=16)
    assert region["stride"] * 64 + region["off"] <= lay.remote_bytes
    win = region["off"] + 4 * region["stride"]
    ids = [3, -4, 0, 8, 7, 40, -1, 5, 9, 9, 2]
    bad = [v for v in ids if not 0 <= v < 8]
    assert all(-4 <= v <= 40 for v in ids)
    lay.bag(region, ids, [0, 0, 6, 7, 11], rows=8, off=win)                       # bags: -, 3 bad of 6, all bad, 2 bad of 4
    lay.bag(region, ids, [0, 6, 11], rows=8, off=win, mode=MEAN)                  # the divisor counts them
    lay.bag(region, ids, [0, 11], rows=8, off=win, weights=np.arange(11) / np.float32(4))
    return lay, 3 * len(bad)
