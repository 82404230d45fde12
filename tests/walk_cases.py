"""Lists sized from the wave count of their launch (test_list_walk_cpu.py, test_gpu_list_walk.py), one
builder per kind of descriptor list: every wave of the launch walks at least three tiles, so the state a
list kernel carries from tile to tile (row and piece counters, the indices of a row, the skip flag, the
per-op scalars, the scale row in LDS) is what the comparison rests on.

A builder takes `waves` and returns a case whose `lower_bound` counts the units every kind's tile rule
gives at least one tile for (non-empty ops, non-empty rows, bags of a non-empty row), without mirroring
the rule itself; the tests assert lower_bound >= 2 * waves + 1 before they run anything. Most units are
tiny (16-byte rows, 4 fp32 elements, 32 converted elements); in the middle of the tile sequence lie ops
whose rows or ops have 2 and 3 tiles, each as several stretches a one-tile unit apart (so that waves start
inside a row, at every piece, whatever a wave's share of tiles is: wave_ranges, asserted on the CPU), runs
of one-row ops, empty ops, and for the indexed kinds rows
with out-of-range indices inside windows (whatever a broken check lets through stays inside the pair).
Adjacent ops differ in direction, row size, indexed side, element type, format, scale, weights and mode.
No op writes what another op of the list reads (check_disjoint), so the result does not depend on the
order of the waves. The models are those of the kinds' own case files."""
import numpy as np
import torch

import acc_cases
import bag_cases
import indexed_cases
import quant_indexed_cases
import strided_cases
from oncilla_amd import api
from oncilla_amd.ops import accumulate_reference
from quant_cases import UNIT, random_elems, read_local
from quant_indexed_cases import record_bytes, record_up32, table_reference
from quant_strided_cases import load_pair
from strided_cases import SENTINEL, fill_pair, remote_bytes_of

# The stripe unit of every pool here. ocm_alloc takes no unit below 4 KiB, so the byte tile of the
# striped pool is 4 KiB as well and rows of 2 and 3 byte tiles have some 4.1 and 8.2 KB.
assert UNIT == 4096
HOST_WAVES = 4 * 128                       # the host tier's launch: 128 workgroups of 4 waves
WAVES = (HOST_WAVES, 4 * 8 * 256, 4 * 8 * 304)  # and 8 workgroups per CU on 256 and on 304 CUs
# Rows (or ops) of 3 tiles in a list: about 40 where a tile has 4 KiB (rows of 8.2 KB), a few hundred
# where tiles are fixed and small. They come as three ops (stretches) with a one-tile unit between them,
# so that whatever multiple of 3 a wave's share of tiles is, waves start at piece 1 and at piece 2.
MULTI_BYTE_TILES, MULTI_FIXED_TILES = 39, 240
MULTI2 = 40                                # rows of 2 tiles, as two ops with a one-tile row between them

BYTES = {1: (16, 24, 17), 2: (4100, 4103, 4111), 3: (8200, 8195, 8207)}  # rows of 1, 2, 3 byte tiles
QUANT_ELEMS = {1: 32, 2: 2048 + 32, 3: 2 * 2048 + 32}                    # of 2048-element tiles
ACC_ELEMS = {1: 4, 2: 1024 + 4, 3: 2 * 1024 + 4}                         # of 1024-element tiles
BAG_ROW_BYTES = {1: 16, 2: 1024 + 16, 3: 2 * 1024 + 16}                  # of 1024-byte tiles
QUANT_DTYPES = (torch.bfloat16, torch.float16)
FORMATS = ("mxfp8", "mxfp4")

# Out-of-range indices: a table of WIN rows that starts LEAD rows into a region of REGION rows, and bad
# indices only out of BAD, so row LEAD + index of the region exists for every index a list names.
WIN, LEAD, REGION = 8, 4, 25
BAD = (-4, -1, 8, 20)
# Every skipped row is followed by an in-range one; the last row of 'E' is skipped and the op behind it
# is not empty. Destination indices are duplicate-free.
SKIP_OPS = {"S": dict(put=0, lidx=None, ridx=[3, -4, 0, 8, 7, 20, 5, -1, 2, 2, 6, 1]),          # a gather, rows of 3 tiles
            "E": dict(put=1, lidx=[0, -1, 2, 3, 4, 8, 6, 7, 1], ridx=[4, 5, 6, 20, 0, 1, 2, 3, -4]),
            "L": dict(put=0, lidx=[5, -4, 0, 20, 7, 8, 2], ridx=None)}
# (ids, offsets) of the bag ops in their place: bad ids inside bags, a bag of nothing else, an empty bag
BAG_SKIP_OPS = {"S": ([3, -4, 0, 8, 7, 20, 5, -1, 2, 2, 6], [0, 3, 6, 8, 9, 11, 11]),
                "E": ([1, 8, 2, -4], [0, 2, 4]),
                "L": ([20, 5, -1, 0, 7], [0, 1, 3, 5])}
SKIP_ROWS = {t: len(s["lidx"] if s["lidx"] is not None else s["ridx"]) for t, s in SKIP_OPS.items()}
BAG_SKIP_ROWS = {t: len(offsets) - 1 for t, (_, offsets) in BAG_SKIP_OPS.items()}


def _up(x, m):
    return (x + m - 1) // m * m


def need(waves):
    """The tiles a list must have for every wave of the launch to walk at least three."""
    return 2 * waves + 1


def row_plan(waves, multi=MULTI_BYTE_TILES, skip_rows=SKIP_ROWS):
    """(rows, tiles per row, skip tag) of the ops of a list of a kind whose ops have rows (for bags: bags).
    24 ops of one-tile rows carry the count; between them, in the middle of the list: runs of one-row ops,
    empty ops, `multi` rows of 3 tiles in three ops and MULTI2 rows of 2 tiles in two, each with a one-tile
    row between them, and the ops with skipped rows: the one of 3-tile rows ('S') three times, a one-tile
    row apart, so that it starts at every phase of 3."""
    one, S = (1, 1, ""), (skip_rows["S"], 3, "S")
    m3 = [(multi // 3, 3, ""), one, (multi // 3, 3, ""), one, (multi - 2 * (multi // 3), 3, "")]
    m2 = [(MULTI2 // 2, 2, ""), one, (MULTI2 // 2, 2, "")]
    mid = [[one, one, (1, 3, ""), (0, 1, ""), one] + m3 + [one, (0, 2, ""), (0, 1, "")],
           [(1, 2, ""), S, one, S, one, S, one, (skip_rows["E"], 1, "E"), one, one, one] + m2 + [one],
           [(skip_rows["L"], 1, "L"), one, (2, 3, ""), one, (0, 3, ""), (3, 2, ""), one, one]]
    per = -(-need(waves) // 24)
    fills = [(per + i % 5, 1, "") for i in range(24)]
    return fills[:8] + mid[0] + fills[8:12] + mid[1] + fills[12:16] + mid[2] + fills[16:]


def op_plan(waves, multi=MULTI_BYTE_TILES):
    """Tiles of every op (0: an empty op) of a list of a kind whose ops have no rows: need(waves) non-empty
    ops, most of one tile; a third into the list `multi` ops of 3 tiles with a one-tile op after every 13
    of them, two thirds into it MULTI2 ops of 2 tiles with a one-tile op in the middle; two empty ops
    side by side every 97 ops; single ops of 2 and 3 tiles now and then."""
    n, out, live, i = need(waves), [], 0, 0
    len3 = multi + (multi - 1) // 13
    while live < n:
        if n // 3 <= i < n // 3 + len3:
            c = 1 if (i - n // 3) % 14 == 13 else 3
        elif 2 * n // 3 <= i < 2 * n // 3 + MULTI2 + 1:
            c = 1 if i - 2 * n // 3 == MULTI2 // 2 else 2
        elif i % 97 in (50, 51):
            c = 0
        else:
            c = 2 if i % 331 == 5 else 3 if i % 499 == 7 else 1
        out.append(c)
        live += c > 0
        i += 1
    assert len(out) - live >= 2 and out[-1] > 0
    return out


def wave_ranges(total_tiles, waves):
    """[t0, t1) of every wave with tiles: list_wave_range of csrc/include/ocm/list.h."""
    per = -(-total_tiles // waves)
    return [(t, min(t + per, total_tiles)) for t in range(0, total_tiles, per)]


# ---- disjointness ----
def _spans(pairs):
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return a[a[:, 1] > a[:, 0]]


def check_disjoint(case):
    """No op writes a byte that another write of the list, or any read of it, touches; on either half."""
    t = case.touched()
    for side in ("local", "remote"):
        w, r = _spans(t[side + "_writes"]), _spans(t[side + "_reads"])
        w = w[np.argsort(w[:, 0], kind="stable")]
        assert (w[1:, 0] >= w[:-1, 1]).all(), f"{case.kind}: two writes of the {side} half overlap"
        if len(w) and len(r):
            hits = np.searchsorted(w[:, 0], r[:, 1], "left") - np.searchsorted(w[:, 1], r[:, 0], "right")
            assert (hits <= 0).all(), f"{case.kind}: a write of the {side} half overlaps a read"
        size = case.local_bytes if side == "local" else case.remote_bytes
        for s in (w, r):
            assert not len(s) or (s.min() >= 0 and s[:, 1].max() <= size)


def _plain_touched(rows, lsize, rsize):
    """rows: (put, local offset, remote offset, local bytes, remote bytes) of plain copies."""
    t = dict(local_reads=[], local_writes=[], remote_reads=[], remote_writes=[])
    for put, lo, ro, ln, rn in rows:
        t["local_reads" if put else "local_writes"].append((lo, lo + ln))
        t["remote_writes" if put else "remote_reads"].append((ro, ro + rn))
    return t


# ---- per-op element types ----
def set_op_field(ops, field, values):
    """Gives every op of a prepared list (api.quant_ops, api.bag_ops, ...) its own value of a descriptor
    field that the api functions take once per list, such as the element type. The descriptors carry it
    per op; the record array behind a prepared list (its `keep`) is written in place."""
    rec = ops.keep
    assert field in rec.dtype.names and len(values) == ops.n, (field, rec.dtype.names, len(values), ops.n)
    rec[field][:ops.n] = values


# ---- running ----
def _call(a, fn, async_):
    err = None
    try:
        fn()
        if async_:
            a.wait()
    except Exception as e:  # noqa: BLE001  (the caller sees it)
        err = e
    return err


def _compare(a, case, want_l, want_r):
    got_l = read_local(a, 0, case.local_bytes).numpy()
    bad = np.flatnonzero(got_l != want_l)
    assert bad.size == 0, f"{case.kind}: local half: {bad.size} bad bytes, first {bad[:4]}"
    got_r = remote_bytes_of(a, case.local_bytes, case.remote_bytes)
    bad = np.flatnonzero(got_r != want_r)
    assert bad.size == 0, f"{case.kind}: remote half: {bad.size} bad bytes, first {bad[:4]}"


class Case:
    """A list and its pair's sizes. run(a) fills the pair `a`, runs the list as one call, compares every
    byte of both halves with the model and returns (the model's skip count, the error the call or its
    wait raised)."""
    kind = ""
    skips = False  # the kind counts skipped rows

    @property
    def remote_bytes(self):
        return max(_up(self.rpos + 64, UNIT), 4 * UNIT)  # at least a unit on each of three owners

    @property
    def local_bytes(self):
        return _up(self.lpos + 64, 4096)


# ---- batch ----
class BatchCase(Case):
    kind = "batch"

    def __init__(self, waves):
        self.ops = []  # (op_flag, local offset, remote offset, bytes)
        self.lpos, self.rpos = 3, 21
        for i, c in enumerate(op_plan(waves)):
            n = BYTES[c][i % 3] if c else 0
            self.ops.append((i % 2, self.lpos, self.rpos, n))
            self.lpos += n + (i % 4)
            self.rpos += n + (i % 3) * 5
        self.lower_bound = sum(1 for o in self.ops if o[3])

    def touched(self):
        return _plain_touched([(f, lo, ro, n, n) for f, lo, ro, n in self.ops], self.local_bytes, self.remote_bytes)

    def run(self, a, async_=False):
        local, remote = fill_pair(a, self.local_bytes, self.remote_bytes, seed=2, random_remote=True)
        want_l, want_r = local.copy(), remote.copy()
        for f, lo, ro, n in self.ops:
            if f:
                want_r[ro:ro + n] = local[lo:lo + n]
            else:
                want_l[lo:lo + n] = remote[ro:ro + n]
        ops = api.batch_ops(np.asarray(self.ops, dtype=np.int64))
        err = _call(a, lambda: a.batch(ops, async_=async_), async_)
        _compare(a, self, want_l, want_r)
        return 0, err


# ---- strided ----
class StridedCase(Case):
    kind = "strided_batch"

    def __init__(self, waves):
        self.ops = []  # [op_flag, local offset, remote offset, row bytes, rows, local stride, remote stride]
        self.lpos, self.rpos = 3, 24
        for i, (rows, c, _) in enumerate(row_plan(waves)):
            rb = BYTES[c][i % 3]
            ls, rs = rb + (0, 7)[i % 2], rb + (0, 13, 16)[i % 3]
            op = [i % 2, _up(self.lpos, 16) + i % 16, _up(self.rpos, 16) + (5 * i) % 16, rb, rows, ls, rs]
            self.lpos, self.rpos = op[1] + max(rows, 1) * ls + 1, op[2] + max(rows, 1) * rs + 1
            if rows == 0 and i % 2:
                op[3], op[4] = 0, 3  # rows without bytes
            self.ops.append(op)
        self.lower_bound = sum(o[4] for o in self.ops if o[3] and o[4])

    def touched(self):
        return _plain_touched([(f, lo, ro, n, n) for f, lo, ro, n in strided_cases.expand(self.ops).tolist()],
                              self.local_bytes, self.remote_bytes)

    def run(self, a, async_=False):
        local, remote = fill_pair(a, self.local_bytes, self.remote_bytes, seed=3, random_remote=True)
        want_l, want_r = strided_cases.model(local, remote, self.ops)
        ops = api.strided_ops(np.asarray(self.ops, dtype=np.int64))
        err = _call(a, lambda: a.strided_batch(ops, async_=async_), async_)
        _compare(a, self, want_l, want_r)
        return 0, err


# ---- indexed ----
def index_specs(plan, seed):
    """What every op of a plan does with index arrays: direction, the arrays (None: that side is walked in
    order), the rows both tables say they have, and which tables are windows of a larger region."""
    rng = np.random.RandomState(seed)
    for i, (rows, c, tag) in enumerate(plan):
        if tag:
            s = SKIP_OPS[tag]
            lidx, ridx = s["lidx"], s["ridx"]
            n = len(lidx if lidx is not None else ridx)
            assert n == rows and all(-LEAD <= v < REGION - LEAD for v in (lidx or []) + (ridx or []))
            yield dict(put=s["put"], lidx=lidx, ridx=ridx, rows=n, cls=c, lrows=WIN if lidx is not None else n,
                       rrows=WIN if ridx is not None else n, lwin=lidx is not None, rwin=ridx is not None)
            continue
        n = max(rows, 1)
        tr = n + 3
        perm, other = rng.permutation(tr)[:n], rng.permutation(tr)[:n]
        lidx, ridx = (None, perm) if i % 3 == 0 else (perm, None) if i % 3 == 1 else (perm, other)
        yield dict(put=i % 2, lidx=lidx, ridx=ridx, rows=rows, cls=c, lrows=tr if lidx is not None else n,
                   rrows=tr if ridx is not None else n, lwin=False, rwin=False)


def _indexed_touched(case, plain, index_arrays, itype):
    t = _plain_touched(plain, case.local_bytes, case.remote_bytes)
    t["local_reads"] += [(off, off + len(vals) * 4 * itype) for off, vals in index_arrays]
    return t


class IndexedCase(Case):
    skips = True

    def __init__(self, waves, itype):
        self.kind = f"indexed_batch[{'int32' if itype == api.OCM_INDEX_I32 else 'int64'}]"
        self.itype = itype
        lay = self.lay = indexed_cases.Layout(itype)
        for i, s in enumerate(index_specs(row_plan(waves), seed=3)):
            rb = BYTES[s["cls"]][i % 3]
            ls, rs = rb + (0, 7)[i % 2], rb + (0, 13)[i % 2]
            li, ri = lay.index(s["lidx"]), lay.index(s["ridx"])
            loff = lay.table(REGION if s["lwin"] else s["lrows"], ls, rb, i % 16) + (LEAD * ls if s["lwin"] else 0)
            roff = lay.rtable(REGION if s["rwin"] else s["rrows"], rs, rb, (5 * i) % 16) + (LEAD * rs if s["rwin"] else 0)
            op = [s["put"], loff, roff, rb, s["rows"], ls, rs, li, ri, s["lrows"], s["rrows"]]
            if s["rows"] == 0 and i % 2:
                op[indexed_cases.RB], op[indexed_cases.NROWS] = 0, 1  # a row without bytes
            lay.ops.append(op)
        self.lower_bound = sum(o[4] for o in lay.ops if o[3] and o[4])

    local_bytes = property(lambda self: self.lay.local_bytes)
    remote_bytes = property(lambda self: self.lay.remote_bytes)

    def _local_image(self):
        local = np.zeros(self.local_bytes, dtype=np.uint8)
        for off, vals in self.lay.indices:
            raw = np.frombuffer(vals.tobytes(), dtype=np.uint8)
            local[off:off + len(raw)] = raw
        return local

    def touched(self):
        plain = indexed_cases.expand(self._local_image(), self.lay.ops, self.itype).tolist()
        return _indexed_touched(self, [(f, lo, ro, n, n) for f, lo, ro, n in plain], self.lay.indices, self.itype)

    def run(self, a, async_=False):
        return indexed_cases.run_layout(a, self.lay, seed=4, async_=async_)


# ---- converting kinds: the torch oracle over tables of rows ----
def _quant_word(dtype, fmt):
    return api.quant_dtype(dtype) | api.quant_format(fmt)


def fill_tables(local_bytes, remote_bytes, tables, seed):
    """Both halves before converting rows run, and every table's oracle results. tables: (put, format,
    dtype, row elements, local offsets, remote offsets), a row per offset; every row gets random elements
    of its own (puts) or the oracle record of such elements (gets), the sentinel lies everywhere else.
    Returns (local, remote, [(records, round trips) of a table's rows, or None for a table of nothing])."""
    local = np.full(local_bytes, SENTINEL, dtype=np.uint8)
    remote = np.full(remote_bytes, SENTINEL, dtype=np.uint8)
    refs = []
    for n, (put, fmt, dtype, re, loffs, roffs) in enumerate(tables):
        k = len(loffs) if put else len(roffs)
        if not k or not re:
            refs.append(None)
            continue
        x = random_elems(k * re, dtype, seed=seed * 1000 + n).view(k, re)
        rec, back = table_reference(x, fmt)
        raw = x.view(torch.uint8).numpy().reshape(k, 2 * re)
        for r in range(k):
            if put:
                local[loffs[r]:loffs[r] + 2 * re] = raw[r]
            else:
                remote[roffs[r]:roffs[r] + rec.shape[1]] = rec[r]
        refs.append((rec, back))
    return local, remote, refs


def convert_images(local_bytes, remote_bytes, tables, seed):
    """Both halves before and after converting rows that pair local offset r with remote offset r."""
    local, remote, refs = fill_tables(local_bytes, remote_bytes, tables, seed)
    want_l, want_r = local.copy(), remote.copy()
    for (put, fmt, dtype, re, loffs, roffs), ref in zip(tables, refs):
        if ref is None:
            continue
        rec, back = ref
        for r, (lo, ro) in enumerate(zip(loffs, roffs)):
            if put:
                want_r[ro:ro + rec.shape[1]] = rec[r]
            else:
                want_l[lo:lo + 2 * re] = back[r]
    return local, remote, want_l, want_r


class QuantCase(Case):
    kind = "quant"

    def __init__(self, waves):
        self.ops, self.fmts, self.dtypes = [], [], []  # [op_flag, local offset, remote offset, elems]
        self.lpos, self.rpos = 48, 32
        for i, c in enumerate(op_plan(waves, MULTI_FIXED_TILES)):
            n = QUANT_ELEMS[c] if c else 0
            fmt, dtype = FORMATS[(i >> 1) & 1], QUANT_DTYPES[(i >> 2) & 1]
            self.ops.append([i & 1, self.lpos, self.rpos, n])
            self.fmts.append(fmt)
            self.dtypes.append(dtype)
            self.lpos += 2 * n + 16 * (i % 2)
            self.rpos += record_up32(n, fmt) + 32 * (i % 3 == 0)
        self.lower_bound = sum(1 for o in self.ops if o[3])

    def _tables(self):
        groups = {}
        for (put, lo, ro, n), fmt, dtype in zip(self.ops, self.fmts, self.dtypes):
            g = groups.setdefault((put, fmt, dtype, n), ([], []))
            g[0].append(lo)
            g[1].append(ro)
        return [(put, fmt, dtype, n, ls, rs) for (put, fmt, dtype, n), (ls, rs) in groups.items()]

    def touched(self):
        return _plain_touched([(p, lo, ro, 2 * n, record_bytes(n, f)) for (p, lo, ro, n), f in zip(self.ops, self.fmts)],
                              self.local_bytes, self.remote_bytes)

    def run(self, a, async_=False):
        local, remote, want_l, want_r = convert_images(self.local_bytes, self.remote_bytes, self._tables(), seed=5)
        load_pair(a, local, remote)
        ops = api.quant_ops(np.asarray(self.ops, dtype=np.int64), QUANT_DTYPES[0], self.fmts)
        set_op_field(ops, "dt", [_quant_word(d, f) for d, f in zip(self.dtypes, self.fmts)])
        err = _call(a, lambda: a.quant_batch(ops, async_=async_), async_)
        _compare(a, self, want_l, want_r)
        return 0, err


class QuantStridedCase(Case):
    kind = "quant_strided"

    def __init__(self, waves):
        self.ops, self.fmts, self.dtypes = [], [], []  # [op_flag, lo, ro, row elems, rows, local stride, remote stride]
        self.lpos, self.rpos = 48, 32
        for i, (rows, c, _) in enumerate(row_plan(waves, MULTI_FIXED_TILES)):
            re = QUANT_ELEMS[c]
            fmt, dtype = FORMATS[(i >> 1) & 1], QUANT_DTYPES[(i >> 2) & 1]
            ls, rs = 2 * re + 16 * (i % 2), record_up32(re, fmt) + 32 * (i % 3)
            op = [i & 1, _up(self.lpos, 16), _up(self.rpos, 32), re, rows, ls, rs]
            self.lpos, self.rpos = op[1] + max(rows, 1) * ls + 16, op[2] + max(rows, 1) * rs + 32
            if rows == 0 and i % 2:
                op[3], op[4] = 0, 3  # rows without elements
            self.ops.append(op)
            self.fmts.append(fmt)
            self.dtypes.append(dtype)
        self.lower_bound = sum(o[4] for o in self.ops if o[3] and o[4])

    def _tables(self):
        return [(p, f, d, re, [lo + r * ls for r in range(rows)], [ro + r * rs for r in range(rows)])
                for (p, lo, ro, re, rows, ls, rs), f, d in zip(self.ops, self.fmts, self.dtypes)]

    def touched(self):
        rows = [(p, lo, ro, 2 * re, record_bytes(re, f)) for p, f, _, re, los, ros in self._tables() if re
                for lo, ro in zip(los, ros)]
        return _plain_touched(rows, self.local_bytes, self.remote_bytes)

    def run(self, a, async_=False):
        local, remote, want_l, want_r = convert_images(self.local_bytes, self.remote_bytes, self._tables(), seed=6)
        load_pair(a, local, remote)
        ops = api.quant_strided_ops(np.asarray(self.ops, dtype=np.int64), QUANT_DTYPES[0], self.fmts)
        set_op_field(ops, "dt", [_quant_word(d, f) for d, f in zip(self.dtypes, self.fmts)])
        err = _call(a, lambda: a.quant_strided_batch(ops, async_=async_), async_)
        _compare(a, self, want_l, want_r)
        return 0, err


class _QuantIndexedLayout(quant_indexed_cases.Layout):
    """The layout of quant_indexed_cases with an element type per op."""

    def __init__(self, itype):
        super().__init__(itype)
        self.dtypes = []

    def prepare(self, seed):
        """Both halves before and after the list, and the rows skipped: prepare() of quant_indexed_cases
        with self.dtypes[n] as op n's element type."""
        tables = []
        for o, fmt, dtype in zip(self.ops, self.formats, self.dtypes):
            flag, loff, roff, re, rows, ls, rs, li, ri, lrows, rrows = (int(v) for v in o)
            live = rows and re
            # every row of the table that is read holds data of its own: a wrong row shows
            tables.append((flag, fmt, dtype, re if live else 0, [loff + r * ls for r in range(lrows if flag else 0)],
                           [roff + r * rs for r in range(0 if flag else rrows)]))
        local, remote, refs = fill_tables(self.local_bytes, self.remote_bytes, tables, seed)
        for off, vals in self.indices:
            raw = np.frombuffer(vals.tobytes(), dtype=np.uint8)
            local[off:off + len(raw)] = raw
        want_l, want_r = local.copy(), remote.copy()
        plain, skipped = quant_indexed_cases.expand(local, self.ops, self.itype)
        for n, flag, lo, ro, re in plain:
            o, (rec, back) = self.ops[n], refs[n]
            if flag:
                want_r[ro:ro + rec.shape[1]] = rec[(lo - o[1]) // o[5]]
            else:
                want_l[lo:lo + 2 * re] = back[(ro - o[2]) // o[6]]
        return local, remote, want_l, want_r, skipped


class QuantIndexedCase(Case):
    kind = "quant_indexed"
    skips = True

    def __init__(self, waves, itype=api.OCM_INDEX_I32):
        self.itype = itype
        lay = self.lay = _QuantIndexedLayout(itype)
        for i, s in enumerate(index_specs(row_plan(waves, MULTI_FIXED_TILES), seed=7)):
            re = QUANT_ELEMS[s["cls"]]
            fmt, dtype = FORMATS[(i >> 1) & 1], QUANT_DTYPES[(i >> 2) & 1]
            ls, rs = 2 * re + 16 * (i % 2), record_up32(re, fmt) + 32 * (i % 3)
            li, ri = lay.index(s["lidx"]), lay.index(s["ridx"])
            loff, roff = _up(lay.lpos, 16), _up(lay.rpos, 32)
            lay.lpos = loff + (REGION if s["lwin"] else s["lrows"]) * ls + 16
            lay.rpos = roff + (REGION if s["rwin"] else s["rrows"]) * rs + 32
            op = [s["put"], loff + (LEAD * ls if s["lwin"] else 0), roff + (LEAD * rs if s["rwin"] else 0), re, s["rows"], ls, rs,
                  li, ri, s["lrows"], s["rrows"]]
            if s["rows"] == 0 and i % 2:
                op[3], op[4] = 0, 1  # a row without elements
            lay.ops.append(op)
            lay.formats.append(fmt)
            lay.dtypes.append(dtype)
        self.lower_bound = sum(o[4] for o in lay.ops if o[3] and o[4])

    local_bytes = property(lambda self: self.lay.local_bytes)
    remote_bytes = property(lambda self: self.lay.remote_bytes)

    def touched(self):
        local = IndexedCase._local_image(self)
        plain, _ = quant_indexed_cases.expand(local, self.lay.ops, self.itype)
        rows = [(f, lo, ro, 2 * re, record_bytes(re, self.lay.formats[n])) for n, f, lo, ro, re in plain]
        return _indexed_touched(self, rows, self.lay.indices, self.itype)

    def run(self, a, async_=False):
        lay = self.lay
        local, remote, want_l, want_r, skipped = lay.prepare(seed=8)
        load_pair(a, local, remote)
        ops = api.quant_indexed_ops(lay.ops, QUANT_DTYPES[0], lay.itype, lay.formats)
        set_op_field(ops, "dt", [_quant_word(d, f) for d, f in zip(lay.dtypes, lay.formats)])
        err = _call(a, lambda: a.quant_indexed_batch(ops, async_=async_), async_)
        _compare(a, self, want_l, want_r)
        return skipped, err


# ---- accumulate ----
class AccCase(Case):
    kind = "accumulate"

    def __init__(self, waves):
        self.ops = []  # (local offset, remote offset, elems, torch dtype, scale)
        self.lpos, self.rpos = 0, 16
        for i, c in enumerate(op_plan(waves, MULTI_FIXED_TILES)):
            n = ACC_ELEMS[c] if c else 0
            dtype, scale = acc_cases.DTYPES[i % 3], acc_cases.SCALES[(i // 3 + i) % len(acc_cases.SCALES)]
            self.ops.append((self.lpos, self.rpos, n, dtype, scale))
            self.lpos += _up(n * torch.empty((), dtype=dtype).element_size(), 16)
            self.rpos += 4 * n + 16 * (1 + i % 2)  # guard bytes between the accumulators
        assert all(a[3] != b[3] and a[4] != b[4] for a, b in zip(self.ops, self.ops[1:]))
        self.lower_bound = sum(1 for o in self.ops if o[2])

    def touched(self):
        t = dict(local_reads=[], local_writes=[], remote_reads=[], remote_writes=[])
        for lo, ro, n, dtype, _ in self.ops:
            t["local_reads"].append((lo, lo + n * torch.empty((), dtype=dtype).element_size()))
            t["remote_writes"].append((ro, ro + 4 * n))
        return t

    def run(self, a, async_=False):
        local = np.full(self.local_bytes, SENTINEL, dtype=np.uint8)
        remote = np.full(self.remote_bytes, acc_cases.GUARD, dtype=np.uint8)
        want_r = remote.copy()
        groups = {}
        for op in self.ops:
            if op[2]:
                groups.setdefault((op[3], op[4]), []).append(op)
        for g, ((dtype, scale), ops) in enumerate(groups.items()):
            total = sum(o[2] for o in ops)
            x = acc_cases.random_elems(total, dtype, seed=2000 + g)
            acc = acc_cases.random_elems(total, torch.float32, seed=3000 + g)
            res = accumulate_reference(acc, x, scale)  # elementwise: one call for the ops that share dtype and scale
            assert not torch.isnan(res).any()
            xb, ab, rb = (t.contiguous().view(torch.uint8).numpy() for t in (x, acc, res))
            es, at = x.element_size(), 0
            for lo, ro, n, _, _ in ops:
                local[lo:lo + n * es] = xb[at * es:(at + n) * es]
                remote[ro:ro + 4 * n] = ab[4 * at:4 * (at + n)]
                want_r[ro:ro + 4 * n] = rb[4 * at:4 * (at + n)]
                at += n
        load_pair(a, local, remote)
        arr = np.array([[lo, ro, n, api.acc_dtype(dt), s] for lo, ro, n, dt, s in self.ops], dtype=np.float64)
        ops = api.acc_ops(arr)
        err = _call(a, lambda: a.accumulate_batch(ops, async_=async_), async_)
        _compare(a, self, local, want_r)  # bit for bit, the guard bytes included; the local half unchanged
        return 0, err


# ---- bag ----
class BagCase(Case):
    kind = "bag_batch"
    skips = True

    def __init__(self, waves, itype=api.OCM_INDEX_I64):
        rng = np.random.RandomState(9)
        self.itype = itype
        lay = self.lay = bag_cases.Layout(itype, bag_cases.F32)
        self.dtypes, tables = [], {}
        for i, (rows, c, tag) in enumerate(row_plan(waves, MULTI_FIXED_TILES, BAG_SKIP_ROWS)):
            dtype = lay.dtype = bag_cases.DTYPES[i % 3]  # the layout's tables and ops take its current type
            mode = bag_cases.MEAN if i % 4 == 2 else bag_cases.SUM  # weights (odd ops) go with the sum only
            elems = BAG_ROW_BYTES[c] // bag_cases.ESIZE[dtype]
            if tag:
                region = lay.table(bag_cases.grid_values(rng, REGION, elems), gap=16)
                ids, offsets = BAG_SKIP_OPS[tag]
                assert all(-LEAD <= v < REGION - LEAD for v in ids) and len(offsets) - 1 == rows
                kw = dict(rows=WIN, off=region["off"] + LEAD * region["stride"])
                t, n_bags = region, None
            else:
                if (dtype, c) not in tables:
                    tables[dtype, c] = lay.table(bag_cases.grid_values(rng, 19, elems), gap=16 * (c - 1))
                t, kw, n_bags = tables[dtype, c], {}, (0 if rows == 0 else None)
                ids, offsets = bag_cases.ids_for(rng, [(1, 2, 0, 5, 1, 3)[(b + i) % 6] for b in range(max(rows, 1))], 19)
            w = rng.randint(-64, 65, len(ids)).astype(np.float32) / np.float32(48) if i % 2 else None
            lay.bag(t, ids, offsets, weights=w, mode=mode, out_gap=16 * (i % 2), bags=n_bags, **kw)
            self.dtypes.append(dtype)
        self.lower_bound = sum(o[bag_cases.BAGS] for o in lay.ops if o[bag_cases.RELEMS])

    local_bytes = property(lambda self: self.lay.local_bytes)
    remote_bytes = property(lambda self: self.lay.remote_bytes)

    def touched(self):
        t = dict(local_reads=[(off, off + len(raw)) for off, raw in self.lay.local_data], local_writes=[],
                 remote_reads=[(off, off + len(raw)) for off, raw in self.lay.remote_data], remote_writes=[])
        for o, dtype in zip(self.lay.ops, self.dtypes):
            rb = o[bag_cases.RELEMS] * bag_cases.ESIZE[dtype]
            t["local_writes"] += [(o[0] + b * o[bag_cases.LSTRIDE], o[0] + b * o[bag_cases.LSTRIDE] + rb) for b in range(o[bag_cases.BAGS])]
        return t

    def model(self, local, remote):
        """bag_cases.model op by op, each with its own element type (no op reads what another writes)."""
        want, skipped = local.copy(), 0
        for o, mode, dtype in zip(self.lay.ops, self.lay.modes, self.dtypes):
            res, n = bag_cases.model(local, remote, [o], [mode], self.itype, dtype)
            lo, hi = o[0], o[0] + o[bag_cases.BAGS] * o[bag_cases.LSTRIDE]
            want[lo:hi] = res[lo:hi]
            skipped += n
        return want, skipped

    def run(self, a, async_=False):
        lay = self.lay
        local, remote = lay.images(seed=10)
        bag_cases.fill(a, local, remote)
        want, skipped = self.model(local, remote)
        ops = api.bag_ops(lay.ops, bag_cases.F32, lay.itype, lay.modes)
        set_op_field(ops, "dt", self.dtypes)
        err = _call(a, lambda: a.bag_batch(ops, async_=async_), async_)
        _compare(a, self, want, remote)
        return skipped, err


BUILDERS = {
    "batch": BatchCase,
    "strided_batch": StridedCase,
    "indexed_batch-int32": lambda waves: IndexedCase(waves, api.OCM_INDEX_I32),
    "indexed_batch-int64": lambda waves: IndexedCase(waves, api.OCM_INDEX_I64),
    "quant": QuantCase,
    "quant_strided": QuantStridedCase,
    "quant_indexed": QuantIndexedCase,
    "accumulate": AccCase,
    "bag_batch": BagCase,
}


def check_skips(case, skipped, err, async_, before, after):
    """How a list reports the rows it skipped: the error's text and the counter, exactly the model's count."""
    if not case.skips:
        assert skipped == 0 and err is None, err
        return
    assert skipped > 0, "the list has out-of-range indices"
    assert isinstance(err, api.OcmError) and f"skipped {skipped} " in str(err), err
    assert ("ocm_wait" in str(err)) == async_
    assert after["n_indexed_skipped"] == before["n_indexed_skipped"] + skipped
