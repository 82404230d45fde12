"""Cases shared by the indexed converting tests (test_quant_indexed_cpu.py,
test_gpu_quant_indexed.py): a model of ocm_copy_onesided_quant_indexed (the list expanded into
plain converting rows with the skip rule, the indices read from the local array, each row through
the torch oracle of its format) and a layout helper that never lets an op write what another
reads. Every table row holds data of its own, so a wrong row shows; everything is compared byte for
byte over both halves: records against the record reference, decoded rows against the oracle round
trip, and the sentinel in stride padding, in unpicked destination rows and everywhere else."""
import numpy as np
import torch

from indexed_cases import NONE, NP_INDEX, _index, index_sets  # noqa: F401  (re-exported)
from mx4_cases import FORMATS
from oncilla_amd import api
from oncilla_amd.ops import mx4_decode_reference, mx4_encode_reference, mx8_decode_reference, mx8_encode_reference
from quant_cases import UNIT, random_elems, read_local, write_local
from quant_strided_cases import load_pair
from strided_cases import SENTINEL, remote_bytes_of

ROW_ELEMS = (32, 1024, 1056, 2048, 2080, 4128)
DTYPES = (torch.bfloat16, torch.float16)
FORMAT_NAMES = ("mxfp8", "mxfp4")
# columns of an op row: those of indexed_cases with row_elems in place of row_bytes
FLAG, LOFF, ROFF, RE, NROWS, LSTRIDE, RSTRIDE, LIDX, RIDX, LROWS, RROWS = range(11)
_CODEC = {"mxfp8": (mx8_encode_reference, mx8_decode_reference), "mxfp4": (mx4_encode_reference, mx4_decode_reference)}


def _up(x, m):
    return (x + m - 1) // m * m


def record_bytes(re, fmt):
    return (re if fmt == "mxfp8" else re // 2) + re // 32


def record_up32(re, fmt):
    """A row's record rounded up to the 32 bytes the next record must start on."""
    return _up(record_bytes(re, fmt), 32)


def table_reference(x2d, fmt):
    """(records [rows, record bytes] uint8, round trips [rows, 2 * row_elems] uint8) of a table of
    rows, through the torch oracle of `fmt`. Groups of 32 never span rows, so the whole table is
    encoded at once and cut into one record per row: its codes, then its scale bytes."""
    rows, re = x2d.shape
    enc, dec = _CODEC[fmt]
    codes, scales = enc(x2d.reshape(-1))
    rec = torch.cat([codes.view(rows, -1), scales.view(rows, -1)], dim=1)
    assert rec.shape[1] == record_bytes(re, fmt)
    back = dec(codes, scales, x2d.dtype).view(rows, re)
    return rec.numpy(), back.contiguous().view(torch.uint8).numpy().reshape(rows, 2 * re)


def expand(local, ops, itype):
    """The model of the call: (plain converting rows [op number, op_flag, local_offset, remote_offset,
    elems], one per in-range row, and the number of rows skipped), the index arrays read from the
    byte array `local`. Indices are compared as unsigned: negative ones are out of range."""
    out, skipped = [], 0
    for n, o in enumerate(ops):
        flag, loff, roff, re, rows, ls, rs, li, ri, lrows, rrows = (int(v) for v in o)
        if rows == 0 or re == 0:
            continue
        lidx, ridx = _index(local, li, itype, rows), _index(local, ri, itype, rows)
        for lr, rr in zip(lidx.tolist(), ridx.tolist()):
            if 0 <= lr < lrows and 0 <= rr < rrows:
                out.append([n, flag, loff + lr * ls, roff + rr * rs, re])
            else:
                skipped += 1
    return out, skipped


def nominal(ops, formats):
    """(rows named, 16-bit source bytes, record bytes) of the non-empty ops: every named row counts."""
    live = [(o, f) for o, f in zip(ops, formats) if int(o[NROWS]) and int(o[RE])]
    return (sum(int(o[NROWS]) for o, _ in live), sum(int(o[NROWS]) * 2 * int(o[RE]) for o, _ in live),
            sum(int(o[NROWS]) * record_bytes(int(o[RE]), f) for o, f in live))


class Layout:
    """Lays ops and index arrays out in one pair so that no op writes what another reads: tables take
    fresh ranges of the local half and of the remote half, index arrays fresh ranges of the local
    half, which no op ever writes. `formats` has the record format of every op."""

    def __init__(self, itype):
        self.itype = itype
        self.lpos, self.rpos = 48, 32
        self.ops, self.formats, self.indices = [], [], []  # ops; their formats; (local offset, values) of every index array

    def index(self, values):
        if values is None:
            return NONE
        off = _up(self.lpos, 8)
        self.indices.append((off, np.asarray(values, dtype=NP_INDEX[self.itype])))
        self.lpos = off + len(values) * 4 * self.itype
        return off

    def op(self, put, fmt, re, lidx, ridx, lrows, rrows, lpad=0, rpad=0, rows=None, at=None):
        """One op: `lidx` / `ridx` index arrays (None: that side has no index) into tables of lrows /
        rrows rows; lpad / rpad: bytes between rows beyond the dense strides; rows: the op's row count
        where it is not the arrays' length (an empty op); at: a fixed remote offset for the table."""
        rows = len(lidx if lidx is not None else ridx) if rows is None else rows
        ls, rs = 2 * re + lpad, record_up32(re, fmt) + rpad
        li, ri = self.index(lidx), self.index(ridx)
        loff = _up(self.lpos, 16)
        self.lpos = loff + max(lrows - 1, 0) * ls + 2 * re + 16
        if at is None:
            roff = _up(self.rpos, 32)
            self.rpos = roff + max(rrows - 1, 0) * rs + record_bytes(re, fmt) + 32
        else:
            roff = at
        self.ops.append([int(put), loff, roff, re, rows, ls, rs, li, ri, lrows, rrows])
        self.formats.append(fmt)
        return self.ops[-1]

    @property
    def local_bytes(self):
        return _up(self.lpos + 64, 4096)

    @property
    def remote_bytes(self):
        return max(_up(self.rpos + 64, UNIT), 4 * UNIT)  # at least a unit on each of three owners

    def prepare(self, dtype, seed):
        """Both halves before and after the list: (local, remote, want_local, want_remote, skipped).
        The sentinel everywhere; the index arrays; every row of a table a put reads holds random
        elements of its own, every row of a table a get reads the oracle record of such elements."""
        local = np.full(self.local_bytes, SENTINEL, dtype=np.uint8)
        remote = np.full(self.remote_bytes, SENTINEL, dtype=np.uint8)
        for off, vals in self.indices:
            raw = np.frombuffer(vals.tobytes(), dtype=np.uint8)
            local[off:off + len(raw)] = raw
        refs = []
        for n, (o, fmt) in enumerate(zip(self.ops, self.formats)):
            flag, loff, roff, re, rows, ls, rs, li, ri, lrows, rrows = (int(v) for v in o)
            if rows == 0 or re == 0:
                refs.append(None)
                continue
            trows = lrows if flag else rrows  # the table that is read
            x = random_elems(trows * re, dtype, seed=seed * 1000 + n).view(trows, re)
            rec, back = table_reference(x, fmt)
            refs.append((rec, back))
            raw = x.view(torch.uint8).numpy().reshape(trows, 2 * re)
            for r in range(trows):
                if flag:
                    local[loff + r * ls: loff + r * ls + 2 * re] = raw[r]
                else:
                    remote[roff + r * rs: roff + r * rs + rec.shape[1]] = rec[r]
        want_l, want_r = local.copy(), remote.copy()
        plain, skipped = expand(local, self.ops, self.itype)
        for n, flag, lo, ro, re in plain:
            o, (rec, back) = self.ops[n], refs[n]
            if flag:
                r = (lo - o[LOFF]) // o[LSTRIDE]
                want_r[ro:ro + rec.shape[1]] = rec[r]
            else:
                r = (ro - o[ROFF]) // o[RSTRIDE]
                want_l[lo:lo + 2 * re] = back[r]
        return local, remote, want_l, want_r, skipped

    def plain_ops(self, local):
        """The same transfer as Allocation.quant_batch rows [op_flag, local_offset, remote_offset, elems]
        with one format per row: what the call is defined as."""
        plain, _ = expand(local, self.ops, self.itype)
        return np.asarray([p[1:] for p in plain], dtype=np.int64).reshape(-1, 4), [self.formats[p[0]] for p in plain]


def _first_bad(got, want):
    return np.flatnonzero(got != want)[:4].tolist()


def run_layout(a, lay, dtype, seed=1, async_=False, run=None):
    """Prepares both halves, runs the layout's ops as one list (or `run(local)` in its place) and
    compares every byte of both halves with the model. Returns (the model's skip count, the error
    the call or its wait raised, both halves)."""
    local, remote, want_l, want_r, skipped = lay.prepare(dtype, seed)
    load_pair(a, local, remote)
    err = None
    try:
        if run is not None:
            run(local)
        else:
            a.quant_indexed_batch(api.quant_indexed_ops(lay.ops, dtype, lay.itype, lay.formats), async_=async_)
            if async_:
                a.wait()
    except Exception as e:  # noqa: BLE001  (the caller sees it)
        err = e
    got_l = read_local(a, 0, lay.local_bytes).numpy()
    got_r = remote_bytes_of(a, lay.local_bytes, lay.remote_bytes)
    assert np.array_equal(got_r, want_r), f"remote half: first bad bytes {_first_bad(got_r, want_r)}"
    assert np.array_equal(got_l, want_l), f"local half: first bad bytes {_first_bad(got_l, want_l)}"
    return skipped, err, (got_l, got_r)


# (put, local index, remote index) of the kinds an edge layout carries, by name in index_sets; the
# side being written never has duplicates
KINDS = ((0, None, "perm"), (0, None, "dup"), (0, None, "same"), (0, None, "rev"),  # gathers
         (1, None, "perm"),                                                        # a scatter
         (0, "rev", "perm"), (1, "perm", "rev"),                                   # both indices at once
         (1, "dup", None), (0, "rev", None))                                       # local-index-only put and get


def edge_layouts(itype, fmt, re, rows, lpad, rpad, limit=960 << 10):
    """Layouts that between them carry every kind of KINDS for rows of `re` elements, `rows` rows an
    op, each layout with both halves under `limit` bytes. Tables have rows + 3 rows."""
    tr = rows + 3
    sets = index_sets(rows, tr, seed=re + rows)
    lays = [Layout(itype)]
    for put, lname, rname in KINDS:
        # a side without an index is walked in order: rows 0 .. rows - 1 of a table of `rows` rows
        lrows, rrows = (tr if lname else rows), (tr if rname else rows)
        lay = lays[-1]
        need_l = lrows * (2 * re + lpad) + 2 * 8 * rows + 256
        need_r = rrows * (record_up32(re, fmt) + rpad) + 256
        if lay.ops and (lay.lpos + need_l + 4096 > limit or lay.rpos + need_r + 4096 > limit):
            lay = Layout(itype)
            lays.append(lay)
        lay.op(put, fmt, re, sets[lname] if lname else None, sets[rname] if rname else None, lrows, rrows, lpad, rpad)
    assert all(L.local_bytes <= 1 << 20 and L.remote_bytes <= 1 << 20 for L in lays)
    return lays


def mixed_layout(itype, n_ops, seed=11):
    """n_ops mixed puts and gets of both formats, gathers, scatters and both-index ops, with empty ops
    (no rows, or no elements) first, last and two adjacent in the middle."""
    rng = np.random.RandomState(seed)
    lay = Layout(itype)
    empty = (0, n_ops // 2, n_ops // 2 + 1, n_ops - 1)
    for i in range(n_ops):
        re = int(rng.choice([32, 64, 96, 1024, 1056, 2080]))
        rows, tr = int(rng.choice([1, 2, 5])), int(rng.choice([5, 9]))
        perm, other = rng.permutation(tr)[:rows], rng.permutation(tr)[:rows]
        fmt = FORMAT_NAMES[(i // 2) % 2]
        put = i % 3 != 0
        pads = (16 * (i % 2), 32 * (i % 4))
        if i % 4 == 0:
            o = lay.op(put, fmt, re, None, perm, rows, tr, *pads)
        elif i % 4 == 1:
            o = lay.op(put, fmt, re, perm, None, tr, rows, *pads)
        else:
            o = lay.op(put, fmt, re, perm, other, tr, tr, *pads)
        if i in empty:
            o[RE if i % 2 else NROWS] = 0  # an empty op: it keeps its ranges and moves nothing
    live = [(o[FLAG], f) for o, f in zip(lay.ops, lay.formats) if o[RE] and o[NROWS]]
    assert {(p, f) for p, f in live} == {(p, f) for p in (0, 1) for f in FORMAT_NAMES}
    return lay


def embedding_reference(table, fmt):
    """What a lookup of a compressed RemoteEmbedding returns for every row: the oracle decode of the
    oracle encode of the loaded rows, [num_rows, dim] in the table's dtype."""
    _, roundtrip = FORMATS[fmt]
    return roundtrip(table.reshape(-1)).view(table.shape)
