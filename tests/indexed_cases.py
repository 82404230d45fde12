"""Cases shared by the indexed-transfer tests (test_indexed_cpu.py, test_gpu_indexed.py): a numpy
model of ocm_copy_onesided_indexed with its skip rule, and case builders that never write a byte
another op of the list reads. Everything is compared byte for byte with the model."""
import numpy as np
import torch

from strided_cases import (ROW_BYTES, SENTINEL, UNIT, fill_pair, read_local, remote_bytes_of,  # noqa: F401  (re-exported)
                           write_local)

NONE = (1 << 64) - 1
# columns of an op row
FLAG, LOFF, ROFF, RB, NROWS, LSTRIDE, RSTRIDE, LIDX, RIDX, LROWS, RROWS = range(11)
NP_INDEX = {1: np.int32, 2: np.int64}
TORCH_INDEX = {1: torch.int32, 2: torch.int64}


def _up(x, m):
    return (x + m - 1) // m * m


def _index(arr, off, itype, rows):
    if off == NONE:
        return np.arange(rows, dtype=np.int64)
    size = 4 * itype
    return np.frombuffer(arr[off:off + rows * size].tobytes(), dtype=NP_INDEX[itype]).astype(np.int64)


def model(local, remote, ops, itype):
    """Both byte arrays after the ops, and the number of rows skipped. The index arrays are read from
    `local` as it was; puts read the local array as it was, gets the remote one."""
    lo, re = np.array(local, dtype=np.uint8), np.array(remote, dtype=np.uint8)
    skipped = 0
    for o in ops:
        flag, loff, roff, rb, rows, ls, rs, li, ri, lrows, rrows = (int(v) for v in o)
        if rows == 0 or rb == 0:
            continue
        lidx, ridx = _index(local, li, itype, rows), _index(local, ri, itype, rows)
        for j in range(rows):
            lr, rr = int(lidx[j]), int(ridx[j])
            if not (0 <= lr < lrows and 0 <= rr < rrows):  # unsigned compare: negatives are out of range
                skipped += 1
                continue
            a, b = loff + lr * ls, roff + rr * rs
            if flag:
                re[b:b + rb] = local[a:a + rb]
            else:
                lo[a:a + rb] = remote[b:b + rb]
    return lo, re, skipped


def expand(local, ops, itype):
    """The same transfer as Allocation.batch rows [op_flag, local_offset, remote_offset, bytes], one per
    in-range row, built on the host from the index arrays in `local`."""
    out = []
    for o in ops:
        flag, loff, roff, rb, rows, ls, rs, li, ri, lrows, rrows = (int(v) for v in o)
        if rows == 0 or rb == 0:
            continue
        lidx, ridx = _index(local, li, itype, rows), _index(local, ri, itype, rows)
        out += [[flag, loff + int(l) * ls, roff + int(r) * rs, rb] for l, r in zip(lidx, ridx)
                if 0 <= l < lrows and 0 <= r < rrows]
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def nominal(ops):
    """(rows named, nominal bytes) of the non-empty ops."""
    live = [o for o in ops if int(o[NROWS]) and int(o[RB])]
    return sum(int(o[NROWS]) for o in live), sum(int(o[NROWS]) * int(o[RB]) for o in live)


class Layout:
    """Lays ops and index arrays out in one pair so that no op writes what another reads: tables take
    fresh ranges of the local half (`table`) and of the remote half (`rtable`), index arrays fresh
    ranges of the local half (`index`), which no op ever writes."""

    def __init__(self, itype):
        self.itype = itype
        self.lpos, self.rpos = 0, 16
        self.ops, self.indices = [], []  # ops; (local offset, values) of every index array

    def table(self, rows, stride, rb, mod16):
        off = _up(self.lpos, 16) + mod16
        self.lpos = off + (rows - 1) * stride + rb + 1
        return off

    def rtable(self, rows, stride, rb, mod16):
        off = _up(self.rpos, 16) + mod16
        self.rpos = off + (rows - 1) * stride + rb + 1
        return off

    def index(self, values):
        if values is None:
            return NONE
        off = _up(self.lpos, 8)
        self.indices.append((off, np.asarray(values, dtype=NP_INDEX[self.itype])))
        self.lpos = off + len(values) * 4 * self.itype
        return off

    def op(self, put, rb, lidx, ridx, lrows, rrows, dense, lmod, rmod, remote_gap=0):
        rows = len(lidx if lidx is not None else ridx)
        ls = rb if dense else rb + 7
        rs = (rb if dense else rb + 13) + remote_gap
        li, ri = self.index(lidx), self.index(ridx)
        self.ops.append([int(put), self.table(lrows, ls, rb, lmod), self.rtable(rrows, rs, rb, rmod), rb, rows, ls, rs,
                         li, ri, lrows, rrows])
        return self.ops[-1]

    @property
    def local_bytes(self):
        return _up(self.lpos + 64, 4096)

    @property
    def remote_bytes(self):
        return max(_up(self.rpos + 64, UNIT), 4 * UNIT)  # at least a unit on each of three owners

    def install(self, a, local):
        """Writes the index arrays into the pair's local half and into the model's copy of it."""
        for off, vals in self.indices:
            raw = np.frombuffer(vals.tobytes(), dtype=np.uint8)
            local[off:off + len(raw)] = raw
            write_local(a, off, torch.from_numpy(raw.copy()))


def run_layout(a, lay, seed=1, async_=False, random_remote=True):
    """Runs the layout's ops as one list and compares every byte of both halves with the model.
    Returns the model's skip count (the caller checks how it was reported)."""
    local, remote = fill_pair(a, lay.local_bytes, lay.remote_bytes, seed, random_remote=random_remote)
    lay.install(a, local)
    want_l, want_r, skipped = model(local, remote, lay.ops, lay.itype)
    err = None
    try:
        a.indexed_batch(lay.ops, lay.itype, async_=async_)
        if async_:
            a.wait()
    except Exception as e:  # noqa: BLE001  (the caller sees it)
        err = e
    got_l = read_local(a, 0, lay.local_bytes).numpy()
    assert np.array_equal(got_l, want_l), f"local half: first bad bytes {np.flatnonzero(got_l != want_l)[:4]}"
    got_r = remote_bytes_of(a, lay.local_bytes, lay.remote_bytes)
    assert np.array_equal(got_r, want_r), f"remote half: first bad bytes {np.flatnonzero(got_r != want_r)[:4]}"
    return skipped, err


def index_sets(rows, table_rows, seed):
    """Index arrays of `rows` entries into a table of table_rows: a permutation's head, duplicates
    (with repeats of one row), all rows the same, and a reversed order."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(table_rows)[:rows]
    dup = rng.randint(0, table_rows, rows)
    if rows > 1:
        dup[-1] = dup[0]
    same = np.full(rows, table_rows - 1)
    rev = np.arange(table_rows)[::-1][:rows]
    return {"perm": perm, "dup": dup, "same": same, "rev": rev}


def edge_layout(itype, rb, rows, dense, agree, remote_gap=0, limit=960 << 10):
    """Ops of `rows` rows of rb bytes, in this order while both halves stay under `limit` bytes (the
    largest rows fit only the first few; the small ones carry every kind): a gather (remote index)
    with a permutation, a scatter with a permutation, both indices at once, gathers with duplicates,
    a local-index-only put, gathers of one row repeated and in reversed order, a local-index-only get.
    Tables have up to 64 rows. Destination indices are always duplicate-free."""
    lay = Layout(itype)
    lmod, rmod = (3, 3) if agree else (6, 8)
    tr = 64 if rb <= 255 else rows + 3
    sets = index_sets(rows, tr, seed=rb + rows)
    kinds = [(0, None, "perm", rows, tr), (1, None, "perm", rows, tr), (rb % 2, "rev", "perm", tr, tr),
             (0, None, "dup", rows, tr), (1, "dup", None, tr, rows), (0, None, "same", rows, tr),
             (0, None, "rev", rows, tr), (0, "rev", None, tr, rows)]
    for put, lname, rname, lrows, rrows in kinds:
        idx_bytes = 2 * 8 * rows + 64
        if (lay.lpos + lrows * (rb + 7) + idx_bytes + 4096 > limit or
                lay.rpos + rrows * (rb + 13 + remote_gap) + 4096 > limit) and lay.ops:
            break
        lay.op(put, rb, sets[lname] if lname else None, sets[rname] if rname else None, lrows, rrows, dense, lmod, rmod,
               remote_gap)
    return lay


def mixed_layout(itype, n_ops, seed=11):
    """n_ops mixed puts and gets, gathers, scatters and both-index ops, with a few empty ops (no rows,
    no bytes) first, last and in the middle."""
    rng = np.random.RandomState(seed)
    lay = Layout(itype)
    for i in range(n_ops):
        rb = int(rng.choice([1, 7, 16, 33, 255, 1024, 4097, 5000]))
        rows, tr = int(rng.choice([1, 2, 5])), int(rng.choice([5, 9, 17]))
        perm = rng.permutation(tr)[:rows]
        other = rng.permutation(tr)[:rows]
        kind = i % 4
        put = i % 3 != 0
        if kind == 0:
            o = lay.op(put, rb, None, perm, rows, tr, i % 2 == 0, i % 16, (5 * i) % 16)
        elif kind == 1:
            o = lay.op(put, rb, perm, None, tr, rows, i % 2 == 0, i % 16, (5 * i) % 16)
        else:
            o = lay.op(put, rb, perm, other, tr, tr, i % 2 == 0, i % 16, (5 * i) % 16)
        if i in (0, n_ops // 2, n_ops // 2 + 1, n_ops - 1):
            o[RB if i % 2 else NROWS] = 0  # an empty op: it keeps its ranges and moves nothing
    return lay


def exercise_indexed_kv(kv, rounds, seed, device):
    """The swap pattern and block model of test_kv_offload.py, with the ids in tensors on `device` and
    every swap one indexed op; odd rounds swap the same blocks in the list form and compare."""
    import random

    rng = random.Random(seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    pool_model = {}
    for r in range(rounds):
        fresh = torch.randn((kv.num_gpu_blocks, *kv.block_shape), generator=g).to(kv.dtype).to(device)
        kv.gpu_cache.copy_(fresh)  # written by torch on its stream; swap_out must see it
        k = rng.randint(1, min(kv.num_gpu_blocks, kv.indexed_ids))
        gpu_ids = rng.sample(range(kv.num_gpu_blocks), k)
        pool_ids = rng.sample(range(kv.num_pool_blocks), k)
        dt = torch.int64 if r % 2 else torch.int32  # any integer ids: the region holds int64
        assert kv.swap_out_indexed(torch.tensor(gpu_ids, dtype=dt, device=device),
                                   torch.tensor(pool_ids, dtype=dt, device=device), async_=bool(r % 3)) == 1
        for gi, pi in zip(gpu_ids, pool_ids):
            pool_model[pi] = fresh[gi].clone()
        kv.gpu_cache.zero_()
        known = list(pool_model)
        back = rng.sample(known, min(len(known), kv.num_gpu_blocks, kv.indexed_ids))
        dst = rng.sample(range(kv.num_gpu_blocks), len(back))
        kv.swap_in_indexed(torch.tensor(back, device=device), torch.tensor(dst, device=device), async_=bool(r % 2))
        # torch reads on its stream right away: swap_in_indexed made it wait for the copies
        for pi, gi in zip(back, dst):
            assert torch.equal(kv.gpu_cache[gi], pool_model[pi]), (r, pi, gi)
        if r % 2:  # the list form brings the same blocks
            got = kv.gpu_cache.clone()
            kv.gpu_cache.zero_()
            kv.swap_in(list(zip(back, dst)), async_=False)
            assert torch.equal(kv.gpu_cache, got), r
    kv.wait()
