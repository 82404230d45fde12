"""Cases shared by the strided converting tests (test_quant_strided_cpu.py,
test_gpu_quant_strided.py): the grid of row sizes, row counts and strides, a model of
ocm_copy_onesided_quant_strided (the list expanded into plain converting rows, each row
through the torch oracle), and a helper that compares every byte of both halves, so the
bytes between rows keep their sentinel. Everything is compared byte for byte: records
against mx8_record_reference, decoded rows against roundtrip."""
import random

import numpy as np
import torch

from oncilla_amd import api
from oncilla_amd.ops import mx8_record_reference
from quant_cases import UNIT, random_elems, read_local, roundtrip, write_local, write_remote
from strided_cases import SENTINEL, remote_bytes_of

# one group; one round exactly; a round plus a group; one tile exactly; a tile plus a group;
# two tiles plus a group
ROW_ELEMS = (32, 1024, 1056, 2048, 2080, 4128)
ROWS = (1, 2, 5)
# (local stride, remote stride) of a row of `re` elements
LOCAL_STRIDES = {"dense": lambda re: 2 * re, "pad16": lambda re: 2 * re + 16, "cache": lambda re: 3 * 2 * re}
REMOTE_STRIDES = {"dense": lambda re: record_up32(re), "pad32": lambda re: record_up32(re) + 32,
                  "pad96": lambda re: record_up32(re) + 96}
STRIDES = (("dense", "dense"), ("pad16", "pad32"), ("cache", "pad96"))
DTYPES = (torch.bfloat16, torch.float16)
# columns of an op row
FLAG, LOFF, ROFF, RE, NROWS, LSTRIDE, RSTRIDE = range(7)


def record_up32(re):
    """A row's record rounded up to the 32 bytes the next record must start on."""
    return (re + re // 32 + 31) // 32 * 32


def _up(x, m):
    return (x + m - 1) // m * m


def expand(ops):
    """The model of the call: the same transfer as Allocation.quant_batch rows
    [op_flag, local_offset, remote_offset, elems], one per row."""
    out = []
    for flag, loff, roff, re, rows, ls, rs in np.asarray(ops, dtype=np.int64).reshape(-1, 7):
        if re:
            out += [[flag, loff + r * ls, roff + r * rs, re] for r in range(rows)]
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def src_wire_bytes(ops):
    rows = expand(ops)
    return int(2 * rows[:, 3].sum()), int((rows[:, 3] + rows[:, 3] // 32).sum())


class Case:
    """A list of ops over one pair whose destinations are disjoint and never another op's source.
    prepare() fills both halves: the sentinel everywhere, random elements where puts read, oracle
    records of random elements where gets read; and gives both halves as they must be afterwards."""

    def __init__(self, ops, local_bytes, remote_bytes):
        self.ops = np.asarray(ops, dtype=np.int64).reshape(-1, 7)
        self.local_bytes, self.remote_bytes = local_bytes, remote_bytes

    def prepare(self, dtype, seed):
        local = np.full(self.local_bytes, SENTINEL, dtype=np.uint8)
        remote = np.full(self.remote_bytes, SENTINEL, dtype=np.uint8)
        want_l, want_r = local.copy(), remote.copy()
        for i, (flag, lo, ro, n) in enumerate(expand(self.ops).tolist()):
            x = random_elems(n, dtype, seed=seed * 1000 + i)
            rec = mx8_record_reference(x).numpy()
            if flag:
                local[lo:lo + 2 * n] = want_l[lo:lo + 2 * n] = x.view(torch.uint8).numpy()
                want_r[ro:ro + len(rec)] = rec
            else:
                remote[ro:ro + len(rec)] = want_r[ro:ro + len(rec)] = rec
                want_l[lo:lo + 2 * n] = roundtrip(x).view(torch.uint8).numpy()
        return local, remote, want_l, want_r


def load_pair(a, local, remote):
    """Both halves of `a` from numpy arrays (the remote one with plain puts staged in the local half)."""
    chunk = min(len(local), len(remote))
    for off in range(0, len(remote), chunk):
        write_remote(a, 0, off, torch.from_numpy(remote[off:off + chunk].copy()))
    write_local(a, 0, torch.from_numpy(local.copy()))


def halves(a, case):
    return read_local(a, 0, case.local_bytes).numpy(), remote_bytes_of(a, case.local_bytes, case.remote_bytes)


def _first_bad(got, want):
    return np.flatnonzero(got != want)[:4].tolist()


def run_case(a, case, dtype, seed=1, run=None):
    """Prepare, run the list on `a`, and compare every byte of both halves: the records, the
    decoded rows, and the sentinel everywhere else. Returns both halves."""
    local, remote, want_l, want_r = case.prepare(dtype, seed)
    load_pair(a, local, remote)
    (run or (lambda ops: a.quant_strided_batch(ops, dtype)))(case.ops)
    got_l, got_r = halves(a, case)
    assert np.array_equal(got_r, want_r), f"remote half: first bad bytes {_first_bad(got_r, want_r)}"
    assert np.array_equal(got_l, want_l), f"local half: first bad bytes {_first_bad(got_l, want_l)}"
    return got_l, got_r


def edge_case(rows, lmode, rmode):
    """One put and one get per row size of ROW_ELEMS, `rows` rows each, in one list. The puts of
    1024 and 2048 elements lie so that row 0's codes (remote offset 2 * UNIT - 64) and row 0's
    scale bytes (5 * UNIT - 2080: they start 32 bytes before a unit boundary) cross a stripe
    unit; everything else is packed behind 8 * UNIT."""
    fixed = {1024: 2 * UNIT - 64, 2048: 5 * UNIT - 2080}
    ops = []
    loff, roff = 48, 8 * UNIT
    for flag in (1, 0):
        for re in ROW_ELEMS:
            ls, rs = LOCAL_STRIDES[lmode](re), REMOTE_STRIDES[rmode](re)
            if flag and re in fixed:
                ro = fixed[re]
                assert ro + rows * rs <= (8 * UNIT if re == 2048 else fixed[2048])
            else:
                ro, roff = roff, roff + rows * rs + 32 * (re // 32 % 3)
            ops.append([flag, loff, ro, re, rows, ls, rs])
            loff = _up(loff + rows * ls, 16) + 16 * (re // 32 % 2)
    case = Case(ops, _up(loff + 64, 4096), _up(roff + 64, UNIT))
    assert (fixed[1024] + 1024) // UNIT != fixed[1024] // UNIT                  # row 0's codes on two units
    assert (fixed[2048] + 2048) // UNIT != (fixed[2048] + 2048 + 63) // UNIT    # row 0's scale bytes too
    return case


def list_case(n_ops, seed=5):
    """n_ops mixed puts and gets on disjoint slots: 1 to 3 rows of 32 to 2080 elements, padded and
    dense strides; ops without elements first, last and two in a row, one of them without rows."""
    rng = random.Random(seed)
    sizes = (32, 96, 1024, 2080, 64, 1056, 2048, 160)
    lslot, rslot = 3 * (2 * 2080 + 16) + 64, 3 * (record_up32(2080) + 96) + 96
    ops = []
    for i in range(n_ops):
        re = 0 if i in (0, 7, 8, n_ops - 1) else sizes[i % len(sizes)]
        rows = 1 + i % 3
        ls = 2 * re + 16 * rng.choice([0, 1])
        rs = record_up32(re) + 32 * rng.choice([0, 1, 3])
        ops.append([i % 3 != 1, i * lslot + 16 * (i % 4), _up(i * rslot, 32) + 32 * (i % 3), re, rows, ls, rs])
    ops[8][NROWS] = 0
    ops[7][RE], ops[7][NROWS] = 64, 0  # rows == 0 with a row size kept
    assert {o[FLAG] for o in ops if o[RE] and o[NROWS]} == {0, 1}
    return Case(ops, _up(n_ops * lslot, 4096), _up(n_ops * rslot + 64, UNIT))


def exercise_layered_quant_kv(kv, rounds, seed, device):
    """The swap pattern of test_kv_offload.py on a layered cache [L, blocks, ...] whose pool holds
    one record per layer: what comes back is, per layer, the oracle decode of the oracle encode."""
    rng = random.Random(seed)
    g = torch.Generator(device="cpu").manual_seed(seed)
    pool_model = {}
    L = kv.layers
    for r in range(rounds):
        fresh = torch.randn((L, kv.num_gpu_blocks, *kv.block_shape), generator=g).to(kv.dtype)
        kv.gpu_cache.copy_(fresh.to(device))  # written by torch on its stream; swap_out must see it
        k = rng.randint(1, kv.num_gpu_blocks)
        gpu_ids = rng.sample(range(kv.num_gpu_blocks), k)
        pool_ids = rng.sample(range(kv.num_pool_blocks), k)
        assert kv.swap_out(list(zip(gpu_ids, pool_ids)), async_=bool(r % 3)) == k  # one op per block
        for gi, pi in zip(gpu_ids, pool_ids):
            pool_model[pi] = torch.stack([roundtrip(fresh[layer, gi]) for layer in range(L)])
        kv.gpu_cache.zero_()  # overwrite the GPU blocks
        known = list(pool_model)
        back = rng.sample(known, min(len(known), kv.num_gpu_blocks))
        dst = rng.sample(range(kv.num_gpu_blocks), len(back))  # other GPU blocks
        kv.swap_in(list(zip(back, dst)), async_=bool(r % 2))
        # torch reads on its stream right away: swap_in made it wait for the copies
        got = kv.gpu_cache.cpu()
        for pi, gi in zip(back, dst):
            assert torch.equal(got[:, gi].view(torch.int16), pool_model[pi].view(torch.int16)), (r, pi, gi)
    kv.wait()
