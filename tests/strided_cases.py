"""Cases shared by the strided-transfer tests (test_strided_cpu.py, test_gpu_strided.py):
a numpy model of ocm_copy_onesided_strided, case builders that write only to disjoint
destinations, and helpers that move raw bytes through an allocation. Everything is
compared byte for byte with the model."""
import random

import numpy as np
import torch

from quant_cases import UNIT, read_local, read_remote, write_local, write_remote  # noqa: F401  (re-exported)

SENTINEL = 0xA5
ROW_BYTES = (1, 15, 16, 17, 4095, 4096, 4097, 8195)
ROWS = (1, 2, 5)
# columns of an op row
FLAG, LOFF, ROFF, RB, NROWS, LSTRIDE, RSTRIDE = range(7)


def model(local, remote, ops):
    """Both byte arrays after the ops (puts read the local array as it was, gets the remote one:
    the builders here never write what another op of the list reads)."""
    lo, re = np.array(local, dtype=np.uint8), np.array(remote, dtype=np.uint8)
    for flag, loff, roff, rb, rows, ls, rs in np.asarray(ops, dtype=np.int64).reshape(-1, 7):
        for r in range(rows):
            a, b = loff + r * ls, roff + r * rs
            if flag:
                re[b:b + rb] = local[a:a + rb]
            else:
                lo[a:a + rb] = remote[b:b + rb]
    return lo, re


def expand(ops):
    """The same transfer as Allocation.batch rows [op_flag, local_offset, remote_offset, bytes], one per row."""
    out = []
    for flag, loff, roff, rb, rows, ls, rs in np.asarray(ops, dtype=np.int64).reshape(-1, 7):
        out += [[flag, loff + r * ls, roff + r * rs, rb] for r in range(rows)]
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def moved_bytes(ops):
    o = np.asarray(ops, dtype=np.int64).reshape(-1, 7)
    return int((o[:, RB] * o[:, NROWS]).sum())


def _up(x, m):
    return (x + m - 1) // m * m


class Case:
    """A put list and a get list over one pair: the puts take rows out of local [0, half) into the
    remote half, the gets bring the same rows back into local [half, 2 * half) at other offsets."""

    def __init__(self, puts, gets, half, remote_bytes):
        self.puts = np.asarray(puts, dtype=np.int64).reshape(-1, 7)
        self.gets = np.asarray(gets, dtype=np.int64).reshape(-1, 7)
        self.half = half
        self.local_bytes = 2 * half
        self.remote_bytes = remote_bytes


def edge_case(rows, dense, agree, remote_gap=0):
    """One put and one get per row size of ROW_BYTES, `rows` rows each. dense: strides == row_bytes,
    else padded by an odd amount. agree: local and remote offsets equal mod 16, else they differ.
    remote_gap: extra bytes between remote rows (test_rows_across_stripe_units)."""
    puts, gets = [], []
    loff, roff, goff = 3, 16 + (3 if agree else 8), 19 if agree else 6
    for rb in ROW_BYTES:
        ls = rb if dense else rb + 7
        rs = (rb if dense else rb + 13) + remote_gap
        gs = rb if dense else rb + 3
        puts.append([1, loff, roff, rb, rows, ls, rs])
        gets.append([0, goff, roff, rb, rows, gs, rs])
        # the next op: past this one's last row, at the same offset mod 16 on every side
        loff = _up(loff + rows * ls, 16) + 3
        goff = _up(goff + rows * gs, 16) + (19 if agree else 6)
        roff = _up(roff + rows * rs, 16) + (3 if agree else 8)
    half = _up(max(loff, goff) + 64, 4096)
    for g in gets:
        g[LOFF] += half
    return Case(puts, gets, half, _up(roff + 64, UNIT))


def mixed_list(n=70, seed=17):
    """n mixed puts and gets with disjoint destinations (more ops than travel in the kernel
    arguments): op i owns local [i * slot, +slot) and remote [i * rslot, +rslot); row sizes from 1
    byte to over two wave-tiles, 1 to 6 rows, odd paddings, a few empty ops."""
    rng = random.Random(seed)
    slot, rslot = 12288, 12288 + 512
    ops = []
    for i in range(n):
        rows = rng.choice([1, 2, 3, 6])
        rb = rng.choice([1, 7, 16, 33, 255, 1024, 2048, 4097, 9000]) if i % 9 else 0
        rb = min(rb, (slot - 64) // rows - 8)
        ls, rs = rb + rng.choice([0, 1, 5]), rb + rng.choice([0, 3, 16])
        ops.append([i % 3 != 0, i * slot + rng.randrange(0, 16), i * rslot + rng.randrange(0, 32), rb, rows, ls, rs])
    ops[5][NROWS] = 0  # an op without rows, its row size kept
    return np.asarray(ops, dtype=np.int64), n * slot, _up(n * rslot, UNIT)


def fill_pair(a, local_bytes, remote_bytes, seed, random_remote=False):
    """Random local bytes in `a`; the remote half holds the sentinel, or random bytes too. Written
    with plain puts staged in the local half. Returns both halves as numpy arrays."""
    g = torch.Generator().manual_seed(seed)
    local = torch.randint(0, 256, (local_bytes,), dtype=torch.uint8, generator=g)
    if random_remote:
        remote = torch.randint(0, 256, (remote_bytes,), dtype=torch.uint8, generator=g)
    else:
        remote = torch.full((remote_bytes,), SENTINEL, dtype=torch.uint8)
    chunk = min(local_bytes, remote_bytes)
    for off in range(0, remote_bytes, chunk):
        write_remote(a, 0, off, remote[off:off + chunk])
    write_local(a, 0, local)
    return local.numpy().copy(), remote.numpy().copy()


def remote_bytes_of(a, local_bytes, remote_bytes):
    """The whole remote half, read with plain gets through the local half (which is put back)."""
    keep = read_local(a, 0, local_bytes)
    chunk = min(local_bytes, remote_bytes)
    out = []
    for off in range(0, remote_bytes, chunk):
        n = min(chunk, remote_bytes - off)
        out.append(read_remote(a, 0, off, n))
    write_local(a, 0, keep)
    return torch.cat(out).numpy()


def run_case(a, case, seed=1, run=None):
    """Puts, then gets into the second local region, each checked against the model over every
    byte of both halves (the bytes outside the rows keep the sentinel / their old value)."""
    run = run or (lambda ops: a.strided_batch(ops))
    local, remote = fill_pair(a, case.local_bytes, case.remote_bytes, seed)
    local[case.half:] = SENTINEL
    write_local(a, case.half, torch.full((case.half,), SENTINEL, dtype=torch.uint8))
    run(case.puts)
    want_l, want_r = model(local, remote, case.puts)
    assert np.array_equal(remote_bytes_of(a, case.local_bytes, case.remote_bytes), want_r), "remote half after the puts"
    assert np.array_equal(read_local(a, 0, case.local_bytes).numpy(), want_l), "local half after the puts"
    run(case.gets)
    want_l2, want_r2 = model(want_l, want_r, case.gets)
    got_l = read_local(a, 0, case.local_bytes).numpy()
    assert np.array_equal(got_l, want_l2), f"local half after the gets: first bad byte {np.flatnonzero(got_l != want_l2)[:4]}"
    assert np.array_equal(remote_bytes_of(a, case.local_bytes, case.remote_bytes), want_r2), "remote half after the gets"
    # what came back is what went out
    for p, g in zip(case.puts, case.gets):
        for r in range(p[NROWS]):
            s, d = p[LOFF] + r * p[LSTRIDE], g[LOFF] + r * g[LSTRIDE]
            assert np.array_equal(got_l[d:d + p[RB]], local[s:s + p[RB]])


def exercise_layered_kv(kv, rounds, seed, device):
    """The swap pattern of test_kv_offload.py on a layered cache [L, blocks, ...]: exact, per layer."""
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
            pool_model[pi] = fresh[:, gi].clone()
        kv.gpu_cache.zero_()  # overwrite the GPU blocks
        known = list(pool_model)
        back = rng.sample(known, min(len(known), kv.num_gpu_blocks))
        dst = rng.sample(range(kv.num_gpu_blocks), len(back))  # other GPU blocks
        kv.swap_in(list(zip(back, dst)), async_=bool(r % 2))
        # torch reads on its stream right away: swap_in made it wait for the copies
        for pi, gi in zip(back, dst):
            for layer in range(L):
                assert torch.equal(kv.gpu_cache[layer, gi].cpu().view(torch.int16),
                                   pool_model[pi][layer].view(torch.int16)), (r, pi, gi, layer)
    kv.wait()
