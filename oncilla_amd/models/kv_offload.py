"""Paged KV-cache offload onto disaggregated memory (a serving workload).

LLM serving keeps the KV cache in fixed-size blocks on the GPU. When memory runs
short, blocks of idle sequences are swapped out to a larger pool and swapped back
in before their next step. The usual implementation issues one memcpy per block.
Here the GPU cache is the *local half* of one oncilla remote pair, and the
offload pool is its *remote half*. The pool can be HBM striped over the node's
other MI355X (xGMI), the pinned host tier, or another node. A whole swap list
becomes ONE batched one-sided launch (ocm_copy_onesided_batch), with runs of
consecutive blocks coalesced into single ops.

With ``compress="mxfp8"`` the pool holds MXFP8 records (e4m3fn codes and one
power-of-two scale byte per 32 elements, ``oncilla_amd.ops.mx8_encode_reference``):
a block takes 33/64 of its bytes in the pool and on the link, converted as it is
copied (ocm_copy_onesided_quant), and comes back rounded to that format.

With ``layers=L`` the GPU cache has the layout serving engines use, one cache per
layer: ``[L, num_gpu_blocks, *block_shape]``. A logical block is then L pieces of
block_bytes, num_gpu_blocks * block_bytes apart; in the pool it is L * block_bytes
contiguous bytes, layer-major. Each swapped block is one strided op
(ocm_copy_onesided_strided, rows = L) and the whole list still one launch.

``layers=L`` with ``compress="mxfp8-rows"`` combines the two: a pool block is L MXFP8
records side by side, layer-major, one per layer, each rounded up to 32 bytes. Each
swapped block is one strided converting op (ocm_copy_onesided_quant_strided, rows = L,
local stride num_gpu_blocks * block_bytes, remote stride the rounded record), the whole
list one launch, and every layer comes back rounded to the format on its own.
(``compress="mxfp8"`` keeps one record per block and cannot be layered.)

``compress="mxfp4"`` and ``compress="mxfp4-rows"`` are the same two layouts with MXFP4
records (E2M1 codes, two to a byte, ``oncilla_amd.ops.mx4_encode_reference``): 17/64 of
the bytes, so a pool of the same size holds 1.94 times the blocks of an MXFP8 one.

Streams: swap_out waits for work already queued on torch's current stream (the
kernels that wrote the cache). After an async swap_in, that stream waits for the
copies, so later attention kernels see the blocks without a host sync.
"""
from __future__ import annotations

import math
from typing import Iterable, Sequence

import numpy as np

from .. import api


def coalesce_array(pairs) -> "np.ndarray":
    """(k, 2) [src, dst] block pairs -> (r, 3) [src, dst, count] runs where both sides are consecutive."""
    a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if a.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.int64)
    a = a[np.argsort(a[:, 0], kind="stable")]
    brk = np.ones(a.shape[0], dtype=bool)
    brk[1:] = (np.diff(a[:, 0]) != 1) | (np.diff(a[:, 1]) != 1)
    starts = np.flatnonzero(brk)
    counts = np.diff(np.append(starts, a.shape[0]))
    return np.stack([a[starts, 0], a[starts, 1], counts], axis=1)


def coalesce(pairs: Iterable[tuple[int, int]]) -> list[tuple[int, int, int]]:
    """[(src, dst)] block pairs -> [(src, dst, count)] runs where both sides are consecutive."""
    return [tuple(int(v) for v in r) for r in coalesce_array(list(pairs))]


class PagedKVOffload:
    """GPU KV-cache blocks (local half) + an offload pool of blocks (remote half)."""

    def __init__(self, client: api.Client, num_gpu_blocks: int, num_pool_blocks: int, block_shape: Sequence[int],
                 dtype=None, kind: int = api.OCM_REMOTE_GPU, flags: int = api.OCM_ALLOC_STRIPE, stripe_unit: int = 0,
                 remote_rank: int = -1, compress=None, layers: int = 0):
        import torch

        self.dtype = dtype or torch.float16
        self.block_shape = tuple(block_shape)
        elem = torch.empty((), dtype=self.dtype).element_size()
        self.block_elems = int(math.prod(self.block_shape))
        self.block_bytes = self.block_elems * elem
        self.num_gpu_blocks = num_gpu_blocks
        self.num_pool_blocks = num_pool_blocks
        self.compress = compress
        self.layers = int(layers)
        if self.layers < 0:
            raise ValueError("layers must be 0 (one cache of whole blocks) or the number of per-layer caches")
        if self.layers and compress in ("mxfp8", "mxfp4"):
            raise ValueError(f"layers > 0 cannot be combined with compress='{compress}' (one record per block): "
                             f"use compress='{compress}-rows', one record per layer")
        if compress in ("mxfp8-rows", "mxfp4-rows") and not self.layers:
            raise ValueError(f"compress='{compress}' keeps one record per layer: it needs layers > 0 "
                             f"(a cache of whole blocks takes compress='{compress[:5]}')")
        # bytes between pool blocks: the block itself, or its record rounded up to 32
        self.pool_block_bytes = self.block_bytes
        if compress is not None:
            if compress not in ("mxfp8", "mxfp8-rows", "mxfp4", "mxfp4-rows"):
                raise ValueError(f"unknown compression {compress!r} (None, 'mxfp8', 'mxfp8-rows', 'mxfp4' or "
                                 "'mxfp4-rows')")
            self.format = compress[:5]  # the record format: "mxfp8" or "mxfp4"
            if self.dtype not in (torch.float16, torch.bfloat16):
                raise ValueError(f"compress={compress!r} needs float16 or bfloat16 blocks")
            if self.block_elems % 32 or self.block_bytes % 16:
                raise ValueError(f"compress={compress!r} needs a block element count that is a multiple of 32")
            self.record_bytes = (api.quant_bytes(self.block_elems, self.format) + 31) // 32 * 32
            self.pool_block_bytes = self.record_bytes
        if self.layers:  # a block's layers side by side: their bytes, or their records
            self.pool_block_bytes = self.layers * self.pool_block_bytes
        lead = (self.layers, num_gpu_blocks) if self.layers else (num_gpu_blocks,)
        local_bytes = math.prod(lead) * self.block_bytes
        self.alloc = client.alloc(kind, local_bytes=local_bytes,
                                  remote_bytes=num_pool_blocks * self.pool_block_bytes, remote_rank=remote_rank,
                                  flags=flags, stripe_unit=stripe_unit)
        # The cache the model reads and writes: a zero-copy view of the local half.
        self.gpu_cache = self.alloc.local_tensor(self.dtype)[: local_bytes // elem].view(*lead, *self.block_shape)

    def _quant_ops(self, pairs, put: bool) -> api.BatchOps:
        # One op per block, never a coalesced run: a run's record would hold all its codes and
        # then all its scales, which a later read of one block could not find.
        a = np.asarray(pairs if isinstance(pairs, np.ndarray) else list(pairs), dtype=np.int64).reshape(-1, 2)
        g, p = (a[:, 0], a[:, 1]) if put else (a[:, 1], a[:, 0])  # (gpu block, pool block)
        if len(a) and ((g < 0).any() or (g >= self.num_gpu_blocks).any() or (p < 0).any()
                       or (p >= self.num_pool_blocks).any()):
            raise IndexError("block out of range")
        ops = np.stack([np.full_like(g, 1 if put else 0), g * self.block_bytes, p * self.pool_block_bytes,
                        np.full_like(g, self.block_elems)], axis=1)
        if len(a) and len(np.unique(a[:, 1])) != len(a):
            raise ValueError("compressed swaps take one op per block: a destination block is named twice")
        return api.quant_ops(ops, self.dtype, self.format)

    def _strided_ops(self, pairs, put: bool) -> api.BatchOps:
        # One op per block: rows = layers, a cache apart on the GPU, side by side in the pool.
        a = np.asarray(pairs if isinstance(pairs, np.ndarray) else list(pairs), dtype=np.int64).reshape(-1, 2)
        g, p = (a[:, 0], a[:, 1]) if put else (a[:, 1], a[:, 0])  # (gpu block, pool block)
        if len(a) and ((g < 0).any() or (g >= self.num_gpu_blocks).any() or (p < 0).any()
                       or (p >= self.num_pool_blocks).any()):
            raise IndexError("block out of range")
        if len(a) and len(np.unique(a[:, 1])) != len(a):
            raise ValueError("layered swaps take one op per block: a destination block is named twice")
        bb = self.block_bytes
        ops = np.stack([np.full_like(g, 1 if put else 0), g * bb, p * self.pool_block_bytes, np.full_like(g, bb),
                        np.full_like(g, self.layers), np.full_like(g, self.num_gpu_blocks * bb), np.full_like(g, bb)],
                       axis=1)
        return api.strided_ops(ops)

    def _quant_strided_ops(self, pairs, put: bool) -> api.BatchOps:
        # One op per block: rows = layers, a cache apart on the GPU, one record per layer side by
        # side in the pool.
        a = np.asarray(pairs if isinstance(pairs, np.ndarray) else list(pairs), dtype=np.int64).reshape(-1, 2)
        g, p = (a[:, 0], a[:, 1]) if put else (a[:, 1], a[:, 0])  # (gpu block, pool block)
        if len(a) and ((g < 0).any() or (g >= self.num_gpu_blocks).any() or (p < 0).any()
                       or (p >= self.num_pool_blocks).any()):
            raise IndexError("block out of range")
        if len(a) and len(np.unique(a[:, 1])) != len(a):
            raise ValueError("compressed swaps take one op per block: a destination block is named twice")
        bb = self.block_bytes
        ops = np.stack([np.full_like(g, 1 if put else 0), g * bb, p * self.pool_block_bytes,
                        np.full_like(g, self.block_elems), np.full_like(g, self.layers),
                        np.full_like(g, self.num_gpu_blocks * bb), np.full_like(g, self.record_bytes)], axis=1)
        return api.quant_strided_ops(ops, self.dtype, self.format)

    def _ops(self, pairs, put: bool) -> api.BatchOps:
        if self.compress and self.compress.endswith("-rows"):
            return self._quant_strided_ops(pairs, put)
        if self.compress:
            return self._quant_ops(pairs, put)
        if self.layers:
            return self._strided_ops(pairs, put)
        runs = coalesce_array(pairs if isinstance(pairs, np.ndarray) else list(pairs))
        g, p = (runs[:, 0], runs[:, 1]) if put else (runs[:, 1], runs[:, 0])  # (gpu block, pool block)
        n = runs[:, 2]
        if len(n) and ((g < 0).any() or (g + n > self.num_gpu_blocks).any() or (p < 0).any()
                       or (p + n > self.num_pool_blocks).any()):
            raise IndexError("block run out of range")
        bb = self.block_bytes
        ops = np.stack([np.full_like(n, 1 if put else 0), g * bb, p * bb, n * bb], axis=1)
        return api.batch_ops(ops)

    def _run(self, ops: api.BatchOps, async_: bool) -> None:
        if self.compress and self.compress.endswith("-rows"):
            self.alloc.quant_strided_batch(ops, async_=async_)
        elif self.compress:
            self.alloc.quant_batch(ops, async_=async_)
        elif self.layers:
            self.alloc.strided_batch(ops, async_=async_)
        else:
            self.alloc.batch(ops, async_=async_)

    def swap_out(self, gpu_to_pool: Iterable[tuple[int, int]], async_: bool = True) -> int:
        """Copy GPU blocks to pool blocks. Returns the number of batched ops issued."""
        ops = self._ops(gpu_to_pool, put=True)
        self.alloc.stream_wait()  # after the kernels that produced the blocks
        self._run(ops, async_)
        if async_:
            self.alloc.stream_signal()  # and before anything that overwrites them
        return ops.n

    def swap_in(self, pool_to_gpu: Iterable[tuple[int, int]], async_: bool = True) -> int:
        """Copy pool blocks into GPU blocks; torch's current stream waits for them."""
        ops = self._ops(pool_to_gpu, put=False)
        self.alloc.stream_wait()  # do not overwrite blocks still being read
        self._run(ops, async_)
        if async_:
            self.alloc.stream_signal()
        return ops.n

    def wait(self) -> None:
        self.alloc.wait()

    def close(self) -> None:
        self.alloc.free()
