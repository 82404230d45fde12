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

Indexed swaps (``indexed_ids``) cover the plain cache only: combined with ``compress`` they
raise ValueError. The library has the call they would take, indexed rows of MX records
(ocm_copy_onesided_quant_indexed, which RemoteEmbedding uses); compressed indexed KV swaps
are a later change.

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
                 remote_rank: int = -1, compress=None, layers: int = 0, indexed_ids: int = 0):
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
        # swap_out_indexed / swap_in_indexed: a tail of the local half for two arrays of
        # `indexed_ids` int64 block ids (0: no tail, the half is the cache alone)
        self.indexed_ids = int(indexed_ids)
        if self.indexed_ids < 0:
            raise ValueError("indexed_ids must be 0 or the most blocks one indexed swap names")
        if self.indexed_ids and (self.layers or compress):
            raise ValueError("indexed swaps cover the plain cache only: no layers (an index-times-stride op) "
                             "and no compress")
        self._ids_off = (local_bytes + 15) // 16 * 16
        cache_bytes = local_bytes
        if self.indexed_ids:
            local_bytes = self._ids_off + 2 * 8 * self.indexed_ids
        self.alloc = client.alloc(kind, local_bytes=local_bytes,
                                  remote_bytes=num_pool_blocks * self.pool_block_bytes, remote_rank=remote_rank,
                                  flags=flags, stripe_unit=stripe_unit)
        # The cache the model reads and writes: a zero-copy view of the local half.
        self.gpu_cache = self.alloc.local_tensor(self.dtype)[: cache_bytes // elem].view(*lead, *self.block_shape)
        if self.indexed_ids:
            ids = self.alloc.local_tensor(torch.uint8)[self._ids_off: self._ids_off + 16 * self.indexed_ids]
            self._ids = ids.view(torch.int64).view(2, self.indexed_ids)  # [0]: GPU block ids, [1]: pool block ids

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

    def _swap_indexed(self, gpu_ids, pool_ids, put: bool, async_: bool) -> int:
        if self.layers or self.compress:
            raise ValueError("indexed swaps cover the plain cache only: no layers (an index-times-stride op) "
                             "and no compress")
        if not self.indexed_ids:
            raise ValueError("indexed swaps need the id region: construct with indexed_ids=N")
        k = int(gpu_ids.numel())
        if k != int(pool_ids.numel()):
            raise ValueError("one pool block id per GPU block id")
        if k > self.indexed_ids:
            raise ValueError(f"{k} blocks in one indexed swap, the id region holds {self.indexed_ids}")
        if k == 0:
            return 0
        # onto the id region on torch's current stream (no host sync, whichever device the ids are on)
        self._ids[0, :k].copy_(gpu_ids.reshape(-1), non_blocking=True)
        self._ids[1, :k].copy_(pool_ids.reshape(-1), non_blocking=True)
        bb = self.block_bytes
        op = [[1 if put else 0, 0, 0, bb, k, bb, bb, self._ids_off, self._ids_off + 8 * self.indexed_ids,
               self.num_gpu_blocks, self.num_pool_blocks]]
        self.alloc.stream_wait()  # after the copies above and the kernels that produced ids and blocks
        try:
            self.alloc.indexed_batch(api.indexed_ops(op, api.OCM_INDEX_I64), async_=async_)
        except api.OcmError as e:
            if "skipped" in str(e):
                raise IndexError(f"indexed swap: {e}") from None
            raise
        if async_:
            self.alloc.stream_signal()
        return 1

    def swap_out_indexed(self, gpu_ids, pool_ids, async_: bool = True) -> int:
        """swap_out with the block ids in tensors (on the GPU: chosen by a scheduler kernel): GPU block
        gpu_ids[i] goes to pool block pool_ids[i], as ONE indexed op with both index arrays and no host
        loop over blocks. pool_ids must be unique (duplicate destinations have no defined result). An id
        outside its cache skips that block; the call (blocking) or the next wait() (async) then raises
        IndexError. Plain caches only: with `layers` or `compress` it raises ValueError. Returns the
        number of ops issued."""
        return self._swap_indexed(gpu_ids, pool_ids, True, async_)

    def swap_in_indexed(self, pool_ids, gpu_ids, async_: bool = True) -> int:
        """swap_in likewise: pool block pool_ids[i] comes into GPU block gpu_ids[i] (gpu_ids unique);
        torch's current stream waits for the copies."""
        return self._swap_indexed(gpu_ids, pool_ids, False, async_)

    def wait(self) -> None:
        try:
            self.alloc.wait()
        except api.OcmError as e:
            if "skipped" in str(e):
                raise IndexError(f"indexed swap: {e}") from None
            raise

    def close(self) -> None:
        self.alloc.free()
