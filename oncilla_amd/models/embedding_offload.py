"""An embedding table in disaggregated memory, looked up by id.

The table (num_rows x dim) lives in the remote half of one pair: peer HBM, striped, or
the pinned host tier, as the pool places it. The local half holds an output region of
``max_ids`` rows and an id region. A lookup copies the ids into the id region on torch's
current stream and runs ONE indexed get (ocm_copy_onesided_indexed, remote index only):
the library's own copy loop moves exactly the rows asked for, the ids never visit the
host, and nothing the host sends grows with their number. ``update`` is the scatter put.

Streams: a lookup waits for the work already queued on torch's current stream (the
kernel that produced the ids) and, when async, makes that stream wait for the copy, so
the rows can be consumed there without a host sync.

Ids outside [0, num_rows) move nothing: their output rows keep what they held, they are
counted, and IndexError names the count, at once for a blocking lookup and at ``wait()``
for an async one.
"""
from __future__ import annotations

from .. import api


def _index_error(e: api.OcmError):
    return IndexError(f"embedding ids outside the table: {e}") if "skipped" in str(e) else e


class RemoteEmbedding:
    """num_rows x dim table of `dtype` in a remote half; lookups of up to max_ids ids."""

    def __init__(self, client: api.Client, num_rows: int, dim: int, dtype=None, max_ids: int = 4096,
                 kind: int = api.OCM_REMOTE_GPU, flags: int = api.OCM_ALLOC_STRIPE, stripe_unit: int = 0,
                 remote_rank: int = -1):
        import torch

        self.dtype = dtype or torch.float16
        self.num_rows, self.dim, self.max_ids = int(num_rows), int(dim), int(max_ids)
        if self.num_rows < 1 or self.dim < 1 or self.max_ids < 1:
            raise ValueError("num_rows, dim and max_ids must be positive")
        self.row_bytes = self.dim * torch.empty((), dtype=self.dtype).element_size()
        out_bytes = self.max_ids * self.row_bytes
        self._ids_off = (out_bytes + 15) // 16 * 16  # int64 ids, or int32 in the same region
        self.alloc = client.alloc(kind, local_bytes=self._ids_off + 8 * self.max_ids,
                                  remote_bytes=self.num_rows * self.row_bytes, remote_rank=remote_rank, flags=flags,
                                  stripe_unit=stripe_unit)
        raw = self.alloc.local_tensor(torch.uint8)
        # zero-copy views of the local half: the rows a lookup returns, and where its ids go
        self.out = raw[:out_bytes].view(self.dtype).view(self.max_ids, self.dim)
        self._ids = {torch.int64: raw[self._ids_off: self._ids_off + 8 * self.max_ids].view(torch.int64),
                     torch.int32: raw[self._ids_off: self._ids_off + 4 * self.max_ids].view(torch.int32)}

    def load(self, weight) -> None:
        """Put the whole table (num_rows x dim, any device), in chunks staged through the output region."""
        if tuple(weight.shape) != (self.num_rows, self.dim) or weight.dtype != self.dtype:
            raise ValueError(f"the table is {self.num_rows} x {self.dim} of {self.dtype}")
        for r in range(0, self.num_rows, self.max_ids):
            n = min(self.max_ids, self.num_rows - r)
            self.out[:n].copy_(weight[r:r + n])
            self.alloc.stream_wait()
            self.alloc.put(0, r * self.row_bytes, n * self.row_bytes)  # blocking: the region is free again

    def _stage_ids(self, ids):
        import torch

        if ids.dtype not in self._ids:
            raise TypeError(f"ids must be int32 or int64, not {ids.dtype}")
        k = int(ids.numel())
        if k > self.max_ids:
            raise ValueError(f"{k} ids in one call, the id region holds {self.max_ids}")
        # on torch's current stream, from whichever device the ids are on: no host sync
        self._ids[ids.dtype][:k].copy_(ids.reshape(-1), non_blocking=True)
        return k, api.OCM_INDEX_I64 if ids.dtype == torch.int64 else api.OCM_INDEX_I32

    def _run(self, put: bool, k: int, itype: int, async_: bool) -> None:
        rb = self.row_bytes
        op = [[1 if put else 0, 0, 0, rb, k, rb, rb, api.OCM_INDEX_NONE, self._ids_off, self.max_ids, self.num_rows]]
        self.alloc.stream_wait()  # after the id copy, and the kernel that produced the ids
        try:
            self.alloc.indexed_batch(api.indexed_ops(op, itype), async_=async_)
        except api.OcmError as e:
            raise _index_error(e) from None
        if async_:
            self.alloc.stream_signal()  # torch's stream reads the rows after the copy

    def lookup(self, ids, async_: bool = True):
        """Rows ids[0], ids[1], ... of the table: a (len(ids), dim) view of the output region, valid
        until the next lookup or update. async_: queued, with torch's current stream made to wait for
        it; an id outside the table then raises IndexError at wait(), not here."""
        k, itype = self._stage_ids(ids)
        if k:
            self._run(False, k, itype, async_)
        return self.out[:k]

    def update(self, ids, rows, async_: bool = False) -> None:
        """Scatter put: table row ids[i] = rows[i]. The ids must be unique: two rows for one id have
        no defined result (either may win, and their pieces may mix)."""
        k, itype = self._stage_ids(ids)
        if tuple(rows.shape) != (k, self.dim) or rows.dtype != self.dtype:
            raise ValueError(f"rows must be {k} x {self.dim} of {self.dtype}")
        if k:
            self.out[:k].copy_(rows, non_blocking=True)
            self._run(True, k, itype, async_)

    def wait(self) -> None:
        """Completes queued lookups and updates; raises IndexError if they skipped ids."""
        try:
            self.alloc.wait()
        except api.OcmError as e:
            raise _index_error(e) from None

    def close(self) -> None:
        self.alloc.free()
