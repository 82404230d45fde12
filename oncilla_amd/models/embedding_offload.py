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

``compress="mxfp8"`` or ``"mxfp4"`` keeps the table as MX records in the remote half, one
record per row (its codes, then its scale bytes: the layout of ocm_copy_onesided_quant) at a
stride of the record bytes rounded up to 32: 33/64 or 17/64 of the bytes cross the link and,
but for that padding, lie in the pool. ``load`` is then the strided converting put, a lookup ONE
indexed converting get (ocm_copy_onesided_quant_indexed) and ``update`` the indexed converting
put; a lookup returns the decode of the encode of the rows that were loaded, which is not the
rows themselves. Ids, streams and out-of-range ids are as without it.

Ids outside [0, num_rows) move nothing: their output rows keep what they held, they are
counted, and IndexError names the count, at once for a blocking lookup and at ``wait()``
for an async one.

``max_bags > 0`` adds what nn.EmbeddingBag's forward needs: ``lookup_bags(ids, offsets)`` runs
ONE pooled lookup (ocm_copy_onesided_bag) that reads every bag's rows out of the remote half,
sums them in registers (in order, in fp32; optionally weighted, or the mean) and writes
``bags x dim`` sums. No row is written to the local half and read back, the output region
is sized for the bags of a batch and not for its ids, and there is no second launch. Ids
outside the table add nothing to their bag and are reported as above.

RemoteEmbeddingAdam trains such a table where it lives: one fused row-sparse Adam launch per
step (ocm_x_adam_rows) on the rows whose ids were in the batch, with the moments (and, for a
bfloat16 table, fp32 master rows) in the remote half of a second pair.
"""
from __future__ import annotations

from .. import api


def _index_error(e: api.OcmError):
    return IndexError(f"embedding ids outside the table: {e}") if "skipped" in str(e) else e


class RemoteEmbedding:
    """num_rows x dim table of `dtype` in a remote half; lookups of up to max_ids ids. compress:
    None, or "mxfp8" / "mxfp4" for a table of float16 or bfloat16 rows with dim % 32 == 0 kept as
    one MX record per row. record_stride: bytes from one row to the next in the remote half;
    remote_bytes: the bytes the table takes there. max_bags: 0, or the most bags one lookup_bags
    call pools (a table of float32, bfloat16 or float16 rows of a multiple of 16 bytes); with 0 the
    local half is laid out as it always was."""

    def __init__(self, client: api.Client, num_rows: int, dim: int, dtype=None, max_ids: int = 4096,
                 kind: int = api.OCM_REMOTE_GPU, flags: int = api.OCM_ALLOC_STRIPE, stripe_unit: int = 0,
                 remote_rank: int = -1, compress=None, max_bags: int = 0):
        import torch

        self.dtype = dtype or torch.float16
        self.compress = compress
        self.client = client
        self._place = dict(kind=kind, flags=flags, stripe_unit=stripe_unit, remote_rank=remote_rank)
        self.num_rows, self.dim, self.max_ids = int(num_rows), int(dim), int(max_ids)
        if self.num_rows < 1 or self.dim < 1 or self.max_ids < 1:
            raise ValueError("num_rows, dim and max_ids must be positive")
        self.row_bytes = self.dim * torch.empty((), dtype=self.dtype).element_size()
        # bytes from one table row to the next in the remote half, and the bytes the table takes there
        self.record_stride = self.row_bytes
        if compress is not None:
            api.quant_format(compress)  # ValueError for anything but "mxfp8" / "mxfp4"
            if self.dtype not in (torch.float16, torch.bfloat16):
                raise ValueError(f"a compressed table holds float16 or bfloat16 rows, not {self.dtype}")
            if self.dim % 32 != 0:
                raise ValueError(f"a compressed table needs dim % 32 == 0 (one scale per 32 elements), not dim {self.dim}")
            self.record_stride = (api.quant_bytes(self.dim, compress) + 31) // 32 * 32
        self.remote_bytes = self.num_rows * self.record_stride
        out_bytes = self.max_ids * self.row_bytes
        self._ids_off = (out_bytes + 15) // 16 * 16  # int64 ids, or int32 in the same region
        local_bytes = self._ids_off + 8 * self.max_ids
        self.max_bags = int(max_bags)
        if self.max_bags < 0:
            raise ValueError("max_bags must not be negative")
        if self.max_bags:
            if compress is None and (self.row_bytes % 16 != 0 or self.dtype not in (torch.float32, torch.bfloat16, torch.float16)):
                raise ValueError(f"pooled lookups need float32, bfloat16 or float16 rows of a multiple of 16 bytes, "
                                 f"not {self.dim} x {self.dtype}")
            # behind the ids: bags + 1 offsets (typed as the ids are), one fp32 weight per id, the bags' sums
            self._offs_off = local_bytes
            self._w_off = self._offs_off + 8 * (self.max_bags + 1)
            self._bag_off = (self._w_off + 4 * self.max_ids + 15) // 16 * 16
            local_bytes = self._bag_off + self.max_bags * self.row_bytes
        self.alloc = client.alloc(kind, local_bytes=local_bytes,
                                  remote_bytes=self.remote_bytes, remote_rank=remote_rank, flags=flags,
                                  stripe_unit=stripe_unit)
        raw = self.alloc.local_tensor(torch.uint8)
        # zero-copy views of the local half: the rows a lookup returns, and where its ids go
        self.out = raw[:out_bytes].view(self.dtype).view(self.max_ids, self.dim)
        self._ids = {torch.int64: raw[self._ids_off: self._ids_off + 8 * self.max_ids].view(torch.int64),
                     torch.int32: raw[self._ids_off: self._ids_off + 4 * self.max_ids].view(torch.int32)}
        if self.max_bags:
            n = self.max_bags + 1
            self._offs = {torch.int64: raw[self._offs_off: self._offs_off + 8 * n].view(torch.int64),
                          torch.int32: raw[self._offs_off: self._offs_off + 4 * n].view(torch.int32)}
            self._w = raw[self._w_off: self._w_off + 4 * self.max_ids].view(torch.float32)
            self.bag_out = raw[self._bag_off: self._bag_off + self.max_bags * self.row_bytes].view(self.dtype).view(self.max_bags, self.dim)

    def load(self, weight) -> None:
        """Put the whole table (num_rows x dim, any device), in chunks staged through the output region."""
        if tuple(weight.shape) != (self.num_rows, self.dim) or weight.dtype != self.dtype:
            raise ValueError(f"the table is {self.num_rows} x {self.dim} of {self.dtype}")
        for r in range(0, self.num_rows, self.max_ids):
            n = min(self.max_ids, self.num_rows - r)
            self.out[:n].copy_(weight[r:r + n])
            self.alloc.stream_wait()
            if self.compress is None:
                self.alloc.put(0, r * self.row_bytes, n * self.row_bytes)  # blocking: the region is free again
            else:  # one record per row, blocking likewise
                self.alloc.quant_strided_batch([[1, 0, r * self.record_stride, self.dim, n, self.row_bytes, self.record_stride]],
                                               self.dtype, format=self.compress)

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
        # row_bytes, or for a compressed table row_elems, in column 3
        op = [[1 if put else 0, 0, 0, rb if self.compress is None else self.dim, k, rb, self.record_stride, api.OCM_INDEX_NONE,
               self._ids_off, self.max_ids, self.num_rows]]
        self.alloc.stream_wait()  # after the id copy, and the kernel that produced the ids
        try:
            if self.compress is None:
                self.alloc.indexed_batch(api.indexed_ops(op, itype), async_=async_)
            else:
                self.alloc.quant_indexed_batch(api.quant_indexed_ops(op, self.dtype, itype, self.compress), async_=async_)
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

    def lookup_bags(self, ids, offsets, per_sample_weights=None, mode: str = "sum", async_: bool = True):
        """nn.functional.embedding_bag's forward over the remote table: bag b is ids[offsets[b]:
        offsets[b + 1]] (the last one runs to the end of ids, as torch's does), and row b of the result
        is the sum of the table rows its ids pick, their weighted sum with per_sample_weights (one per
        id, mode "sum" only), or their mean. A (bags, dim) view of the bag-output region, valid until
        the next lookup_bags. The terms are added in the order of ids, in fp32, and the sum is narrowed to
        the table's dtype once: torch adds in another order, so the two agree to rounding, not bit for
        bit. offsets gets its closing entry len(ids) on the device; nothing syncs the host. Streams and
        ids outside the table (IndexError; they add nothing to their bag) as for lookup."""
        import torch

        if self.compress is not None:
            raise TypeError(f"lookup_bags does not serve a compressed ({self.compress}) table: pooling MX records is not built")
        if not self.max_bags:
            raise ValueError("lookup_bags needs a RemoteEmbedding made with max_bags > 0")
        if per_sample_weights is not None and mode != "sum":
            raise ValueError("per_sample_weights go with mode 'sum' only")
        bags = int(offsets.numel())
        if bags > self.max_bags:
            raise ValueError(f"{bags} bags in one call, the bag-output region holds {self.max_bags}")
        if offsets.dtype not in self._offs:
            raise TypeError(f"offsets must be int32 or int64, not {offsets.dtype}")
        k, itype = self._stage_ids(ids)
        if per_sample_weights is not None and int(per_sample_weights.numel()) != k:
            raise ValueError(f"{int(per_sample_weights.numel())} weights for {k} ids")
        if bags == 0:
            return self.bag_out[:0]
        # on torch's current stream, as the ids are: the offsets in the ids' type, then the closing entry
        offs = self._offs[ids.dtype]
        offs[:bags].copy_(offsets.reshape(-1), non_blocking=True)
        offs[bags:bags + 1].fill_(k)
        w_off = api.OCM_INDEX_NONE
        if per_sample_weights is not None and k:
            self._w[:k].copy_(per_sample_weights.reshape(-1), non_blocking=True)
            w_off = self._w_off
        op = [[self._bag_off, 0, self.dim, bags, k, self.row_bytes, self.record_stride, self.num_rows, self._ids_off,
               self._offs_off, w_off]]
        self.alloc.stream_wait()  # after the copies above, and the kernels that produced what they copied
        try:
            self.alloc.bag_batch(api.bag_ops(op, self.dtype, itype, mode), async_=async_)
        except api.OcmError as e:
            raise _index_error(e) from None
        if async_:
            self.alloc.stream_signal()  # torch's stream reads the sums after the lookup
        return self.bag_out[:bags]

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


class RemoteEmbeddingAdam:
    """Row-sparse ("lazy") Adam for a RemoteEmbedding of float32 or bfloat16.

    The state is a pair of its own, placed as the table is: exp_avg and exp_avg_sq tables of
    num_rows x dim fp32 in its remote half, zeroed, and for a bfloat16 table fp32 master rows,
    initialised from the table. ``step`` updates the rows whose ids it is given, and nothing
    else, in one launch: the element rule is the dense fused Adam's (Allocation.adam), with the
    global step count in the bias corrections for every row, so a row's moments do not move
    while it is not picked. This is not torch.optim.SparseAdam's arithmetic (which adds eps
    before the bias correction). There is no weight decay: what it would mean for rows that are
    not picked is a policy nobody has chosen. float16 tables are not served."""

    def __init__(self, emb: RemoteEmbedding, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0):
        import torch

        if getattr(emb, "compress", None) is not None:
            raise TypeError(f"RemoteEmbeddingAdam does not serve a compressed ({emb.compress}) table: "
                            "training a quantized table is not defined here")
        if emb.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"RemoteEmbeddingAdam serves float32 and bfloat16 tables, not {emb.dtype} "
                            "(RemoteEmbedding's default dtype is float16: pass dtype=torch.float32 or torch.bfloat16)")
        if weight_decay != 0.0:
            raise ValueError("RemoteEmbeddingAdam has no weight decay: it is not defined for rows that are not picked")
        self.emb, self.lr, self.betas, self.eps = emb, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.bf16 = emb.dtype == torch.bfloat16
        self.t = 0
        n, dim, k = emb.num_rows, emb.dim, emb.max_ids
        self.row_bytes = 4 * dim  # of every state table (fp32)
        table = (n * self.row_bytes + 15) // 16 * 16
        names = ("m", "v", "w") if self.bf16 else ("m", "v")
        self.off = {name: i * table for i, name in enumerate(names)}
        self._ids_off = (k * self.row_bytes + 15) // 16 * 16
        self.state = emb.client.alloc(local_bytes=self._ids_off + 8 * k, remote_bytes=len(names) * table, **emb._place)
        raw = self.state.local_tensor(torch.uint8)
        self._stage = raw[:k * self.row_bytes].view(torch.float32).view(k, dim)
        self._ids = {torch.int64: raw[self._ids_off: self._ids_off + 8 * k].view(torch.int64),
                     torch.int32: raw[self._ids_off: self._ids_off + 4 * k].view(torch.int32)}
        dev = self._stage.device
        self._skipped = torch.zeros(1, dtype=torch.int64, device=dev) if dev.type == "cuda" else None
        for r in range(0, n, k):
            c = min(k, n - r)
            for name in names:
                if name == "w":  # the master starts as the table's value
                    emb.alloc.get(0, r * emb.row_bytes, c * emb.row_bytes)
                    self._stage[:c].copy_(emb.out[:c])
                else:
                    self._stage[:c].zero_()
                self.state.stream_wait()
                self.state.put(0, self.off[name] + r * self.row_bytes, c * self.row_bytes)  # blocking

    def _hp(self, t: int) -> tuple:
        import math

        b1, b2 = self.betas
        return (b1, b2, self.eps, 0.0, self.lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t))

    def step(self, ids, grad_rows=None, scale: float = 1.0) -> None:
        """One step on table rows ``ids`` (int32 / int64, any shape, on the table's GPU) with the
        gradient rows ``grad_rows`` (ids.numel() x dim), or ``step(sparse_grad)`` with a sparse COO
        gradient of the table's shape, as nn.Embedding(sparse=True) produces. Duplicate ids are
        coalesced with torch on the device (torch.unique and index_add_ in fp32; a sparse gradient by
        coalesce()), the sum is cast to the table's dtype, and ONE ocm_x_adam_rows launch is queued on
        torch's current stream: the gradient of a row is fl32(scale * sum). torch.unique (and
        coalesce) sync the host for the number of distinct ids; the launch itself does not. Ids outside
        the table move nothing and are counted (``skipped``). A later lookup() sees the step."""
        import torch

        if grad_rows is None:
            sp = ids.coalesce()
            if tuple(sp.shape) != (self.emb.num_rows, self.emb.dim) or sp.sparse_dim() != 1:
                raise ValueError(f"the sparse gradient must be {self.emb.num_rows} x {self.emb.dim} with one sparse dimension")
            uniq, g = sp.indices()[0].contiguous(), sp.values().float()
        else:
            ids = ids.reshape(-1)
            if ids.dtype not in (torch.int32, torch.int64):
                raise TypeError(f"ids must be int32 or int64, not {ids.dtype}")
            if tuple(grad_rows.shape) != (ids.numel(), self.emb.dim):
                raise ValueError(f"grad_rows must be {ids.numel()} x {self.emb.dim}")
            uniq, inv = torch.unique(ids, return_inverse=True)  # a host sync: the count
            g = torch.zeros((uniq.numel(), self.emb.dim), dtype=torch.float32, device=grad_rows.device)
            g.index_add_(0, inv, grad_rows.float())
        if uniq.numel() == 0:
            return
        g = g.to(self.emb.dtype).contiguous()
        self.t += 1
        emb, rb = self.emb, self.row_bytes
        emb.alloc.adam_rows(self.state, uniq, g, (0, emb.row_bytes), (self.off["m"], rb), (self.off["v"], rb),
                            self._hp(self.t), emb.num_rows, master=(self.off["w"], rb) if self.bf16 else None,
                            gscale=scale, skipped=self._skipped)

    def step_bags(self, ids, offsets, grad_bags, per_sample_weights=None, scale: float = 1.0) -> None:
        """One step from the gradient of a lookup_bags(ids, offsets, per_sample_weights) sum: the
        gradient of the row an id picked is its bag's gradient row (times the id's weight). The bag
        gradient (bags x dim) is expanded to one row per id with torch on the device, in fp32, and
        handed to ``step``: there is no kernel of its own."""
        import torch

        ids = ids.reshape(-1)
        k, bags = int(ids.numel()), int(offsets.numel())
        if tuple(grad_bags.shape) != (bags, self.emb.dim):
            raise ValueError(f"grad_bags must be {bags} x {self.emb.dim}")
        if per_sample_weights is not None and int(per_sample_weights.numel()) != k:
            raise ValueError(f"{int(per_sample_weights.numel())} weights for {k} ids")
        offs = offsets.reshape(-1).to(device=ids.device, dtype=torch.int64)
        ends = torch.cat([offs[1:], torch.full((1,), k, dtype=torch.int64, device=ids.device)])
        # output_size: the host already knows it, so repeat_interleave does not sync for it
        bag_of_id = torch.repeat_interleave(torch.arange(bags, device=ids.device), ends - offs, output_size=k)
        g = grad_bags.float().index_select(0, bag_of_id)
        if per_sample_weights is not None:
            g = g * per_sample_weights.reshape(-1).float().unsqueeze(1)
        self.step(ids, g, scale)

    def skipped(self) -> int:
        """Rows skipped so far because their id was outside the table. A host sync; resets nothing."""
        return int(self._skipped.item()) if self._skipped is not None else 0

    def _rows(self, name: str, ids):
        k = int(ids.numel())
        if ids.dtype not in self._ids:
            raise TypeError(f"ids must be int32 or int64, not {ids.dtype}")
        if k > self.emb.max_ids:
            raise ValueError(f"{k} ids in one call, the id region holds {self.emb.max_ids}")
        if k == 0:
            return self._stage[:0].clone()
        self._ids[ids.dtype][:k].copy_(ids.reshape(-1), non_blocking=True)
        rb = self.row_bytes
        op = [[0, 0, self.off[name], rb, k, rb, rb, api.OCM_INDEX_NONE, self._ids_off, self.emb.max_ids, self.emb.num_rows]]
        self.state.stream_wait()  # after the id copy and the steps queued on torch's stream
        try:
            self.state.indexed_batch(api.indexed_ops(op, api.index_type_of(ids.dtype)))
        except api.OcmError as e:
            raise _index_error(e) from None
        return self._stage[:k].clone()

    def moments(self, ids):
        """(exp_avg rows, exp_avg_sq rows) of ``ids`` (at most max_ids), read back with indexed gets:
        for tests and checkpoints."""
        return self._rows("m", ids), self._rows("v", ids)

    def master(self, ids):
        """The fp32 master rows of ``ids`` (bfloat16 tables only)."""
        if not self.bf16:
            raise TypeError("only a bfloat16 table has master rows")
        return self._rows("w", ids)

    def close(self) -> None:
        self.state.free()
