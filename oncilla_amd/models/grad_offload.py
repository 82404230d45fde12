"""Gradient accumulation in disaggregated memory (a training workload).

Gradients that build up over several micro-batches are kept as fp32, usually in the app
GPU's HBM: the memory an offloaded optimizer exists to free. Here the fp32 accumulators
are the *remote half* of one oncilla remote pair (peer HBM over xGMI, the pinned host
tier, another node) and the *local half* holds only what a micro-batch produces: the
flat gradients in the parameters' own dtype, installed as each parameter's ``.grad``.
After every backward, :meth:`OffloadedGradAccumulator.add` issues ONE one-sided
accumulate (ocm_copy_onesided_accumulate): ``remote_f32 += scale * grad``, two fp32
roundings per element (``oncilla_amd.ops.accumulate_reference``), no fp32 staging buffer
and no round trip of the accumulators through HBM.

Local half::

    [ flat gradients, each tensor padded to 4 elements | fp32 read-back region ]

With ``readback=False`` the read-back region, 4 bytes per parameter of local HBM, gives way to
one chunk of zeros of at most 4 MiB::

    [ flat gradients, each tensor padded to 4 elements | zero chunk ]

``read()`` then raises: the consumer is ``OffloadedAdam.step(accumulator=...)``, whose kernel
reads the accumulators where they are and zeroes them in the same pass, so ``zero()`` (one
batch of puts from the chunk) runs only when the accumulator is built.

``sumsq()`` / ``grad_norm()`` reduce the accumulators where they live (one read-only kernel pass:
per-parameter fp64 sums of squares and counts of inf / NaN words), with ``readback`` either way:
what gradient clipping and loss scaling need, without the read-back region.

Streams: ``add`` waits for work already queued on torch's current stream (the backward
that wrote the gradients), and after an async ``add`` that stream waits for the
accumulate before anything overwrites them (``zero_grads``, the next backward).
"""
from __future__ import annotations

import math
from typing import Iterable

import numpy as np

from .. import api


def _pad(n: int, to: int) -> int:
    return (n + to - 1) // to * to


class OffloadedGradAccumulator:
    """Parameters' gradients (local half) + their fp32 accumulators (remote half)."""

    _ZERO_CHUNK = 4 << 20  # readback=False: at most this many bytes of zeros in the local half

    def __init__(self, params: Iterable, client: api.Client, kind: int = None, flags: int = api.OCM_ALLOC_STRIPE,
                 stripe_unit: int = 0, remote_rank: int = -1, readback: bool = True):
        import torch

        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no parameters that require gradients")
        for p in self.params:
            api.acc_dtype(p.dtype)  # ValueError for a type the accumulate cannot read
        on_gpu = self.params[0].is_cuda
        if kind is None:
            kind = api.OCM_REMOTE_GPU if on_gpu else api.OCM_REMOTE_RDMA
        # element index of each tensor among the accumulators, byte offset among the gradients;
        # a run of one dtype is one op, and an op starts on a 16-byte boundary on both sides
        self._slots = []  # (param, acc element index, local byte offset, numel)
        runs = []         # [local_offset, remote_offset, elems, dtype value]
        e = lo = 0
        for p in self.params:
            size, dt = p.element_size(), api.acc_dtype(p.dtype)
            if not runs or runs[-1][3] != dt:
                lo = _pad(lo, 16)
                runs.append([lo, 4 * e, 0, dt])
            n = _pad(p.numel(), 4)
            self._slots.append((p, e, lo, p.numel()))
            runs[-1][2] += n
            e += n
            lo += n * size
        self.total_elems = e
        self.grad_bytes = _pad(lo, 16)
        self.readback = readback
        self.zero_bytes = min(4 * e, self._ZERO_CHUNK)  # readback=False: the zero chunk
        self.local_bytes = self.grad_bytes + (4 * e if readback else self.zero_bytes)
        self.alloc = client.alloc(kind, local_bytes=self.local_bytes, remote_bytes=4 * e, remote_rank=remote_rank,
                                  flags=flags, stripe_unit=stripe_unit)
        self._runs = np.asarray(runs, dtype=np.int64)
        local = self.alloc.local_tensor(torch.uint8)
        self._grad_region = local[: self.grad_bytes]
        self._readback = local[self.grad_bytes: self.local_bytes].view(torch.float32)
        self._grad_region.zero_()
        for p, _, off, n in self._slots:
            # the gradient autograd accumulates into: a zero-copy view of the local half
            p.grad = local[off: off + n * p.element_size()].view(p.dtype).view(p.shape)
        self.zero()

    def _ops(self, scale: float) -> api.BatchOps:
        r = self._runs
        ops = np.zeros((len(r), 5), dtype=np.float64)  # offsets here are far below 2^53
        ops[:, :4] = r
        ops[:, 4] = scale
        return api.acc_ops(ops)

    def add(self, scale: float = 1.0, async_: bool = True) -> int:
        """accumulators += scale * the current gradients. Returns the number of ops issued
        (one when every parameter has the same dtype)."""
        ops = self._ops(scale)
        self.alloc.stream_wait()  # after the backward that wrote the gradients
        self.alloc.accumulate_batch(ops, async_=async_)
        if async_:
            self.alloc.stream_signal()  # and before anything that overwrites them
        return ops.n

    def zero_grads(self) -> None:
        """Zero the gradients of the local half in place (the views stay installed as ``.grad``;
        an optimizer's ``zero_grad(set_to_none=True)`` would drop them)."""
        self._grad_region.zero_()
        for p, _, off, n in self._slots:
            if p.grad is None or p.grad.data_ptr() != self._grad_region.data_ptr() + off:
                p.grad = self._grad_region[off: off + n * p.element_size()].view(p.dtype).view(p.shape)

    def read(self) -> list:
        """The accumulators, fetched into the read-back region: one fp32 view per parameter,
        valid until the next read() or zero()."""
        if not self.readback:
            raise RuntimeError("read() needs the read-back region (readback=True)")
        self.alloc.stream_wait()  # earlier readers of the region on torch's stream
        self.alloc.get(self.grad_bytes, 0, 4 * self.total_elems)
        return [self._readback[e: e + n].view(p.shape) for p, e, _, n in self._slots]

    def sumsq(self, stream=None):
        """(float64[count + 1], int64[count + 1]) device tensors: per parameter the sum of squares
        of its accumulators (fp64 accumulation) and the number of inf / NaN words among them, the
        totals last; one read-only pass where the accumulators live (Allocation.acc_sumsq over the
        true element counts, not the padded ones). Queued behind the accumulates; no host wait.
        Works with ``readback`` either way."""
        return self.alloc.acc_sumsq([4 * e for _, e, _, _ in self._slots], [n for _, _, _, n in self._slots], stream=stream)

    def _norm_parts(self) -> tuple:
        """(total sum of squares, total non-finite count) as Python numbers: one host synchronise."""
        sumsq, bad = self.sumsq()
        return float(sumsq[-1].item()), int(bad[-1].item())  # .item() waits for the stream

    def grad_norm(self, scale: float = 1.0) -> tuple:
        """(norm, nonfinite): the 2-norm of scale * every accumulator, a Python float, and how many
        accumulator words are inf or NaN. One host synchronise (the results are read back)."""
        total, bad = self._norm_parts()
        return abs(scale) * math.sqrt(total), bad

    def zero(self) -> None:
        """Reset every accumulator to +0."""
        self._readback.zero_()
        self.alloc.stream_wait()
        if self.readback:
            self.alloc.put(self.grad_bytes, 0, 4 * self.total_elems)
            return
        total, z = 4 * self.total_elems, self.zero_bytes  # one batch of puts (op_flag 1) from the zero chunk
        self.alloc.batch([(1, self.grad_bytes, off, min(z, total - off)) for off in range(0, total, z)])

    def wait(self) -> None:
        self.alloc.wait()

    def close(self) -> None:
        self.alloc.free()
