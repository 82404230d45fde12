"""Workloads on the runtime: the BASELINE.json configs (#1-#5) and a serving
use of disaggregated memory (paged KV-cache offload), and a training one (gradient
accumulation in the remote half), and an embedding table in remote memory looked up by id and trained
there by a row-sparse fused Adam."""
from .embedding_offload import RemoteEmbedding, RemoteEmbeddingAdam
from .grad_offload import OffloadedGradAccumulator
from .kv_offload import PagedKVOffload, coalesce
from .optim_offload import OffloadedAdam, OffloadedAdamW
from .workloads import alloc_latency, characterize, churn, percentile, rw_sweep_step, spill_probe, sweep_sizes

__all__ = ["OffloadedAdam", "OffloadedAdamW", "OffloadedGradAccumulator", "PagedKVOffload", "RemoteEmbedding", "RemoteEmbeddingAdam", "alloc_latency", "characterize", "churn", "coalesce", "percentile", "rw_sweep_step",
           "spill_probe", "sweep_sizes"]
