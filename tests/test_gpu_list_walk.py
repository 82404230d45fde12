"""The list kernels where every wave walks several tiles (csrc/src/kernels/xfer_batch.hip, xfer_strided.hip,
xfer_indexed.hip, xfer_quant.hip, xfer_quant_strided.hip, xfer_quant_indexed.hip, xfer_acc.hip, xfer_bag.hip).
A list launch has one wave per tile until the grid reaches its cap (128 workgroups in the host tier, 8 per
CU otherwise), so only lists of more tiles than waves reach the code that carries state from one tile of a
wave to its next: the row and piece counters, a row's indices and its skip flag, the per-op scalars, the
scale row in LDS. The lists of walk_cases.py have at least 2 * waves + 1 tiles for the launch's wave count,
asserted from a lower bound before anything runs, so every wave with tiles walks at least three; their
middle holds rows and ops of 2 and 3 tiles, op changes, empty ops and skipped rows. Every byte of both halves
is compared with the numpy models, with the pool in the pinned host tier (one daemon) and striped over three
owners (four daemons; the 4 KiB stripe unit is the smallest ocm_alloc takes, so byte tiles are 4 KiB).
The host-tier case of every kind runs async and waits."""
import os

import pytest
import torch

from oncilla_amd import api
from walk_cases import BUILDERS, HOST_WAVES, UNIT, check_skips, need

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM


def _waves(n_daemons):
    """The waves of the largest list launch on this tier (xfer_batch_grid)."""
    if n_daemons == 1:
        if "OCM_BATCH_HOST_GRID" in os.environ:
            pytest.skip("OCM_BATCH_HOST_GRID is set: the host-tier grid is not the 128 workgroups these lists are sized for")
        return HOST_WAVES
    return 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("kind", list(BUILDERS))
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_every_wave_walks_at_least_three_tiles(mesh_factory, n_daemons, kind):
    waves = _waves(n_daemons)
    case = BUILDERS[kind](waves)
    # a condition, not a measurement: every kind gives a unit counted here at least one tile
    assert case.lower_bound >= need(waves), (kind, case.lower_bound, waves)
    async_ = n_daemons == 1
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
        a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=case.local_bytes, remote_bytes=case.remote_bytes,
                    flags=api.OCM_ALLOC_STRIPE, stripe_unit=UNIT)
        ext = a.remote_info()["extents"]
        assert len(ext) == (1 if n_daemons == 1 else 3)
        assert all(e["tier"] == (api.OCM_TIER_HOST if n_daemons == 1 else api.OCM_TIER_GPU) for e in ext)
        before = api.indexed_counters()
        skipped, err = case.run(a, async_=async_)
        check_skips(case, skipped, err, async_, before, api.indexed_counters())
        a.wait()  # reported once
        a.free()
