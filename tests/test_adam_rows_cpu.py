"""The row-sparse fused Adam, checked without a GPU: the rule by rows (adam1 on the picked rows, the
global step in the bias corrections) inside adam_cases' bound of the fp64 oracle, RemoteEmbeddingAdam.step
with the native call stubbed (coalescing, offsets and strides, the refusals), and the hook itself on a
CPU mesh. What runs the kernel is tests/test_gpu_adam_rows.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

from adam_acc_cases import scaled
from adam_cases import QUANTITIES, bound, errors, hyper
from adam_rows_cases import (DIMS, HP_NAME, ID_STEPS, TABLE_ROWS, build_case, case, check_rows, kernel_hp_rows, make_table,
                             picked_mask, rows_oracle, rows_rule_fp32, rows_torch)
from oncilla_amd import api
from oncilla_amd.models import RemoteEmbedding, RemoteEmbeddingAdam
from quant_cases import read_remote, write_remote


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("dim", DIMS)
def test_rule_by_rows_within_the_bound(dim, bf16):
    hp, _ = hyper(HP_NAME)
    c = case(dim, bf16)
    got = rows_rule_fp32(c.p, c.steps, hp)[-1]
    check_rows(got, c, f"replay dim={dim} bf16={bf16}")
    # rows never picked: untouched by the oracle, the yardstick and the replay alike
    never = ~c.picked
    assert not bool(never.any())  # the third step picks every row ...
    two = build_case(c.p, c.g_tables, ID_STEPS[:2])  # ... the first two leave 31 alone
    got2 = rows_rule_fp32(two.p, two.steps, hp)[-1]
    assert int((~two.picked).all(dim=1).sum()) == TABLE_ROWS - 6
    assert torch.equal(got2[0][~two.picked], two.p[~two.picked]) and not got2[1][~two.picked].any()
    check_rows(got2, two, f"replay two steps dim={dim} bf16={bf16}")


def test_lazy_bias_correction_is_the_global_step():
    """Row 36 is picked at steps 2 and 4: its second update uses the corrections of step 4, not of its
    own second update. The oracle with per-row step counts is far outside the bound."""
    hp, _ = hyper(HP_NAME)
    c = case(8)
    ids = [36]
    own = [(tuple(ids), c.g_tables[1][ids]), (tuple(ids), c.g_tables[3][ids])]  # the row's own steps 1 and 2
    glob = [((), c.g_tables[0][[]]), own[0], ((), c.g_tables[2][[]]), own[1]]
    want, wrong = rows_oracle(c.p, glob, hp)[-1], rows_oracle(c.p, own, hp)[-1]
    mask = picked_mask(TABLE_ROWS, 8, own)
    t32 = rows_torch(c.p, glob, hp)[-1]
    b = bound(errors(t32, want, hp.lr, mask))
    e = errors(rows_rule_fp32(c.p, glob, hp)[-1], want, hp.lr, mask)
    assert all(e[q] <= b[q] for q in QUANTITIES)
    assert errors((wrong.p, wrong.m, wrong.v), want, hp.lr, mask)["p"] > 100 * b["p"]


def test_gscale_is_one_rounding_of_its_own():
    hp, _ = hyper(HP_NAME)
    c = case(260)
    third = [(ids, scaled(g, 1.0 / 3.0)) for ids, g in c.steps]
    want, t32 = rows_oracle(c.p, third, hp)[-1], rows_torch(c.p, third, hp)[-1]
    got = rows_rule_fp32(c.p, c.steps, hp, gscale=1.0 / 3.0)[-1]
    b, e = bound(errors(t32, want, hp.lr, c.picked)), errors(got, want, hp.lr, c.picked)
    assert all(e[q] <= b[q] for q in QUANTITIES), (e, b)
    one = rows_rule_fp32(c.p, c.steps, hp, gscale=1.0)[-1]
    plain = rows_rule_fp32(c.p, c.steps, hp)[-1]
    assert all(torch.equal(a.view(torch.int32), b_.view(torch.int32)) for a, b_ in zip(one, plain))


# ---- RemoteEmbeddingAdam.step with the native call stubbed ----

class _FakeAlloc:
    def __init__(self, local_bytes, remote_bytes):
        self.buf = torch.zeros(local_bytes, dtype=torch.uint8)
        self.remote_bytes = remote_bytes
        self.calls, self.puts = [], []

    def local_tensor(self, dtype=None):
        return self.buf.view(dtype) if dtype else self.buf

    def put(self, lo, ro, n, **kw):
        self.puts.append((lo, ro, n, self.buf[lo:lo + n].clone()))

    def get(self, lo, ro, n, **kw):
        self.buf[lo:lo + n] = 0x3F  # bf16 pairs 0x3F3F: 0.74609375

    def stream_wait(self, *a, **kw):
        pass

    def adam_rows(self, state, ids, grad, table, exp_avg, exp_avg_sq, hp, table_rows, master=None, gscale=1.0,
                  skipped=None, stream=None):
        self.calls.append(dict(state=state, ids=ids.clone(), grad=grad.clone(), table=table, m=exp_avg, v=exp_avg_sq, hp=hp,
                               rows=table_rows, w=master, gscale=gscale))

    def free(self):
        pass


class _FakeClient:
    device = 0

    def __init__(self):
        self.made = []

    def alloc(self, kind, local_bytes=0, remote_bytes=0, **kw):
        self.made.append(_FakeAlloc(local_bytes, remote_bytes))
        self.made[-1].kw = dict(kind=kind, **kw)
        return self.made[-1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_descriptors(dtype):
    rows, dim, max_ids = 50, 12, 16
    fake = _FakeClient()
    emb = RemoteEmbedding(fake, rows, dim, dtype=dtype, max_ids=max_ids, kind=api.OCM_REMOTE_GPU, flags=0)
    opt = RemoteEmbeddingAdam(emb, lr=1e-2, betas=(0.8, 0.99), eps=1e-6)
    table, state = fake.made
    bf16 = dtype == torch.bfloat16
    tab = rows * dim * 4
    assert state.kw == table.kw and state.remote_bytes == (3 if bf16 else 2) * tab
    assert opt.off == ({"m": 0, "v": tab, "w": 2 * tab} if bf16 else {"m": 0, "v": tab})
    # the state starts zeroed, chunk by chunk; the master as the table's rows, widened
    zeroed = sorted((ro, n) for lo, ro, n, data in state.puts if not data.any())
    assert sum(n for _, n in zeroed) == 2 * tab and zeroed[0][0] == 0
    if bf16:
        masters = [(ro, data) for lo, ro, n, data in state.puts if data.any()]
        assert sum(d.numel() for _, d in masters) == tab and min(ro for ro, _ in masters) == 2 * tab
        assert bool((masters[0][1].view(torch.float32) == 0.74609375).all())
    ids = torch.tensor([[7, 3], [7, 49]], dtype=torch.int32)
    g = torch.arange(4 * dim, dtype=torch.float32).view(4, dim) / 8
    opt.step(ids, g, scale=0.5)
    opt.step(torch.tensor([5], dtype=torch.int64), g[:1])
    first, second = table.calls
    # duplicate ids reach the call once, with summed gradients, in the table's dtype
    assert first["ids"].tolist() == [3, 7, 49] and first["ids"].dtype == torch.int32
    want = torch.stack([g[1], g[0] + g[2], g[3]]).to(dtype)
    assert first["grad"].dtype == dtype and torch.equal(first["grad"], want)
    assert first["state"] is state and first["rows"] == rows and first["gscale"] == 0.5 and second["gscale"] == 1.0
    assert first["table"] == (0, dim * (2 if bf16 else 4))
    assert first["m"] == (0, 4 * dim) and first["v"] == (tab, 4 * dim) and first["w"] == ((2 * tab, 4 * dim) if bf16 else None)
    # the bias corrections follow the global step count; no decay of either kind
    assert opt.t == 2 and first["hp"][4] == 1e-2 / (1 - 0.8) and second["hp"][4] == 1e-2 / (1 - 0.8 ** 2)
    assert second["hp"][5] == 1 / math.sqrt(1 - 0.99 ** 2) and first["hp"][3] == 0.0 and len(first["hp"]) == 6
    assert second["ids"].dtype == torch.int64
    # a sparse COO gradient, as nn.Embedding(sparse=True) makes it: coalesced, the same call
    sp = torch.sparse_coo_tensor(ids.reshape(1, -1).long(), g, (rows, dim))
    opt.step(sp)
    third = table.calls[2]
    assert third["ids"].tolist() == [3, 7, 49] and torch.equal(third["grad"], want) and opt.t == 3
    # nothing to do: no call, and the step does not count
    opt.step(torch.zeros(0, dtype=torch.int64), g[:0])
    assert opt.t == 3 and len(table.calls) == 3
    with pytest.raises(ValueError):
        opt.step(ids, g[:3])
    with pytest.raises(TypeError):
        opt.step(ids.float(), g)
    assert opt.t == 3 and len(table.calls) == 3


def test_fp16_and_weight_decay_are_refused():
    fake = _FakeClient()
    emb = RemoteEmbedding(fake, 8, 4, max_ids=4)  # the default dtype: float16
    with pytest.raises(TypeError, match="float16"):
        RemoteEmbeddingAdam(emb)
    emb32 = RemoteEmbedding(fake, 8, 4, dtype=torch.float32, max_ids=4)
    with pytest.raises(ValueError, match="weight decay"):
        RemoteEmbeddingAdam(emb32, weight_decay=0.01)
    assert len(fake.made) == 2  # no state pair was made for either


# ---- the hook on a CPU mesh ----

def test_hook_needs_a_gpu_and_changes_nothing(mesh_factory, monkeypatch):
    monkeypatch.setenv("OCM_NO_GPU", "1")
    m = mesh_factory(2)
    with api.Client(daemon_rank=0, ns=m.ns) as c:
        a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=1 << 16, remote_bytes=1 << 16)
        try:
            img = torch.arange(1 << 14, dtype=torch.int32)
            write_remote(a, 0, 0, img)
            ids = torch.tensor([1, 2], dtype=torch.int64)
            g = torch.ones(2, 8)
            hp, _ = hyper(HP_NAME)
            for khp, gscale in ((kernel_hp_rows(hp, 1), 1.0), ((0.9, 0.999, 1e-8, 0.01, 1e-3, 1.0), 1.0)):
                with pytest.raises(api.OcmError, match="needs a GPU"):
                    a.adam_rows(a, ids, g, (0, 32), (4096, 32), (8192, 32), khp, 16, gscale=gscale, stream=0)
            # the raw hook, null arguments: refused as such
            rc = api.load().ocm_x_adam_rows(a.handle, a.handle, None, None, None, (ctypes.c_float * 9)(), 1.0, None, None)
            assert rc != 0 and "null argument" in api.last_error()
            assert torch.equal(read_remote(a, 0, 0, 1 << 16).view(torch.int32), img)
        finally:
            a.free()


def test_binding_layout():
    assert ctypes.sizeof(api.OcmAdamRows) == 104  # static_assert in ocm/adam_rows.h
    assert np.dtype(np.uint64).itemsize * 3 == api.OcmAdamRows.index_type.offset
