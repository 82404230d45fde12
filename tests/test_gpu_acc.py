"""One-sided accumulate on the gfx950 kernel path (csrc/src/kernels/xfer_acc.hip): the
accumulators bit for bit against the torch oracle, with the pool in the pinned host tier
(one daemon) and striped over three owners (four daemons)."""
import numpy as np
import pytest
import torch

from acc_cases import DTYPES, UNIT, AccList, assert_bits, exercise_grad_accumulator, random_elems, run_edge_vectors
from oncilla_amd import api
from oncilla_amd.models import OffloadedGradAccumulator
from oncilla_amd.ops import accumulate_reference
from quant_cases import read_local, read_remote, write_local, write_remote

pytestmark = pytest.mark.gpu

N_DAEMONS = [1, 4]  # 1: pool in the pinned host tier; 4: striped over 3 peers' HBM


def _client(mesh_factory, n_daemons):
    m = mesh_factory(n_daemons, gpus=[0] * n_daemons, policy="stripe")
    return api.Client(daemon_rank=0, gpu=0, ns=m.ns)


def _pair(c, local_bytes, remote_bytes, kind=api.OCM_REMOTE_GPU):
    return c.alloc(kind, local_bytes=local_bytes, remote_bytes=remote_bytes, flags=api.OCM_ALLOC_STRIPE, stripe_unit=UNIT)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_edge_vectors(mesh_factory, n_daemons, dtype):
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 8192, 4 * UNIT)
        run_edge_vectors(a, dtype, stage=4096)
        a.free()


@pytest.mark.parametrize("async_", [False, True])
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_sixty_op_list(mesh_factory, n_daemons, async_):
    al = AccList()
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, al.local_bytes, al.remote_bytes)
        assert len(a.remote_info()["extents"]) == (1 if n_daemons == 1 else 3)
        before = api.acc_counters()
        al.run(a, async_=async_)  # async: followed by wait
        after = api.acc_counters()
        assert after["n_acc"] == before["n_acc"] + 1 and after["n_acc_ops"] == before["n_acc_ops"] + 60
        assert after["bytes_acc"] == before["bytes_acc"] + 4 * al.elems
        a.free()


def _sizes_with_empties(n_ops, most):
    # ops of no elements have no tiles: first, last, two in a row and between the others
    return [0 if i in (0, 3, 4, n_ops - 1) or i % 9 == 8 else 4 * (1 + (i * 61) % most) for i in range(n_ops)]


@pytest.mark.parametrize("n_ops", [7, 53])  # in the kernel arguments; uploaded, with a wave table
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_empty_ops_among_others(mesh_factory, n_daemons, n_ops):
    _run_sized_list(mesh_factory, n_daemons, _sizes_with_empties(n_ops, 400))


@pytest.mark.parametrize("n_ops", [48, 49])  # the most ops the kernel arguments hold, and one more
@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_list_at_the_inline_capacity(mesh_factory, n_daemons, n_ops):
    sizes = _sizes_with_empties(n_ops, 375)  # 4 to 1500 elements: one tile or two
    sizes[1], sizes[2] = 4, 1500
    assert max(sizes) == 1500 and min(s for s in sizes if s) == 4 and sizes.count(0) >= 4
    _run_sized_list(mesh_factory, n_daemons, sizes)


def _run_sized_list(mesh_factory, n_daemons, sizes):
    n_ops = len(sizes)
    slot, rslot, dtype = 4096, 2 * UNIT, torch.bfloat16  # bytes per op in the local and in the remote half (<= 1600 elements)
    with _client(mesh_factory, n_daemons) as c:
        stage = n_ops * slot
        a = _pair(c, stage + n_ops * rslot, n_ops * rslot)
        model = torch.full((n_ops * rslot,), 0xA5, dtype=torch.uint8)
        want, rows = model.clone(), []
        for i, n in enumerate(sizes):
            lo, ro = i * slot, i * rslot + 16 * (i % 3)
            assert 2 * n <= slot and 4 * n + 32 <= rslot
            rows.append([lo, ro, n, api.acc_dtype(dtype), 0.5 + i])
            if n:
                acc, x = random_elems(n, torch.float32, 700 + i), random_elems(n, dtype, 800 + i)
                write_local(a, lo, x)
                model[ro:ro + 4 * n] = acc.view(torch.uint8)
                want[ro:ro + 4 * n] = accumulate_reference(acc, x, 0.5 + i).view(torch.uint8)
        write_remote(a, stage, 0, model)
        before = api.acc_counters()
        a.accumulate_batch(np.array(rows, dtype=np.float64))
        after = api.acc_counters()
        assert after["n_acc_ops"] == before["n_acc_ops"] + n_ops
        assert after["bytes_acc"] == before["bytes_acc"] + 4 * sum(sizes)
        assert torch.equal(read_remote(a, stage, 0, n_ops * rslot), want)
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_host_path_matches_kernel_path(mesh_factory, n_daemons):
    n = 4 * 1300  # five full tiles and a partial one, across two stripe-unit boundaries
    with _client(mesh_factory, n_daemons) as c:
        for dtype in DTYPES:
            esize = torch.empty((), dtype=dtype).element_size()
            acc, x = random_elems(n, torch.float32, seed=41), random_elems(n, dtype, seed=42)
            stage = 2 * UNIT * esize
            lb, roff = stage + 4 * n, UNIT - 48
            h = _pair(c, lb, 8 * UNIT, kind=api.OCM_REMOTE_RDMA)  # host local half: the rule on the CPU
            d = _pair(c, lb, 8 * UNIT)                            # device local half: the kernel
            got = []
            for a in (h, d):
                write_local(a, 0, x)
                write_remote(a, stage, roff, acc)
                a.accumulate_batch(np.array([[0, roff, n]]), dtype, 1.0 / 3.0)
                got.append(read_remote(a, stage, roff, 4 * n).view(torch.float32))
            assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32)), dtype
            assert_bits(got[1], accumulate_reference(acc, x, 1.0 / 3.0), str(dtype))
            h.free()
            d.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_two_async_accumulates_then_a_get_are_ordered(mesh_factory, n_daemons):
    n, dtype = 4 * 2500, torch.bfloat16
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 4 * n + 4 * n, 12 * UNIT)
        acc, x = random_elems(n, torch.float32, seed=51), random_elems(2 * n, dtype, seed=52)
        roff, stage = UNIT + 16, 4 * n
        write_local(a, 0, x)
        write_remote(a, stage, roff, acc)
        # no host sync between the three: the second reads what the first wrote, the get what both did
        a.accumulate_batch(np.array([[0, roff, n]]), dtype, 0.1, async_=True)
        a.accumulate_batch(np.array([[2 * n, roff, n]]), dtype, -3.0, async_=True)
        a.get(stage, roff, 4 * n, async_=True)  # queued on the lane behind them, no host wait before it
        a.wait()
        got = read_local(a, stage, 4 * n).view(torch.float32)
        want = accumulate_reference(accumulate_reference(acc, x[:n], 0.1), x[n:], -3.0)
        assert_bits(got, want, "two accumulates")
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_async_accumulate_on_a_side_stream(mesh_factory, n_daemons):
    n, dtype = 4 * 3000, torch.float16
    with _client(mesh_factory, n_daemons) as c:
        a = _pair(c, 2 * n + 4 * n, 16 * UNIT)
        acc, x = random_elems(n, torch.float32, seed=61), random_elems(n, dtype, seed=62)
        roff, stage = 2 * UNIT - 16, 2 * n
        write_remote(a, stage, roff, acc)
        xd = x.to("cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            lt = a.local_tensor(dtype)
            lt[:n].copy_(xd)  # torch fills the local half on the side stream; the list must start after it
            a.stream_wait()
            a.accumulate_batch(np.array([[0, roff, n]]), dtype, -0.5, async_=True)
            a.stream_signal()
            lt[:n].fill_(7.0)  # queued after the accumulate: it must not change the result
        side.synchronize()
        a.wait()
        got = read_remote(a, stage, roff, 4 * n).view(torch.float32)
        assert_bits(got, accumulate_reference(acc, x, -0.5), "side stream")
        a.free()


@pytest.mark.parametrize("n_daemons", N_DAEMONS)
def test_grad_accumulator_gpu(mesh_factory, n_daemons):
    torch.manual_seed(n_daemons)
    with _client(mesh_factory, n_daemons) as c:
        model = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.GELU(), torch.nn.Linear(96, 10)).to("cuda:0", torch.bfloat16)
        params = list(model.parameters())
        acc = OffloadedGradAccumulator(params, c, stripe_unit=UNIT)
        assert len(acc.alloc.remote_info()["extents"]) == (1 if n_daemons == 1 else 3)
        scales = [1.0, 0.25, 1.0 / 3.0, 0.5]
        want = [torch.zeros(p.shape, dtype=torch.float32) for p in params]
        for m, scale in enumerate(scales):
            x = torch.randn(32, 64, device="cuda:0", dtype=torch.bfloat16)
            acc.zero_grads()
            model(x).float().square().mean().backward()
            assert all(p.grad.data_ptr() >= acc.alloc.local_tensor().data_ptr() for p in params)  # still the views
            grads = [p.grad.detach().cpu().clone() for p in params]  # a host sync: test bookkeeping only
            assert any(g.abs().sum() > 0 for g in grads)
            assert acc.add(scale=scale, async_=bool(m % 2)) == 1  # one dtype: a single op
            want = [accumulate_reference(w, g, scale) for w, g in zip(want, grads)]
        for k, (g, w) in enumerate(zip(acc.read(), want)):
            assert_bits(g.cpu(), w, f"parameter {k}")
        acc.zero()
        assert all(not g.cpu().view(torch.int32).any() for g in acc.read())
        acc.close()
