"""bench.py contract on CPU (1 rank, and 2 ranks under torch.distributed.run/gloo)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_bench_single(native):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--device", "cpu", "--steps", "2", "--warmup",
                        "1", "--max-bytes", str(1 << 20), "--alloc-samples", "20"], capture_output=True, text=True,
                       timeout=300, cwd="/tmp")
    assert r.returncode == 0, r.stderr
    res = _last_json(r.stdout)
    assert KEYS <= set(res) and res["n_gpus"] == 1 and res["value"] > 0
    assert res["alloc_p50_us"] > 0 and res["config"]["remote_tier"] == "host"


def _pattern_bytes(seed, nbytes):
    """The library's word pattern (what Allocation.fill writes), computed on the host."""
    import ctypes

    import numpy as np

    from oncilla_amd import api

    buf = np.zeros(nbytes, dtype=np.uint8)
    assert api.load().ocm_x_pattern(ctypes.c_void_p(buf.ctypes.data), nbytes // 4, 0, seed, 0) == 0
    return buf


def _bench_dump(out_dir, max_bytes, device_args, extra=()):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *device_args, "--steps", "2", "--warmup", "1",
                        "--max-bytes", str(max_bytes), "--alloc-samples", "10", "--dump-outputs", str(out_dir), *extra],
                       capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-4000:]
    return _last_json(r.stdout)


def check_dump(out_dir, max_bytes, res):
    """--dump-outputs of a 1-rank run: float32 .npy files within 64 MB, the last get's and
    the last put's bytes at the recorded offsets, both equal to the pattern the bench
    filled the pair with (seed 1234 + rank)."""
    import numpy as np

    files = sorted(os.listdir(out_dir))
    assert files == ["local_rank0.npy", "offsets_rank0.npy", "remote_rank0.npy"], files
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64_000_000
    arrs = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert arrs["local_rank0"].dtype == arrs["remote_rank0"].dtype == np.float32
    assert arrs["offsets_rank0"].dtype == np.float64
    offs = arrs["offsets_rank0"].astype(np.int64)
    assert 0 < len(offs) <= 1 << 21 and offs[0] == 0 and offs[-1] < max_bytes and np.all(np.diff(offs) > 0)
    want = _pattern_bytes(1234, max_bytes)[offs].astype(np.float32)
    assert np.array_equal(arrs["local_rank0"], want) and np.array_equal(arrs["remote_rank0"], want)
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    return arrs


def test_bench_dump_outputs_and_plain_run(native, tmp_path):
    """A plain run times its steps and stops: none of the --full measurements in its line.
    --dump-outputs writes the same arrays on every run with the same arguments (every byte
    at 1 MiB; a seeded sample with every size's end at 4 MiB), --full or not."""
    import numpy as np

    a = _bench_dump(tmp_path / "a", 1 << 20, ["--device", "cpu"])
    assert KEYS <= set(a) and a["value"] > 0 and a["sweep"] == {} and "idle_gap_4k" not in a, a
    assert a["config"]["full"] is False
    arrs = check_dump(tmp_path / "a", 1 << 20, a)
    assert len(arrs["offsets_rank0"]) == 1 << 20
    b = _bench_dump(tmp_path / "b", 4 << 20, ["--device", "cpu"])
    c = _bench_dump(tmp_path / "c", 4 << 20, ["--device", "cpu"], extra=["--full"])
    assert b["sweep"] == {} and c["config"]["full"] is True
    assert sorted(c["sweep"]) == sorted(str(4096 << k) for k in range(11)) and "idle_gap_4k" in c, c
    arrs_b, arrs_c = check_dump(tmp_path / "b", 4 << 20, b), check_dump(tmp_path / "c", 4 << 20, c)
    offs = set(arrs_b["offsets_rank0"].astype(np.int64).tolist())
    assert len(offs) < 4 << 20 and {0, 4095, 4096, (2 << 20) - 1, 2 << 20, (4 << 20) - 1} <= offs
    for k in arrs_b:
        assert np.array_equal(arrs_b[k], arrs_c[k]), k


# "ticks": the main mesh's records ride tick collectives as they would over RCCL on a
# GPU node (--ctrl auto with the socket stand-in), device-sealed and queued 4 at a time
TICK_ENV = {"OCM_CTRL_AUTO_SOCKET": "1", "OCM_TICK_SOCKET_SEAL": "1", "OCM_TICK_SOCKET_BATCH": "4"}


@pytest.mark.parametrize("n,mode", [(2, "tcp"), (8, "tcp"), (8, "ticks"), (8, "embedded")])
def test_bench_multi_rank(native, n, mode):
    # the driver's multi-GPU launch shape (torch.distributed.run, one daemon per rank), on gloo + CPU daemons;
    # "embedded": each rank's daemon on a thread of the rank's process (the bench default on GPUs),
    # records on tick collectives, stream placement live
    env = dict(os.environ, **(TICK_ENV if mode in ("ticks", "embedded") else {}))
    env["OCM_BENCH_DAEMONS"] = "embedded" if mode == "embedded" else "process"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
                        "--master-addr", "127.0.0.1", "--master-port", str(29533 + n + {"tcp": 0, "ticks": 1, "embedded": 2}[mode]),
                        os.path.join(REPO, "bench.py"),
                        "--gpus", str(n), "--device", "cpu", "--steps", "2", "--warmup", "1", "--max-bytes",
                        str(4 << 20), "--alloc-samples", "20", "--full"], capture_output=True, text=True, timeout=300,
                       cwd="/tmp", env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-8000:]  # the ranks' tracebacks precede torchrun's summary
    res = _last_json(r.stdout)
    assert res["n_gpus"] == n and res["value"] > 0 and res["config"]["parallelism"] == f"stripe{n}"
    assert res["config"]["extents_per_pair"] == n - 1  # 8 MiB+1 pair = 9 stripe units: every peer gets one
    # the setup-time autotune ran its all-rank protocol and agreed on one pick per direction
    assert res["autotune"]["ranks"] == n and res["autotune"]["get"] in res["autotune"]["GiBps"], res["autotune"]
    assert len(res["alloc_p50_us_per_rank"]) == n
    # self-diagnosis: every rank reports its data-path state and control transport;
    # CPU ranks move no byte over xGMI, so the flag must say so
    assert res["xgmi"] is False and len(res["ranks"]) == n, res.get("ranks")
    assert all(d["ctrl"] in ("tcp", "socket", "rccl") and d["peer_access"] == 0 for d in res["ranks"]), res["ranks"]
    if mode in ("ticks", "embedded"):
        assert all(d["ctrl"] == "socket" for d in res["ranks"]), res["ranks"]
    assert res["config"]["daemons"] == ("embedded" if mode == "embedded" else "process")
    # control-plane extra: the same allocation path on TCP links and on socket-collective ticks
    cp = res["control_plane"]
    assert "alloc_p50_us" in cp["tcp"] and "alloc_p50_us" in cp["socket"], cp
    assert cp["tcp"]["alloc_p50_us"] > 0 and cp["tcp"]["ticks_rank0"] == 0, cp
    assert cp["socket"]["alloc_p50_us"] > 0 and cp["socket"]["ticks_rank0"] > 0, cp
    # per-rank hop latency of the tick transport (api.tick_stats on every rank; a rank
    # that posted nothing through the ticks has none)
    hops = cp["socket"]["hop_mean_us_per_rank"]
    assert len(hops) == n and all(h is None or h > 0 for h in hops) and any(hops), cp
    assert cp["socket"]["start_mean_us_rank0"] > 0, cp
    # idle ticks: the socket control plane woke nobody over TCP
    assert cp["socket"]["tcp_wakes_all_ranks"] == 0 and cp["socket"]["idle_ticks_rank0"] > 0, cp
    # every measured allocation was placed from the stream (two hops)
    assert cp["socket"]["allocs_three_hop_all_ranks"] == 0 and cp["socket"]["rank0_do_allocs"] == 0, cp
    assert cp["socket"]["allocs_two_hop_all_ranks"] >= cp["socket"]["samples_per_rank"], cp
    assert cp["socket"]["stream_placement_rank0"] == "live" and cp["socket"]["replica_digests_equal"] is True, cp


def test_bench_extras_helpers_run(native):
    # The N>1 extras only run on multi-GPU nodes (the driver's scaling run):
    # exercise their code here so a Python error cannot hide until then.
    sys.path.insert(0, REPO)
    import bench

    b = bench.hw_baseline_extras(None, 2, 0, 0)
    assert isinstance(b, dict)
    assert bench._local(lambda: 1 / 0)[1].startswith("ZeroDivisionError")


class RoundTrip:
    """The data path of a fake pair for autotune's per-candidate verification: a
    pattern seed travels local -> remote -> local; `corrupt(cfg)` spoils a put."""
    corrupt = staticmethod(lambda cfg: False)

    def fill(self, seed, offset=0, nbytes=None):
        self.local = seed

    def put(self, lo, ro, n):
        self.remote = -1 if self.corrupt(self.cur[1]) else self.local

    def get(self, lo, ro, n):
        self.local = self.remote

    def check(self, seed, offset=0, nbytes=None):
        return 0 if self.local == seed else 17


def test_autotune_picks_fastest_by_slowest_rank(native, monkeypatch):
    """workloads.autotune: per-direction pick by the slowest rank, failing candidates
    excluded, and the same number of collectives on every path (no deadlock)."""
    from oncilla_amd import api
    from oncilla_amd.models import workloads as wl

    cur = {}
    monkeypatch.setattr(api, "set_tuning_dir", lambda op, v, b, nt: cur.__setitem__(op, (v, b, nt)))
    # seconds per (variant, blocks, nt, op) on this rank; the "other rank" is 2x slower on reg_b256 puts
    cands = {"auto": (0, 0, 1), "reg_b256": (1, 256, 1), "lds_default": (2, 0, 1), "broken": (1, 64, 0)}
    mine = {(0, 0, 1): (3.0, 3.0), (1, 256, 1): (2.0, 1.0), (2, 0, 1): (1.5, 2.5)}

    class FakePair(RoundTrip):
        last = None

        def time_onesided(self, op, n, iters):
            cfg = self.last = cur[op]
            if cfg == (1, 64, 0):
                raise RuntimeError("launch failed")
            return mine[cfg][op]

    pair = FakePair()
    pair.cur = cur
    calls = []

    def gather(obj):  # two ranks; the other one is 4x slower with reg_b256
        calls.append(obj)
        if isinstance(obj, tuple) and obj[0] is not None and pair.last == (1, 256, 1):
            return [obj, (obj[0] * 4.0, None)]
        return [obj, obj]

    r = wl.autotune(pair, 1 << 20, gather=gather, candidates=cands)
    assert r["get"] == "lds_default", r
    assert r["put"] == "lds_default", r  # reg_b256 is fastest here but not on the other rank
    assert "error" in r["GiBps"]["broken"]["get"] and "error" in r["GiBps"]["broken"]["put"]
    # 2 gathers per (candidate, direction), 1 for its verification, 1 for the rank count
    assert len(calls) == (2 * 2 + 1) * len(cands) + 1
    assert cur[0] == cands[r["get"]] and cur[1] == cands[r["put"]]


@pytest.mark.parametrize("daemons", ["process", "embedded"])
@pytest.mark.parametrize("inject", [("OCM_BENCH_RAISE", "5:verify"), ("OCM_BENCH_FAULT", "3:crash_after_allocs=0")])
def test_bench_eight_ranks_fail_fast(native, inject, daemons):
    """A failure on one of 8 ranks (a raised phase, or its daemon dying at the
    first DO_ALLOC) ends every rank within the bound: non-zero exit, and rank 0
    prints one JSON line naming the phase and the failing ranks' messages."""
    import time

    env = dict(os.environ, OCM_BENCH_TIMEOUT_S="90", OCM_BENCH_DAEMONS=daemons, **{inject[0]: inject[1]})
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8",
                        "--master-addr", "127.0.0.1", "--master-port", str(29561 + len(inject[1]) + 40 * (daemons == "embedded")),
                        os.path.join(REPO, "bench.py"), "--gpus", "8", "--device", "cpu", "--steps", "1", "--warmup",
                        "1", "--max-bytes", str(1 << 20), "--alloc-samples", "10"], capture_output=True, text=True,
                       timeout=280, cwd="/tmp", env=env)
    assert time.time() - t0 < 270
    assert r.returncode != 0
    res = _last_json(r.stdout)
    assert res["value"] is None and res["error"] and res["rank_errors"], res
    if inject[0] == "OCM_BENCH_RAISE":
        assert res["phase"] == "verify" and list(res["rank_errors"]) == ["5"]


@pytest.mark.parametrize("phase", ["verify", "alloc_latency"])
def test_bench_falls_back_to_host_tier_when_peer_hbm_fails(native, phase):
    """--device gpu paths cannot run here, so drive the fallback on CPU ranks by
    injecting a failure into the first run of a phase: the bench redoes it with the
    remote halves in the host tier and still reports a measured value, with the
    fallback recorded."""
    env = dict(os.environ, OCM_BENCH_RAISE_ONCE=f"1:{phase}")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(29591 + len(phase)), os.path.join(REPO, "bench.py"),
                        "--gpus", "2", "--device", "cpu", "--steps", "1", "--warmup", "1", "--max-bytes",
                        str(1 << 20), "--alloc-samples", "10"], capture_output=True, text=True, timeout=300,
                       cwd="/tmp", env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = _last_json(r.stdout)
    assert res["value"] > 0 and res["fallback"]["phase"] == phase and list(res["fallback"]["rank_errors"]) == ["1"]
    assert res["xgmi"] is False  # a fallback is never an xGMI number


def test_autotune_never_installs_the_dma_baseline(native, monkeypatch):
    """the runtime's copy engines stay a reported baseline. Even when
    "dma" is the fastest candidate, a kernel configuration is installed."""
    from oncilla_amd import api
    from oncilla_amd.models import workloads as wl

    cur = {}
    monkeypatch.setattr(api, "set_tuning_dir", lambda op, v, b, nt: cur.__setitem__(op, (v, b, nt)))
    cands = {"auto": (0, 0, 1), "reg_b256": (1, 256, 1), "dma": (3, 0, 1)}
    secs = {(0, 0, 1): 2e-4, (1, 256, 1): 1.5e-4, (3, 0, 1): 1e-4}

    class FakePair(RoundTrip):
        cur = None

        def time_onesided(self, op, n, iters):
            return secs[cur[op]]

    pair = FakePair()
    pair.cur = cur
    r = wl.autotune(pair, 1 << 20, candidates=cands)
    assert r["get"] == "reg_b256" and r["put"] == "reg_b256", r
    assert r["baselines"] == ["dma"] and r["GiBps"]["dma"]["get"] > r["GiBps"]["reg_b256"]["get"], r
    assert cur[0] == (1, 256, 1) and cur[1] == (1, 256, 1)


def test_autotune_drops_a_fast_candidate_that_corrupts_data(native, monkeypatch):
    """The fastest candidate whose round trip comes back wrong (on one rank only)
    is reported as an error and never installed."""
    from oncilla_amd import api
    from oncilla_amd.models import workloads as wl

    cur = {}
    monkeypatch.setattr(api, "set_tuning_dir", lambda op, v, b, nt: cur.__setitem__(op, (v, b, nt)))
    cands = {"auto": (0, 0, 1), "fast_but_wrong": (5, 0, 1), "reg_b256": (1, 256, 1)}
    secs = {(0, 0, 1): 2e-4, (1, 256, 1): 1.5e-4, (5, 0, 1): 0.5e-4}

    class FakePair(RoundTrip):
        def time_onesided(self, op, n, iters):
            return secs[cur[op]]

    pair = FakePair()
    pair.cur = cur
    pair.corrupt = staticmethod(lambda cfg: cfg == (5, 0, 1))

    def gather(obj):  # rank 1 agrees on timings; its verification is the same as ours
        return [obj, obj]

    r = wl.autotune(pair, 1 << 20, gather=gather, candidates=cands)
    assert r["get"] == "reg_b256" and r["put"] == "reg_b256", r
    assert "verification" in r["GiBps"]["fast_but_wrong"]["get"]["error"], r


def _fake_autotune(monkeypatch, secs, cands, gather=None):
    """autotune over a fake pair whose per-config seconds come from secs[(cfg, op)] or secs[cfg]."""
    from oncilla_amd import api
    from oncilla_amd.models import workloads as wl

    cur = {}
    monkeypatch.setattr(api, "set_tuning_dir", lambda op, v, b, nt: cur.__setitem__(op, (v, b, nt)))

    class FakePair(RoundTrip):
        def time_onesided(self, op, n, iters):
            v = secs[cur[op]]
            return v[op] if isinstance(v, tuple) else v

    pair = FakePair()
    pair.cur = cur
    return wl.autotune(pair, 1 << 20, gather=gather, candidates=cands), cur


def test_autotune_keeps_auto_within_the_margin(native, monkeypatch):
    """candidates within 3 % of auto (noise at 5 reps) never
    replace it; one that is 10 % faster on every rank does; the margins are recorded."""
    cands = {"auto": (0, 0, 1), "reg_b256": (1, 256, 1), "lds_default": (2, 0, 1)}
    # get: both candidates 2 % faster (a tie); put: lds_default 10 % faster
    secs = {(0, 0, 1): (1.0, 1.0), (1, 256, 1): (0.98, 0.985), (2, 0, 1): (0.98, 0.90)}
    r, cur = _fake_autotune(monkeypatch, secs, cands)
    assert r["get"] == "auto" and r["put"] == "lds_default", r
    assert r["margin_required"] == 0.03 and r["reps"] == 5
    assert abs(r["margins"]["get"]["reg_b256"] - 0.02) < 1e-6 and abs(r["margins"]["put"]["lds_default"] - 0.1) < 1e-6
    assert cur[0] == (0, 0, 1) and cur[1] == (2, 0, 1)


def test_autotune_needs_the_margin_on_every_rank(native, monkeypatch):
    """A candidate 20 % faster on rank 0 but only 1 % faster on rank 1 keeps auto."""
    cands = {"auto": (0, 0, 1), "reg_b256": (1, 256, 1)}
    secs = {(0, 0, 1): 1.0, (1, 256, 1): 0.8}

    def gather(obj):  # rank 1: reg_b256 is 0.99 of auto there
        if isinstance(obj, tuple) and obj[0] == 0.8:
            return [obj, (0.99, None)]
        return [obj, obj]

    r, _ = _fake_autotune(monkeypatch, secs, cands, gather=gather)
    assert r["get"] == "auto" and r["put"] == "auto", r
    assert abs(r["margins"]["get"]["reg_b256"] - 0.01) < 1e-6, r["margins"]


def test_autotune_never_installs_a_get_only_variant_for_puts(native, monkeypatch):
    """Push-based gets (variant 5) compete for gets only; their 'put' is auto's path."""
    cands = {"auto": (0, 0, 1), "push": (5, 0, 1), "reg_b256": (1, 256, 1)}
    secs = {(0, 0, 1): 1.0, (5, 0, 1): 0.5, (1, 256, 1): 0.9}
    r, _ = _fake_autotune(monkeypatch, secs, cands)
    assert r["get"] == "push" and r["put"] == "reg_b256", r
    assert "push" not in r["margins"]["put"], r["margins"]


def test_push_candidates_are_opt_in(monkeypatch):
    """push-based gets stay out of the default candidates until a
    multi-GPU box has run them (OCM_AUTOTUNE_PUSH=1 opts in)."""
    from oncilla_amd.models import workloads as wl

    monkeypatch.delenv("OCM_AUTOTUNE_PUSH", raising=False)
    assert not any(v[0] == 5 for v in wl.default_candidates().values())
    monkeypatch.setenv("OCM_AUTOTUNE_PUSH", "1")
    assert {"push", "push_b1024"} <= set(wl.default_candidates())


def test_idle_gap_rows_merge_ragged_ranks():
    # Relaunch timings exist only on ranks that relaunched: a merge keyed on one rank's
    # row raised on some ranks and not others, which then waited in different
    # collectives (found in the 8-rank one-GPU rehearsal with HIP lanes).
    from oncilla_amd.models import workloads as wl

    a = {"0": {"get_p50_us": 5.0, "get_relaunches": 0}, "1000": {"get_p50_us": 6.0, "get_relaunches": 2,
                                                              "get_relaunch_host_us": 3.0}}
    b = {"0": {"get_p50_us": 5.5, "get_relaunches": 0}, "1000": {"get_p50_us": 6.5, "get_relaunches": 0}}
    for order in ([a, b], [b, a]):
        m = wl.merge_idle_gap_rows(order)
        assert m["0"] == {"get_p50_us": 5.5, "get_relaunches": 0}
        assert m["1000"] == {"get_p50_us": 6.5, "get_relaunches": 2, "get_relaunch_host_us": 3.0}
        assert list(m) == ["0", "1000"]


def test_idle_gap_rows_merge_cold_splits():
    # Round 5: a relaunched op's cold-start split is a dict per row; with two ranks that
    # both relaunched, max() over dicts raised (TypeError) and would have ended an N>1
    # bench at its idle-gap rows. Each stage merges to its slowest rank, `ops` sums.
    from oncilla_amd.models import workloads as wl

    a = {"10000": {"get_p50_us": 17.0, "get_cold_split_us": {"dispatch_to_start": 9.0, "start_to_seen": 2.0,
                                                             "total": 17.0, "ops": 30}}}
    b = {"10000": {"get_p50_us": 18.0, "get_cold_split_us": {"dispatch_to_start": 8.5, "start_to_seen": 2.5,
                                                             "total": 18.0, "ops": 28}}}
    c = {"10000": {"get_p50_us": 6.0}}
    for order in ([a, b, c], [c, b, a]):
        m = wl.merge_idle_gap_rows(order)
        assert m["10000"]["get_p50_us"] == 18.0
        assert m["10000"]["get_cold_split_us"] == {"dispatch_to_start": 9.0, "ops": 58, "start_to_seen": 2.5,
                                                   "total": 18.0}


def test_bench_ranks_started_without_torchrun(native, tmp_path):
    # tools/launch_ranks.sh: the one-GPU 8-rank rehearsal starts its ranks from a
    # shell loop (no Python parent with the GPU open); the env:// rendezvous and the
    # JSON line on rank 0's stdout must be the same as under torchrun.
    r = subprocess.run(["bash", os.path.join(REPO, "tools", "launch_ranks.sh"), "2", "29597",
                        os.path.join(REPO, "bench.py"), "--gpus", "2", "--device", "cpu", "--steps", "1", "--warmup",
                        "1", "--max-bytes", str(1 << 20), "--alloc-samples", "10", "--no-ctrl-extra"],
                       capture_output=True, text=True, timeout=300, cwd="/tmp",
                       env=dict(os.environ, RANKLOG_DIR=str(tmp_path)))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-8000:] + (tmp_path / "rank1.log").read_text()[-1500:]
    res = _last_json(r.stdout)
    assert res["n_gpus"] == 2 and res["value"] > 0 and len(res["ranks"]) == 2, res
    assert (tmp_path / "rank1.log").exists()
