"""The driver's multi-rank launch rehearsed on ONE MI355X (every rank and daemon on
GPU 0, OCM_BENCH_SHARE_GPU=1): several processes' copy services, launches and
daemons share the GPU, the condition under which round 3's gang completion
stalled for 10 s. The run must be clean: every
rank's copy service without a timeout, and no library warning on any rank."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("daemons", ["embedded", "process"])
def test_shared_gpu_rehearsal_is_clean(daemons):
    # embedded (the bench's default): each rank's daemon on a thread of the rank's process; process: a
    # daemon process per rank
    env = dict(os.environ, OCM_BENCH_SHARE_GPU="1", OCM_BENCH_TIMEOUT_S="90", OCM_BENCH_DAEMONS=daemons)
    log = os.path.join(REPO, "gpurun_out", f"test_gpu_share_{daemons}.log")
    os.makedirs(os.path.dirname(log), exist_ok=True)
    with open(log, "w") as lf:
        # the output goes to a file (kept under gpurun_out/): a hang leaves the phase it stopped in
        p = subprocess.Popen([sys.executable, "-u", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
                              "4", "--master-addr", "127.0.0.1", "--master-port", "29681",
                              os.path.join(REPO, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1",
                              "--max-bytes", str(64 << 20), "--alloc-samples", "50", "--full", "--no-ctrl-extra",
                              "--no-hw-baseline", "--no-optim-extra"],
                             stdout=lf, stderr=subprocess.STDOUT, text=True, cwd="/tmp", env=env,
                             start_new_session=True)
        try:
            rc = p.wait(timeout=120)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, 9)
            p.wait(timeout=30)
            raise AssertionError("the rehearsal did not finish in 120 s: " + open(log).read()[-3000:])
    out = open(log).read()
    assert rc == 0, out[-4000:]
    res = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
    print(json.dumps({k: res.get(k) for k in ("value", "service_clean", "xgmi")}),
          [d.get("service") for d in res["ranks"]])
    assert res["n_gpus"] == 4 and res["value"] > 0 and res["xgmi"] is False, res
    assert res["config"]["daemons"] == daemons, res["config"]
    assert res["service_clean"] is True, res["ranks"]
    warns = [line for line in out.splitlines() if "[ocm W" in line or "[ocm E" in line]
    assert not warns, warns[:20]
    # every size was measured op by op (p50 headline, p99 beside it)
    row = res["sweep"][str(1 << 20)]
    assert row["ops"] >= 5 and row["get_p99_us"] >= row["get_us"] > 0, row


def test_two_embedded_ranks_allocate_1gib_pairs_at_once():
    # The round-5 hang (profiles/embedded_hang_r05o/, native stacks in embedded_hang_r06a/): two ranks
    # with embedded daemons allocating their 2 GiB + 1 pairs (the driver's config) at the same moment,
    # each importing the other's fresh dedicated HBM slab. The runtime's IPC import asked the exporting
    # process for the slab's DMA-BUF and spun forever when that process's fd server closed without
    # one; HBM slabs now travel as DMA-BUFs over the daemon's own mailbox (OCM_GPU_IPC=fd).
    env = dict(os.environ, OCM_BENCH_SHARE_GPU="1", OCM_BENCH_TIMEOUT_S="90", OCM_BENCH_DAEMONS="embedded",
               OCM_HANG_DUMP_S="30")
    log = os.path.join(REPO, "gpurun_out", "test_gpu_share_embedded_1g.log")
    os.makedirs(os.path.dirname(log), exist_ok=True)
    with open(log, "w") as lf:
        p = subprocess.Popen([sys.executable, "-u", "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
                              "2", "--master-addr", "127.0.0.1", "--master-port", "29683",
                              os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                              "--alloc-samples", "20", "--no-characterize", "--no-ctrl-extra", "--no-hw-baseline",
                              "--no-optim-extra", "--no-autotune"],
                             stdout=lf, stderr=subprocess.STDOUT, text=True, cwd="/tmp", env=env,
                             start_new_session=True)
        try:
            rc = p.wait(timeout=150)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, 9)
            p.wait(timeout=30)
            raise AssertionError("the 1 GiB-pair rehearsal did not finish in 150 s: " + open(log).read()[-3000:])
    out = open(log).read()
    assert rc == 0, out[-4000:]
    res = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
    print(json.dumps({k: res.get(k) for k in ("value", "service_clean", "alloc_p50_us")}))
    assert res["config"]["daemons"] == "embedded" and res["config"]["remote_tier"] == "hbm", res["config"]
    assert res["config"]["model"].startswith("ocm_test-4 R/W sweep, 2x1GiB+1"), res["config"]
    assert res["value"] > 0 and res["service_clean"] is True and "fallback" not in res, res
    assert "ocm stack dump" not in out
