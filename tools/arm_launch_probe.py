"""What an idle pre-armed copy-service instance costs OTHER work's launch latency
(round 6). While the copy service is idle, libocm keeps its next
instance queued behind a closed barrier-AND gate on its own AQL queue
(OCM_SERVICE_PREARM, service.cpp's armer). The packet processor holds that packet at
the queue's head until the gate opens. Does the blocked queue slow the dispatch of
kernels on other queues, say a small torch kernel or the control plane's tick kernels?

Each child is a fresh process. It launches a one-element torch kernel and
synchronises, 3000 times, and reports p10 / p50 / p90 of that round trip; then the time
per kernel of 5000 such kernels queued back to back (host-bound), of 1000 in a replayed graph
(packet-processor-bound), and a bf16 8192^3 GEMM. Modes:
  nolib    torch only, libocm not loaded
  default  libocm attached, its defaults (since this probe: arming off)
  unarmed  libocm attached, OCM_SERVICE_PREARM=0 (no instance queued)
  armed    libocm attached, OCM_SERVICE_PREARM=1 with no window (OCM_SERVICE_PREARM_MS=0): an
           instance queued behind its gate for the whole measurement
  armed_normal / armed_low   the same with the service's AQL queue at normal / low priority
                             (OCM_AQL_PRIORITY; the library's default is high)
  armed_window  OCM_SERVICE_PREARM=1 with the default 20 ms window: cancelled before the
           measurement starts (50 ms idle)
  nolone   libocm defaults but OCM_SERVICE_LONE_US=0 (no lead stays resident after an op)
  noinline libocm defaults but OCM_SERVICE_INLINE=0 (a cold start's solo request is polled for, not
           carried in the kernel arguments); inline_armed / noinline_armed: the same with arming on
Each libocm mode also times a 200-kernel graph replayed right after a 4 KiB op (the lone lead
resident by default).
Each libocm mode also reports a 4 KiB get after 10 ms idle and back to back (what arming buys).
Modes are interleaved over rounds, since queue placement can change from process to process.

    python tools/arm_launch_probe.py [--rounds 6] [--modes nolib,unarmed,armed] [--out f.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def pcts(xs):
    xs = sorted(xs)
    n = len(xs)
    return {f"p{p}_us": round(xs[min(n - 1, int(n * p / 100))] * 1e6, 2) for p in (10, 50, 90)}


def launch_rtt(n=3000):
    import torch

    x = torch.zeros(1, device="cuda")
    for _ in range(200):
        x.add_(1)
        torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        x.add_(1)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    r = pcts(out)
    # throughput: 5000 one-element kernels queued back to back, one sync
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5000):
            x.add_(1)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 5000)
    r["queued_us_per_kernel"] = round(sorted(ts)[2] * 1e6, 3)  # host-bound (Python launch cost)
    # packet-processor-bound: 1000 one-element kernels in one captured graph, replayed
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x.add_(1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        for _ in range(1000):
            x.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        graph.replay()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 1000)
    r["graph_us_per_kernel"] = round(sorted(ts)[3] * 1e6, 3)
    # a compute-bound kernel: bf16 GEMM 8192^3, ms
    a = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    for _ in range(3):
        a @ b
    torch.cuda.synchronize()
    g = []
    for _ in range(10):
        t0 = time.perf_counter()
        a @ b
        torch.cuda.synchronize()
        g.append(time.perf_counter() - t0)
    r["gemm8192_ms"] = round(sorted(g)[5] * 1e3, 3)
    return r


def graph_after_op(a, k=200, reps=9):
    """Per-kernel time of a k-kernel graph replayed right after a 4 KiB op, i.e. while the
    copy service's lone lead is still resident (OCM_SERVICE_LONE_US, 2 ms by default)."""
    import torch

    x = torch.zeros(1, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x.add_(1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(k):
            x.add_(1)
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        time.sleep(5e-3)  # the lead has left (and any window ended)
        a.get(0, 0, 4096)
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / k)
    return round(sorted(ts)[reps // 2] * 1e6, 3)


def throwaway_sessions(k: int) -> None:
    """k short library sessions first (mesh, client, a put/get on an HBM and a host-tier pair,
    free, stop), as a long test process runs them: does what they leave behind change the tax?"""
    from oncilla_amd import api
    from oncilla_amd.parallel.mesh import Mesh

    for i in range(k):
        with Mesh(1, gpus=[0], embedded=(i % 2 == 1)) as m:
            with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
                for flags in (api.OCM_ALLOC_LOOPBACK, api.OCM_ALLOC_HOST_TIER):
                    a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=1 << 20, remote_bytes=1 << 20, flags=flags)
                    a.put(0, 0, 1 << 20)
                    a.get(0, 0, 1 << 20)
                    a.free()


def child(mode: str) -> dict:
    import torch

    torch.zeros(1, device="cuda")
    row = {"mode": mode}
    k = int(os.environ.get("ARM_PROBE_SESSIONS", "0"))
    if k and mode != "nolib":
        throwaway_sessions(k)
        row["sessions_before"] = k
        row["threads_before"] = len(os.listdir("/proc/self/task"))
    if mode == "nolib":
        row.update(launch_rtt())
        return row
    from oncilla_amd import api
    from oncilla_amd.parallel.mesh import Mesh

    from oncilla_amd.models import workloads as wl

    with Mesh(1, gpus=[0], embedded=True) as m:
        with api.Client(daemon_rank=0, gpu=0, ns=m.ns) as c:
            a = c.alloc(api.OCM_REMOTE_GPU, local_bytes=4096, remote_bytes=4096, flags=api.OCM_ALLOC_HOST_TIER)
            a.time_onesided_samples(0, 4096, 50)
            time.sleep(0.05)  # past the armer's idle period (~2.6 ms)
            h = api.service_health()
            row["prearmed"] = h.get("prearmed")
            row["prearm_cancels"] = h.get("prearm_cancels")
            row["inline_starts_at_attach"] = h.get("inline_starts")
            row.update(launch_rtt())
            row["prearmed_after"] = api.service_health().get("prearmed")
            # what arming buys: a 4 KiB get after 10 ms idle (this mode's setting), p50
            xs, rel = a.time_onesided_samples(0, 4096, 31, gap_s=10e-3)
            row["get_after_10ms_p50_us"] = round(wl.percentile(xs[1:], 50) * 1e6, 2)
            hc = api.service_health()
            row["cold_start_to_seen_us_p50"] = hc.get("cold_start_to_seen_us_p50")
            row["inline_starts"] = hc.get("inline_starts")
            row["get_hot_p50_us"] = round(wl.percentile(a.time_onesided_samples(0, 4096, 300)[0], 50) * 1e6, 2)
            row["graph_after_op_us_per_kernel"] = graph_after_op(a)
            a.free()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default="")
    ap.add_argument("--modes", default="nolib,default,armed,armed_window")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child)), flush=True)
        return
    res = []
    for r in range(a.rounds):
        for mode in a.modes.split(","):
            env = dict(os.environ)
            if mode.startswith("unarmed"):
                env["OCM_SERVICE_PREARM"] = "0"
            elif mode.startswith("armed"):
                env["OCM_SERVICE_PREARM"] = "1"
                env["OCM_SERVICE_PREARM_MS"] = "20" if mode == "armed_window" else "0"
            if mode == "nolone":
                env["OCM_SERVICE_LONE_US"] = "0"
            if mode.startswith("noinline"):  # noinline / noinline_armed: OCM_SERVICE_INLINE=0
                env["OCM_SERVICE_INLINE"] = "0"
            if mode in ("inline_armed", "noinline_armed"):
                env["OCM_SERVICE_PREARM"] = "1"
            for pr in ("normal", "low"):  # armed_normal / armed_low: the service queue's priority
                if mode.endswith("_" + pr):
                    env["OCM_AQL_PRIORITY"] = pr
            p = subprocess.run([sys.executable, "-u", __file__, "--child", mode], capture_output=True, text=True,
                               timeout=180, env=env)
            line = [x for x in p.stdout.splitlines() if x.startswith("{")]
            row = json.loads(line[-1]) if line else {"error": p.stderr[-1500:], "mode": mode}
            row["round"] = r
            res.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
