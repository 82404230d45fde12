"""Which processes hold the GPU while bench.py runs under torchrun.

Launches `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`
exactly as the driver does (127.0.0.1 rendezvous), optionally with every rank on
GPU 0 (OCM_BENCH_SHARE_GPU=1, a one-GPU box), and samples /proc every 20 ms: a
process "holds the GPU" while it has /dev/kfd (or a /dev/dri/renderD* node) open.
Reports the largest set held at once, what each member is (torchrun's parent,
a bench rank, an ocmd daemon, other), whether the launcher itself ever held it,
and the bench's own JSON line.

    python tools/gpu_holders.py --nproc 4 [--share] [--bench-args "..."] [--out f.json]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_fds(pid: int) -> bool:
    d = f"/proc/{pid}/fd"
    try:
        for fd in os.listdir(d):
            try:
                t = os.readlink(f"{d}/{fd}")
            except OSError:
                continue
            if t == "/dev/kfd" or t.startswith("/dev/dri/renderD"):
                return True
    except OSError:
        pass
    return False


def cmdline(pid: int) -> str:
    try:
        with open(f"/proc/{pid}/cmdline", "rb") as f:
            return f.read().replace(b"\0", b" ").decode(errors="replace").strip()
    except OSError:
        return ""


def kind(pid: int, launcher: int, cl: str) -> str:
    if pid == launcher:
        return "torchrun_parent"
    if "ocmd" in cl:
        return "ocmd_daemon"
    if "bench.py" in cl:
        return "bench_rank"
    return "other"


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nproc", type=int, default=2)
    ap.add_argument("--share", action="store_true", help="every rank on GPU 0 (OCM_BENCH_SHARE_GPU=1)")
    ap.add_argument("--bench-args", default="--full --steps 2 --warmup 1")
    ap.add_argument("--timeout", type=float, default=900)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = a.nproc
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(REPO, "bench.py"),
           "--gpus", str(n), *a.bench_args.split()]
    env = dict(os.environ)
    if a.share:
        env["OCM_BENCH_SHARE_GPU"] = "1"
    uid = os.getuid()
    t0 = time.time()
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=REPO)
    seen = {}        # pid -> (kind, cmdline) for every holder ever seen
    best = []        # largest concurrent holder set
    samples = 0
    last_print = t0
    while proc.poll() is None and time.time() - t0 < a.timeout:
        now_set = []
        for e in os.listdir("/proc"):
            if not e.isdigit():
                continue
            pid = int(e)
            try:
                if os.stat(f"/proc/{pid}").st_uid != uid:
                    continue
            except OSError:
                continue
            if pid == os.getpid() or not gpu_fds(pid):
                continue
            cl = cmdline(pid)
            now_set.append(pid)
            if pid not in seen:
                seen[pid] = (kind(pid, proc.pid, cl), cl[:160])
        samples += 1
        if len(now_set) > len(best):
            best = now_set
        if time.time() - last_print > 30:  # progress for the silence watchdog
            print(f"[holders] {time.time() - t0:.0f}s: {len(now_set)} now, max {len(best)}", file=sys.stderr, flush=True)
            last_print = time.time()
        time.sleep(0.02)
    if proc.poll() is None:
        proc.kill()
    out, err = proc.communicate()
    line = [x for x in out.splitlines() if x.startswith("{")]
    bench = json.loads(line[-1]) if line else None
    kinds = {}
    for pid in best:
        k = seen.get(pid, ("?", ""))[0]
        kinds[k] = kinds.get(k, 0) + 1
    res = {"nproc": n, "share_gpu": a.share, "launcher_cmd": " ".join(cmd[1:5]) + " ...", "samples": samples,
           "max_concurrent_holders": len(best), "holders_at_max_by_kind": kinds,
           "torchrun_parent_ever_held_gpu": proc.pid in seen,
           "every_holder_seen": sorted({v[0] for v in seen.values()}),
           "holders_seen_total": len(seen), "rc": proc.returncode, "wall_s": round(time.time() - t0, 1),
           "library_warnings": [x for x in err.splitlines() if "[ocm W" in x or "[ocm E" in x][:20],
           "bench": bench if bench else {"stderr_tail": err[-2000:]}}
    print(json.dumps({k: v for k, v in res.items() if k != "bench"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.splitext(a.out)[0] + ".ranks.log", "w") as f:  # every rank's stderr (warnings)
            f.write(err)
    return 0 if proc.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
