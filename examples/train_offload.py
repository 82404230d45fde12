"""Training with the optimizer state in disaggregated memory.

A small MLP regression trained with models.OffloadedAdam: the Adam moments (and,
with --bf16, the fp32 master weights) live in the HBM of other daemons' GPUs,
striped over them (on a one-GPU box the daemons share GPU 0), and one fused
gfx950 kernel per parameter updates them in place. Without a GPU the staged path
runs on the CPU with the state in the daemons' host tier.

With --accum N every step sums N micro-batches' gradients in disaggregated memory too
(models.OffloadedGradAccumulator: fp32 accumulators in the remote half, one one-sided
accumulate per micro-batch) and hands the optimizer their mean. With --accum-in-place (GPU)
the fused Adam kernel reads that mean from the accumulators itself and zeroes them in the same
pass: no read-back region, no copy into .grad and no zeroing pass after the first. With
--clip-norm X on top of that, every step first reduces the accumulators where they are to their
global 2-norm (one read-only pass, one host synchronise) and clips the gradient to X through the
kernel's scale; a step whose accumulators hold an inf or NaN is skipped.

    python examples/train_offload.py [--gpu 0] [--bf16] [--steps 200] [--accum 4 [--accum-in-place [--clip-norm 1.0]]]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oncilla_amd import api  # noqa: E402
from oncilla_amd.models import OffloadedAdam, OffloadedGradAccumulator  # noqa: E402
from oncilla_amd.parallel import Mesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", type=int, default=None)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--daemons", type=int, default=3)
    ap.add_argument("--accum", type=int, default=0, help="micro-batches per step, summed in disaggregated memory")
    ap.add_argument("--accum-in-place", action="store_true",
                    help="with --accum: the optimizer reads (and zeroes) the remote accumulators itself")
    ap.add_argument("--clip-norm", type=float, default=None,
                    help="with --accum-in-place: clip the gradient to this global 2-norm, computed over the accumulators")
    args = ap.parse_args()
    if args.accum_in_place and args.accum <= 0:
        ap.error("--accum-in-place goes with --accum N")
    if args.clip_norm is not None and not args.accum_in_place:
        ap.error("--clip-norm goes with --accum-in-place (torch's clip_grad_norm_ serves local gradients)")
    on_gpu = args.gpu is not None
    dev = f"cuda:{args.gpu}" if on_gpu else "cpu"
    dtype = torch.bfloat16 if args.bf16 else torch.float32
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.GELU(), torch.nn.Linear(256, 1)).to(dev, dtype)
    teacher = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Tanh(), torch.nn.Linear(32, 1)).to(dev)
    gpus = [args.gpu] * args.daemons if on_gpu else None
    with Mesh(args.daemons, gpus=gpus, policy="stripe") as mesh:
        with api.Client(daemon_rank=0, gpu=args.gpu, ns=mesh.ns) as c:
            opt = OffloadedAdam(model.parameters(), c, lr=3e-3)
            tiers = sorted({e["tier"] for e in opt.allocs[0].remote_info()["extents"]})
            first = last = norm = None
            clipped = 0
            params = list(model.parameters())
            acc = OffloadedGradAccumulator(params, c, readback=not args.accum_in_place) if args.accum > 0 else None

            def micro_batch():
                x = torch.randn(256, 64, device=dev)
                with torch.no_grad():
                    y = teacher(x)
                return torch.nn.functional.mse_loss(model(x.to(dtype)).float(), y)

            for step in range(args.steps):
                if acc:
                    if not args.accum_in_place:
                        acc.zero()
                    total = 0.0
                    for _ in range(args.accum):
                        loss = micro_batch()
                        acc.zero_grads()
                        loss.backward()
                        acc.add(scale=1.0 / args.accum)  # remote fp32 += grad / N, one launch
                        total += loss.item()
                    if args.clip_norm is not None:
                        norm = opt.step(accumulator=acc, max_norm=args.clip_norm, skip_nonfinite=True)
                        clipped += norm > args.clip_norm
                    elif args.accum_in_place:
                        opt.step(accumulator=acc)  # g = the fp32 accumulators, zeroed by the same kernel
                    else:
                        sums = acc.read()
                        with torch.no_grad():
                            for p, g in zip(params, sums):
                                p.grad.copy_(g)  # the mean gradient, rounded once into the parameter's dtype
                        opt.step()
                    step_loss = total / args.accum  # the step's loss: the mean over its micro-batches
                else:
                    loss = micro_batch()
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
                    step_loss = loss.item()
                if step == 0:
                    first = step_loss
                last = step_loss
            if acc:
                acc.close()
            opt.close()
    where = "+".join({1: "host tier", 2: "peer HBM"}[t] for t in tiers)
    print(f"{args.steps} steps, mode={opt.mode}, {dtype}, optimizer state in {where}: "
          f"loss {first:.4f} -> {last:.4f}")
    if args.clip_norm is not None:
        print(f"clip-norm {args.clip_norm:g}: last gradient norm {norm:.4f}, {clipped} of {args.steps} steps clipped")
    if not last < 0.5 * first:
        raise SystemExit("loss did not go down")


if __name__ == "__main__":
    main()
