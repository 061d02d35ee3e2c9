#!/usr/bin/env python
"""Timing and memory of the bf16-state UVd step on the row-sharded route, on a 1-rank RCCL group (one GPU).

    python tools/uvd_bf16_sharded_timing.py --rows 4194304 --out profiles/uvd_bf16_sharded.txt

Per problem size (r = 20) it appends to --out:
  * the fused step (update -> apply, stochastic rounding) as the unsharded one-call function and through psgd_tf_amd/sharded.py
    on ONE set of tensors: medians of interleaved rounds, and their difference -- the exchange-overhead leg (4 all-gathers on the
    caller's stream + 4 fold kernels + the split fold kernels per step; no xGMI hop: one GPU);
  * bytes allocated over the state during one step of class UVd(group=pg) with a bf16 state: state_route="native" against the
    `widen` route (fp32 copies of this rank's rows every step).
More than one rank is not measured here."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP, R = 0.01, 20


def fused_times(psgd, sharded, dev, rows, steps, rounds=5):
    tiny = torch.finfo(torch.float32).tiny
    g = torch.Generator(device=dev).manual_seed(0)
    sc = (1.0 / (rows * R)) ** 0.5
    U = (torch.randn(rows, R, device=dev, generator=g) * sc).bfloat16()
    V = (torch.randn(rows, R, device=dev, generator=g) * sc).bfloat16()
    d = torch.ones(rows, 1, device=dev).bfloat16()
    v, h, grad = (torch.randn(rows, 1, device=dev, generator=g) for _ in range(3))
    paths = {"unsharded": psgd, "sharded_1rank": sharded}

    def timed(mod, count, seed0):
        for i in range(3):
            mod.update_precond_UVd_math_and_precond_grad(U, V, d, v, h, grad, STEP, tiny, balance=False, update_U=(i % 2 == 0),
                                                         rounding="stochastic", rounding_seed=seed0 + i)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(count):
            out = mod.update_precond_UVd_math_and_precond_grad(U, V, d, v, h, grad, STEP, tiny, balance=False, update_U=(i % 2 == 0),
                                                               rounding="stochastic", rounding_seed=seed0 + 10 + i)
        torch.cuda.synchronize(dev)
        assert torch.isfinite(out).all().item()
        return (time.perf_counter() - t0) / count * 1e3
    runs = {k: [] for k in paths}
    for rnd in range(rounds):                          # interleaved rounds: both paths see the same clocks
        for name in paths:
            runs[name].append(timed(paths[name], steps, 1000 * rnd))
    return {k: statistics.median(x) for k, x in runs.items()}, runs


def step_memory(psgd, dev, rows, group):
    peaks = {}
    for route in ("native", "widen"):
        torch.manual_seed(1)
        w = (torch.randn(rows, device=dev) * 0.1).to(torch.bfloat16).requires_grad_(True)
        c = torch.rand(rows, device=dev) + 0.5
        opt = psgd.UVd([w], rank_of_modification=R, lr_params=0.01, lr_preconditioner=0.01, generator=torch.Generator().manual_seed(1),
                       state_dtype="param", state_route=route, placement=None, group=group)
        closure = lambda: 0.5 * (c * w.float() * w.float()).sum()      # noqa: E731
        opt.step(closure)                                               # warm-up: workspaces exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        opt.step(closure)
        torch.cuda.synchronize()
        peaks[route] = torch.cuda.max_memory_allocated() - before
        del opt, w, c, closure
        torch.cuda.empty_cache()
    return peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-memory", action="store_true", help="skip the class UVd memory leg")
    args = ap.parse_args()
    import torch.distributed as dist
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29543")
    dist.init_process_group(backend="nccl", device_id=dev, rank=0, world_size=1)
    try:
        import preconditioned_stochastic_gradient_descent as psgd
        from psgd_tf_amd import sharded
        med, runs = fused_times(psgd, sharded, dev, args.rows, args.steps)
        lines = ["N = %d, r = %d, 1-rank RCCL group (direct communicator: %s), %d steps x 5 interleaved rounds, stochastic rounding"
                 % (args.rows, R, sharded._direct_comm(None, dev) is not None, args.steps),
                 "  fused step, unsharded native call      %8.3f ms   (rounds: %s)" % (med["unsharded"], " ".join("%.3f" % x for x in runs["unsharded"])),
                 "  fused step, sharded native, 1 rank     %8.3f ms   (rounds: %s)" % (med["sharded_1rank"], " ".join("%.3f" % x for x in runs["sharded_1rank"])),
                 "  exchange overhead (4 exchanges)        %8.1f us per step (%.2f %% of the step)"
                 % ((med["sharded_1rank"] - med["unsharded"]) * 1e3, 100 * (med["sharded_1rank"] - med["unsharded"]) / med["unsharded"])]
        if not args.no_memory:
            peaks = step_memory(psgd, dev, args.rows, dist.group.WORLD)
            lines.append("  class UVd(group=pg) step, allocated over the state: native %.1f MB, widen %.1f MB (one fp32 factor: %.1f MB)"
                         % (peaks["native"] / 1e6, peaks["widen"] / 1e6, 4 * args.rows * R / 1e6))
        text = "\n".join(lines)
        print(text)
        if args.out:
            with open(args.out, "a") as f:
                f.write(text + "\n")
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
