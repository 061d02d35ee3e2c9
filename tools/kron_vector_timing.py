"""Time one whole step of class Kron(any_rank=True) on a model with many vectors, two legs in one job:

    list     vector_route="list": all vectors in one multi_vec_precond_update and one multi_vec_precond_grad launch
    layer    vector_route="layer": every vector through update_precond_kron / precond_grad_kron on its [1, n] view

Workload: 200 vectors of length 1024 plus one 1024 x 4096 layer, exact Hessian-vector products, clipping on, fused step tail,
quadratic loss (the closure is the same in both legs, so it cancels in the difference).  Protocol of tools/kron_step_timing.py: every
leg warms up for at least 0.5 s, then the legs ALTERNATE chunk by chunk; a chunk is `--steps` steps between two synchronises on
the host clock; reported are the median and the range of the per-chunk step times over `--chunks` (>= 7) chunks.  A difference
smaller than the largest range of a leg is not resolved, and the summary line says so.

    python tools/kron_vector_timing.py [--chunks 9] [--steps 50] [--out profiles/kron_vectors.txt]

--kernels runs the list leg alone for `--steps` steps and nothing else: the run to put under a kernel-stats profiler for the two
kernels' own times (k_multi_vec_update, k_multi_vec_apply).
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

VECTORS, LENGTH, MATRIX = 200, 1024, (1024, 4096)
LR, LR_Q = 0.01, 0.01


def leg(route, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    m, n = MATRIX
    hl = torch.exp(torch.empty(m, 1, device=dev).uniform_(-1.0, 1.0, generator=g))
    hr = torch.exp(torch.empty(1, n, device=dev).uniform_(-1.0, 1.0, generator=g))
    hv = torch.exp(torch.empty(VECTORS, LENGTH, device=dev).uniform_(-1.0, 1.0, generator=g))
    W = torch.randn(m, n, device=dev, generator=g).requires_grad_(True)
    vecs = [torch.randn(LENGTH, device=dev, generator=g).requires_grad_(True) for _ in range(VECTORS)]
    params = [W] + vecs
    clip = 0.1 * sum(p.numel() for p in params) ** 0.5

    def closure():
        return 0.5 * torch.sum(W * W * hl * hr) + 0.5 * torch.sum(torch.stack(vecs) ** 2 * hv)
    opt = psgd.Kron(params, "dense", lr_params=LR, lr_preconditioner=LR_Q, grad_clip_max_norm=clip, step_tail="fused", any_rank=True,
                    vector_route=route)
    return lambda: opt.step(closure)


def timed(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.chunks < 7:
        ap.error("--chunks must be at least 7")
    dev = torch.device("cuda:0")
    if a.kernels:
        step = leg("list", dev)
        print("list leg, %d steps: %.1f us per step" % (a.steps, timed(step, a.steps)))
        return
    lines = ["# tools/kron_vector_timing.py --chunks %d --steps %d on %s" % (a.chunks, a.steps, torch.cuda.get_device_name(0)),
             "# %d vectors of length %d plus one %d x %d layer, class Kron(any_rank=True, step_tail='fused'), whole step"
             % ((VECTORS, LENGTH) + MATRIX),
             "# us per step (closure + preconditioner + tail), median [min .. max] over the chunks; legs alternate chunk by chunk"]
    legs = {"list": leg("list", dev), "layer": leg("layer", dev)}
    for step in legs.values():                                      # warm-up: at least 0.5 s each, measured with the device drained
        spent = 0.0
        while spent < 0.5:
            spent += timed(step, 10) * 10e-6
    times = {k: [] for k in legs}
    for _ in range(a.chunks):
        for k, step in legs.items():
            times[k].append(timed(step, a.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append("vector_route=%-6s %10.1f  [%10.1f .. %10.1f]" % (k, med[k], min(v), max(v)))
    spread = max(max(v) - min(v) for v in times.values())
    d = med["layer"] - med["list"]
    lines.append("layer - list = %+.1f us per step: %s (largest range of a leg: %.1f us)"
                 % (d, "resolved" if abs(d) > spread else "NOT resolved by this protocol", spread))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
