#!/usr/bin/env python
"""Time one dense-preconditioner training step three ways on a closure that costs next to nothing:

    functional   the loop a user writes by hand from update_precond_dense / precond_grad_dense and torch ops
                 (demo_usage_of_all_preconditioners.py:30-41): the baseline, code from before class Dense
    torch        class Dense, step_tail="torch"
    fused        class Dense, step_tail="fused"

The closure is 0.5 ||w||^2 over all parameter tensors (tools/uvd_step_tail_timing.py), exact Hessian-vector products, no clipping,
fp32, 16 tensors.  Protocol (tools/splu_step_timing.py): the three legs are built side by side and ALTERNATE chunk by chunk in one
job; --chunks (9) chunks of --steps (50) steps per leg, each timed by the host clock between two device synchronisations; the
figure is the median over the chunks with [min .. max].  A difference between two legs counts as resolved when it exceeds the
larger of their spreads (max - min).  Peak memory: torch.cuda.max_memory_allocated over one further step minus what was allocated
at its entry; beside it, 4 N^2, the bytes of one Q.

    python tools/dense_step_timing.py                         # N = 1028 and N = 8192, written to profiles/dense_class.txt
    python tools/dense_step_timing.py --sizes 1028            # one size
"""
import argparse
import os
import statistics
import sys
import time

import torch

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _root)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from tools.uvd_step_tail_timing import split  # noqa: E402

K, LR, LR_Q = 16, 1e-3, 0.1


def _params(N, seed=0):
    torch.manual_seed(seed)
    return [(torch.randn(n, device="cuda:0") * 0.1).requires_grad_(True) for n in split(N, K)]


def _closure(params):
    def closure():
        sq = torch._foreach_mul(params, params)
        return 0.5 * torch.stack([s.sum() for s in sq]).float().sum()
    return closure


def functional_leg(N):
    params = _params(N)
    closure = _closure(params)
    box = {"Q": psgd.dense_initial_factor(N, 0.1, device=params[0].device)}

    def step():
        with torch.enable_grad():
            grads = torch.autograd.grad(closure(), params, create_graph=True)
            vs = [torch.randn_like(p) for p in params]
            hvs = torch.autograd.grad(grads, params, vs)
        with torch.no_grad():
            box["Q"] = psgd.update_precond_dense(box["Q"], vs, hvs, LR_Q)
            pre = psgd.precond_grad_dense(box["Q"], [g.detach() for g in grads])
            for p, g in zip(params, pre):
                p.sub_(LR * g)
    return step


def class_leg(N, tail):
    params = _params(N)
    opt = psgd.Dense(params, lr_params=LR, lr_preconditioner=LR_Q, step_tail=tail)
    closure = _closure(params)
    return lambda: opt.step(closure)


def peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def table(N, steps, chunks, out):
    legs = {"functional": functional_leg(N), "torch": class_leg(N, "torch"), "fused": class_leg(N, "fused")}
    for fn in legs.values():                                  # warm-up: every leg has run every launch and holds its buffers
        for _ in range(5):
            fn()
    times = {k: [] for k in legs}
    for _ in range(chunks):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    for k in legs:
        out("N=%d k=%d float32 | %-10s: %9.1f [%9.1f .. %9.1f] us per step, peak over a step +%d B (one Q: %d B)"
            % (N, K, k, med[k] * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, peak_delta(legs[k]), 4 * N * N))
    for k in ("torch", "fused"):
        d, s = med[k] - med["functional"], max(spread[k], spread["functional"])
        out("N=%d | %s - functional: %+.1f us (%+.1f %%), spread %.1f us: %s"
            % (N, k, d * 1e6, 100.0 * d / med["functional"], s * 1e6, "resolved" if abs(d) > s else "NOT resolved"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1028,8192")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(_root, "profiles", "dense_class.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("# one dense-preconditioner step, exact Hessian-vector products, no clipping | leg: median [min .. max] over %d chunks of %d "
        "steps, legs alternating" % (a.chunks, a.steps))
    for N in (int(x) for x in a.sizes.split(",")):
        table(N, a.steps, a.chunks, out)
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
