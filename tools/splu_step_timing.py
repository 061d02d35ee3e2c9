#!/usr/bin/env python
"""Time one sparse-LU training step three ways on a closure that costs next to nothing:

    functional   the loop a user writes by hand from update_precond_splu / precond_grad_splu and torch ops
                 (demo_usage_of_all_preconditioners.py:46-62): the baseline, code from before class SPLU
    torch        class SPLU, step_tail="torch"
    fused        class SPLU, step_tail="fused"

The closure is 0.5 ||w||^2 over all parameter tensors (tools/uvd_step_tail_timing.py), exact Hessian-vector products, no clipping,
fp32, r = 10, 256 tensors.  Protocol: the three legs are built side by side and ALTERNATE chunk by chunk in one job; --chunks (9)
chunks of --steps (50) steps per leg, each timed by the host clock between two device synchronisations; the figure is the median
over the chunks with [min .. max].  A difference between two legs counts as resolved when it exceeds the larger of their spreads
(max - min).  Peak memory: torch.cuda.max_memory_allocated over one further step minus what was allocated at its entry.

    python tools/splu_step_timing.py                          # N = 4M and N = 50M, written to profiles/splu_class.txt
    python tools/splu_step_timing.py --sizes 4000000          # one size
    python tools/splu_step_timing.py --trace 4000000          # 5 fused steps and nothing else, for
                                                              # rocprofv3 --kernel-trace --stats -- python tools/splu_step_timing.py --trace 4000000
    python tools/splu_step_timing.py --sizes 4000000 --parent-module FILE --out FILE
        # whether the host layer of a step moved: FILE is the psgd_tf_amd/__init__.py of another commit's built tree, loaded as a
        # second package; its class SPLU runs on each tail TWICE ("parent-torch", "parent-torch-2", ...) in the place of the
        # functional leg.  The bar is the parent in the same job, the margin the difference between the medians of its two legs.
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

R, K, LR, LR_Q = 10, 256, 1e-3, 0.1


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
    box = {"state": psgd.splu_initial_factors(N, R, 0.1, device=params[0].device)}

    def step():
        with torch.enable_grad():
            grads = torch.autograd.grad(closure(), params, create_graph=True)
            vs = [torch.randn_like(p) for p in params]
            hvs = torch.autograd.grad(grads, params, vs)
        with torch.no_grad():
            box["state"] = psgd.update_precond_splu(*box["state"], vs, hvs, LR_Q)
            pre = psgd.precond_grad_splu(*box["state"], [g.detach() for g in grads])
            for p, g in zip(params, pre):
                p.sub_(LR * g)
    return step


def parent_class(path):
    """class SPLU of the package whose __init__.py is at `path`, loaded whole as a second package beside this tree's"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("psgd_tf_amd_parent", path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.psgd.SPLU


def class_leg(N, tail, cls=None):
    params = _params(N)
    opt = (cls or psgd.SPLU)(params, R, lr_params=LR, lr_preconditioner=LR_Q, step_tail=tail)
    closure = _closure(params)
    return lambda: opt.step(closure)


def peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def table(N, steps, chunks, out, parent=None):
    legs = {"functional": functional_leg(N), "torch": class_leg(N, "torch"), "fused": class_leg(N, "fused")}
    pairs = [("torch", "functional"), ("fused", "functional")]
    if parent is not None:
        del legs["functional"]
        pairs = []
        for tail in ("torch", "fused"):
            legs.update({"parent-" + tail: class_leg(N, tail, parent), "parent-%s-2" % tail: class_leg(N, tail, parent)})
            pairs += [(tail, "parent-" + tail), ("parent-%s-2" % tail, "parent-" + tail)]
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
        out("N=%d r=%d k=%d float32 | %-14s: %9.1f [%9.1f .. %9.1f] us per step, peak over a step +%d B"
            % (N, R, K, k, med[k] * 1e6, min(times[k]) * 1e6, max(times[k]) * 1e6, peak_delta(legs[k])))
    for k, base in pairs:
        d, s = med[k] - med[base], max(spread[k], spread[base])
        out("N=%d | %s - %s: %+.1f us (%+.1f %%), spread %.1f us: %s"
            % (N, k, base, d * 1e6, 100.0 * d / med[base], s * 1e6, "resolved" if abs(d) > s else "NOT resolved"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000000,50000000")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(_root, "profiles", "splu_class.txt"))
    ap.add_argument("--trace", type=int, default=None, metavar="N")
    ap.add_argument("--parent-module", default=None, metavar="FILE")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    if a.trace is not None:
        step = class_leg(a.trace, "fused")
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        print("trace: 5 fused steps, N=%d r=%d k=%d fp32" % (a.trace, R, K))
        return
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    out("# one sparse-LU step, exact Hessian-vector products, no clipping | leg: median [min .. max] over %d chunks of %d steps, legs "
        "alternating" % (a.chunks, a.steps))
    parent = parent_class(a.parent_module) if a.parent_module else None
    for N in (int(x) for x in a.sizes.split(",")):
        table(N, a.steps, a.chunks, out, parent)
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
