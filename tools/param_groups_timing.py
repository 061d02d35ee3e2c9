"""Device time of the grouped parameter update (param_groups= / tensor_groups=): G launches of the existing update entry point
over G sub-plans against the one launch without groups.

    python tools/param_groups_timing.py [--chunks 9] [--calls 20] [--steps]

Legs: tensor_groups=None and G = 1, 2, 4, 8 groups of equal total size (tensors dealt round-robin, so the groups are interleaved),
fp32 parameters, clipping and weight decay on, alternating chunk by chunk; median [min .. max] of the chunks, events around
`calls` calls.  Sizes: the flat tail (uvd_step_tail) at N = 4 M and N = 100 M over 256 tensors, and the list tail
(multi_param_update) on 8 x (1024 x 4096) + 8 x (1024 x 1024) repeated to 256 tensors of 41.9 M elements.  --steps: whole steps
of class UVd (N = 4 M over 256 tensors, r = 10, fused tail, exact products) with param_groups=None against G = 4, 9 chunks of 50.

For the kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/param_groups_timing.py --chunks 3 --calls
10` in a run of its own, without counters.  To compare with another commit, run the same command on a checkout of it in the same
job: the None leg is the code path of before.  The results go to profiles/param_groups.txt."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

DEV = torch.device("cuda:0")
GS = (None, 1, 2, 4, 8)


def _groups(k, G):
    return None if G is None else [(tuple(range(j, k, G)), 1.0 - 0.05 * j, 0.01 * (j % 2)) for j in range(G)]


def _timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def _report(title, legs, chunks, calls):
    print(title)
    for fn in legs.values():
        fn()                                                    # tables and sub-plans are made here, not in a timed chunk
    times = {name: [] for name in legs}
    for _ in range(chunks):
        for name, fn in legs.items():
            times[name].append(_timed(fn, calls))
    base = statistics.median(times[next(iter(legs))])
    for name, ts in times.items():
        print("  %-44s %9.1f us  [%8.1f .. %8.1f]   x%.3f" % (name, statistics.median(ts), min(ts), max(ts), statistics.median(ts) / base))


def flat(n, k, chunks, calls):
    sizes = [n // k] * (k - 1) + [n - (n // k) * (k - 1)]
    params = [torch.randn(s, device=DEV) for s in sizes]
    pre = torch.randn(n, device=DEV)
    plan = psgd.UVdTailPlan(sizes, torch.float32, DEV)
    legs = {}
    for G in GS:
        kw = dict(weight_decay=0.01) if G is None else dict(tensor_groups=_groups(k, G))
        legs["uvd_step_tail, %s" % ("no groups" if G is None else "G = %d" % G)] = \
            lambda kw=kw: psgd.uvd_step_tail(params, pre, 1e-3, 1.0, plan=plan, **kw)
    _report("flat, N = %.1f M over %d tensors, clip + weight decay (sum of squares included)" % (n / 1e6, k), legs, chunks, calls)


def lists(chunks, calls):
    shapes = ([(1024, 4096)] * 8 + [(1024, 1024)] * 8)
    sizes = [m * n // 16 for m, n in shapes for _ in range(16)]                   # 256 tensors, 41.9 M elements
    params = [torch.randn(s, device=DEV) for s in sizes]
    grads = [torch.randn(s, device=DEV) for s in sizes]
    sumsq = psgd.multi_sumsq(grads).clone()
    legs = {}
    for G in GS:
        kw = dict(weight_decay=0.01) if G is None else dict(tensor_groups=_groups(len(sizes), G))
        legs["multi_param_update, %s" % ("no groups" if G is None else "G = %d" % G)] = \
            lambda kw=kw: psgd.multi_param_update(params, grads, None, 1e-3, sumsq, 1.0, **kw)
    _report("lists, %.1f M elements in %d tensors, clip + weight decay" % (sum(sizes) / 1e6, len(sizes)), legs, chunks, calls)


def steps(chunks, n=4 << 20, k=256, per_chunk=50):
    legs = {}
    for G in (None, 4):
        params = [torch.randn(n // k, device=DEV, requires_grad=True) for _ in range(k)]
        a = torch.rand(n, device=DEV) + 0.5
        groups = None if G is None else [{"params": params[j::G][:], "lr_scale": 1.0 - 0.05 * j, "weight_decay": 0.01 * (j % 2)}
                                         for j in range(G)]
        opt = psgd.UVd(params, 10, lr_params=1e-3, grad_clip_max_norm=1.0, step_tail="fused", weight_decay=0.01, placement=None,
                       generator=torch.Generator().manual_seed(0), param_groups=groups)
        closure = lambda params=params, a=a: 0.5 * torch.sum(a * torch.cat([p.reshape(-1) for p in params]) ** 2)
        legs["class UVd whole step, %s" % ("param_groups=None" if G is None else "G = %d" % G)] = lambda opt=opt, c=closure: opt.step(c)
    _report("whole step, N = %.1f M over %d tensors, r = 10, fused tail" % (n / 1e6, k), legs, chunks, per_chunk)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", action="store_true")
    args = ap.parse_args()
    flat(4 << 20, 256, args.chunks, args.calls)
    flat(100 * 10 ** 6, 256, args.chunks, args.calls)
    lists(args.chunks, args.calls)
    if args.steps:
        steps(args.chunks)
