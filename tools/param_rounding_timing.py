"""Time of the stochastic step-tail kernels against their round-to-nearest siblings, and of a whole Kron step with
param_rounding="stochastic" against "nearest" (profiles/param_rounding.txt).

    python tools/param_rounding_timing.py --kernels     # device time per launch (events around batches of launches), legs alternating:
                                                        #   lists: 8 x (1024 x 4096) + 8 x (1024 x 1024) = 41.9 M bf16 parameters,
                                                        #          fp32 gradients (psgd_multi_param_update_t / _sr) and bf16 gradients
                                                        #          (psgd_multi_param_update_mixed / _mixed_sr), with vs and weight decay
                                                        #   flat:  N = 100 M over 256 tensors (psgd_uvd_param_update_multi_wd / _sr)
                                                        # run it under `rocprofv3 --kernel-trace --stats --` for the per-kernel table
    python tools/param_rounding_timing.py --steps       # whole finite-difference steps of class Kron on bf16 parameters, fused tail,
                                                        # LeNet5 set and one 1024 x 4096 layer: medians over chunks, legs alternating
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
LIST_SHAPES = [(1024, 4096)] * 8 + [(1024, 1024)] * 8
SETS = {"lenet5": [(26, 6), (151, 16), (257, 120), (121, 84), (85, 10)], "1024x4096": [(1024, 4096)]}


def device_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def alternate(legs, chunks, n):
    """{name: (median, min, max)} of `chunks` chunks of n calls per leg, the legs taking turns"""
    for fn in legs.values():
        device_us(fn, 3)
    seen = {k: [] for k in legs}
    for _ in range(chunks):
        for k, fn in legs.items():
            seen[k].append(device_us(fn, n))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in seen.items()}


def show(title, res, base):
    print(title)
    for k, (med, lo, hi) in res.items():
        print("  %-44s %8.1f us  [%7.1f .. %7.1f]   x%.3f" % (k, med, lo, hi, med / res[base][0]))


def flat_sizes(N, k):
    base = N // k
    sizes = [base + (1 if i % 2 else -1) * (i % 7) for i in range(k)]
    sizes[-1] += N - sum(sizes)
    return sizes


def kernels(a):
    gen = torch.Generator(device=DEV).manual_seed(1)
    mk = lambda shape, dt, s=1.0: (torch.randn(shape, device=DEV, generator=gen) * s).to(dt)
    p = [mk(s, BF) for s in LIST_SHAPES]
    v = [mk(s, BF, 2.0 ** -8) for s in LIST_SHAPES]
    g32 = [mk(s, torch.float32, 1e-3) for s in LIST_SHAPES]
    g16 = [g.to(BF) for g in g32]
    n = sum(t.numel() for t in p)
    kw = dict(weight_decay=0.01)
    sr = dict(rounding="stochastic", rounding_seed=7)
    legs = {"psgd_multi_param_update_t (bf16)": lambda: psgd.multi_param_update(p, g32, v, 1e-3, **kw),
            "psgd_multi_param_update_sr": lambda: psgd.multi_param_update(p, g32, v, 1e-3, **kw, **sr)}
    show("lists, %.1f M elements, fp32 gradients, vs, weight decay (%d bytes per element)" % (n / 1e6, 2 + 2 + 2 + 4),
         alternate(legs, a.chunks, a.calls), "psgd_multi_param_update_t (bf16)")
    legs = {"psgd_multi_param_update_mixed (bf16)": lambda: psgd.multi_param_update(p, g16, v, 1e-3, **kw),
            "psgd_multi_param_update_mixed_sr": lambda: psgd.multi_param_update(p, g16, v, 1e-3, **kw, **sr)}
    show("lists, %.1f M elements, bf16 gradients, vs, weight decay (%d bytes per element)" % (n / 1e6, 2 + 2 + 2 + 2),
         alternate(legs, a.chunks, a.calls), "psgd_multi_param_update_mixed (bf16)")
    del p, v, g32, g16
    sizes = flat_sizes(a.flat, 256)
    p = [mk((s,), BF) for s in sizes]
    v = [mk((s,), BF, 2.0 ** -8) for s in sizes]
    pre = mk((a.flat,), torch.float32, 1e-3)
    plan = psgd.UVdTailPlan(sizes, BF, DEV)
    legs = {"psgd_uvd_param_update_multi_wd (bf16)": lambda: psgd.uvd_step_tail(p, pre, 1e-3, vs=v, plan=plan, **kw),
            "psgd_uvd_param_update_multi_sr": lambda: psgd.uvd_step_tail(p, pre, 1e-3, vs=v, plan=plan, **kw, **sr)}
    show("flat, N = %.0f M over 256 tensors, vs, weight decay (%d bytes per element)" % (a.flat / 1e6, 2 + 2 + 2 + 4),
         alternate(legs, a.chunks, a.calls), "psgd_uvd_param_update_multi_wd (bf16)")


def steps(a):
    for name, shapes in SETS.items():
        legs = {}
        for rounding in ("nearest", "stochastic"):
            gen = torch.Generator(device=DEV).manual_seed(2)
            params = [(torch.randn(s, device=DEV, generator=gen) * 0.1).to(BF).requires_grad_(True) for s in shapes]
            opt = psgd.Kron(params, "dense", 1.0, 1e-3, 0.01, None, 1.0, False, step_tail="fused",
                            generator=torch.Generator(device=DEV).manual_seed(3), param_rounding=rounding)
            closure = (lambda ps: lambda: sum(0.5 * torch.sum(w.float() ** 2) for w in ps))(params)
            legs["Kron bf16 %s, fd step, %s" % (name, rounding)] = (lambda o, c: lambda: o.step(c))(opt, closure)
        show("whole step, %s" % name, alternate(legs, a.chunks, a.calls), "Kron bf16 %s, fd step, nearest" % name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--flat", type=int, default=100_000_000)
    a = ap.parse_args()
    if a.kernels:
        kernels(a)
    if a.steps:
        steps(a)


if __name__ == "__main__":
    main()
