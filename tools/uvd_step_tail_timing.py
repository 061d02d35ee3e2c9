#!/usr/bin/env python
"""Time class UVd's step with the torch tail and with the fused tail (step_tail="fused") on a closure that costs next to nothing.

The closure is 0.5 ||w||^2 over all parameter tensors, so a step is: the closure with its gradient and Hessian-vector product (a few
launches per tensor, the same on both routes -- timed alone as "closure"), the fused update -> apply call, and the tail this tool is
about: lists of tensors -> flat vectors, the clip norm, the parameter update.

Protocol: warm up until the device has been busy for --warm-seconds (and at least 5 steps), then --chunks chunks of --steps steps,
each chunk timed by the host clock between two device synchronisations; the figure is the median over chunks, with the spread.
Peak memory: torch.cuda.max_memory_allocated over three further steps minus what was allocated before them.

    python tools/uvd_step_tail_timing.py                      # the table: N = 1M (1, 16, 256 tensors) and N = 100M (256 tensors)
    python tools/uvd_step_tail_timing.py --quick              # N = 1M only
    python tools/uvd_step_tail_timing.py --tail torch         # one route only (also runs on a checkout that has no step_tail)
    python tools/uvd_step_tail_timing.py --trace N K TAIL     # 20 steps of one configuration and nothing else, for
                                                              # rocprofv3 --kernel-trace --stats -- python tools/... --trace 1000000 256 fused
    python tools/uvd_step_tail_timing.py --momentum           # the fused step at N = 4M and N = 100M, r = 20, 256 tensors: plain,
                                                              # momentum=0.9, and momentum=0.9 with weight_decay=0.01
    python tools/uvd_step_tail_timing.py --momentum --legs plain --root OTHER   # the plain leg of another checkout (one that has
                                                              # no momentum argument): the baseline of the comparison
    python tools/uvd_step_tail_timing.py --guard              # the same shapes: plain against nonfinite="skip" (the checked packs and
                                                              # the 16-byte host read), with a loss scale, and both with momentum=0.9
                                                              # (one more read of the gradients); the legs alternate, --rounds times
    python tools/uvd_step_tail_timing.py --guard --legs plain --root OTHER      # the plain leg of a checkout without the arguments
    python tools/uvd_step_tail_timing.py --whitening          # the same shapes: preconditioner_fit="whitening" against the exact and
                                                              # the finite-difference Hessian steps, legs alternating, --rounds times
    python tools/uvd_step_tail_timing.py --whitening --parent-module FILE       # ... and the default (exact) step of the parent
                                                              # commit's module (its preconditioned_stochastic_gradient_descent.py,
                                                              # loaded next to this one on the same library) as the leg "parent"
"""
import argparse
import os
import statistics
import sys
import time

import torch

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv[1:-1]:                                # the checkout to import from (default: the one this file is in)
    _root = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, _root)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def split(N, k):
    """k sizes that sum to N, none a multiple of 4 where that can be avoided (starts land on odd elements, as in a real model)"""
    base = N // k
    sizes = [base + (1 if i % 2 else -1) * (i % 7) for i in range(k)] if base > 16 else [base] * k
    sizes[-1] += N - sum(sizes)
    assert sum(sizes) == N and min(sizes) >= 0
    return sizes


def build(N, r, k, dtype, clip, tail, seed=0, **extra):
    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    psgd.manual_seed(seed)
    params = [(torch.randn(n, device=dev) * 0.1).to(dtype).requires_grad_(True) for n in split(N, k)]
    kw = dict(extra) if tail == "torch" else dict(extra, step_tail=tail)
    opt = psgd.UVd(params, rank_of_modification=r, lr_params=1e-3, lr_preconditioner=0.01,
                   grad_clip_max_norm=1.0 if clip else None, **kw)

    def closure():
        sq = torch._foreach_mul(params, params)
        return 0.5 * torch.stack([s.sum() for s in sq]).float().sum()
    return params, opt, closure


def closure_only(params, closure):
    """what a step spends outside the optimizer's own code: loss, gradient, Hessian-vector product (psgd.py:706-714)"""
    with torch.enable_grad():
        grads = torch.autograd.grad(closure(), params, create_graph=True)
        vs = [torch.randn_like(p) for p in params]
        torch.autograd.grad(grads, params, vs)


def timed(fn, steps, chunks, warm_seconds):
    torch.cuda.synchronize()
    busy, n = 0.0, 0
    while busy < warm_seconds or n < 5:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        busy += time.perf_counter() - t0
        n += 1
    out = []
    for _ in range(chunks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps)
    return statistics.median(out), min(out), max(out)


def peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


MOMENTUM_LEGS = {"plain": {}, "momentum": {"momentum": 0.9}, "momentum+decay": {"momentum": 0.9, "weight_decay": 0.01}}


def momentum_table(a):
    """the fused step with and without the momentum buffer and the decay term; N floats more to read per step is the expected cost
    of momentum, nothing that of decay"""
    legs = a.legs.split(",")
    print("# fused tail, fp32, r = 20, 256 tensors | leg: median step [min .. max] us, peak bytes over 3 steps   (root: %s)" % _root)
    for N in ([4_000_000] if a.quick else [4_000_000, 100_000_000]):
        steps = a.steps if N <= 4_000_000 else max(5, a.steps // 4)
        for clip in (False, True):
            row = "N=%d r=20 k=256 float32 clip=%s |" % (N, "on" if clip else "off")
            for leg in legs:
                params, opt, closure = build(N, 20, 256, torch.float32, clip, "fused", **MOMENTUM_LEGS[leg])
                med, lo, hi = timed(lambda: opt.step(closure), steps, a.chunks, a.warm_seconds)
                peak = peak_delta(lambda: opt.step(closure))
                row += " %s: %.1f [%.1f .. %.1f] us, peak +%d B |" % (leg, med * 1e6, lo * 1e6, hi * 1e6, peak)
                del params, opt, closure
                torch.cuda.empty_cache()
            print(row, flush=True)


GUARD_LEGS = {"plain": {}, "guard": {"nonfinite": "skip"}, "guard+scale": {"nonfinite": "skip", "loss_scale": 2.0 ** 10},
              "momentum": {"momentum": 0.9}, "guard+momentum": {"nonfinite": "skip", "momentum": 0.9}}


def guard_table(a):
    """the fused step unguarded and guarded, in the same job and alternating (--rounds passes over the legs): a guarded step packs
    with the check (the bytes of the plain pack), reads 16 bytes back on the host -- which also ends the host's run-ahead of the
    device -- and with momentum reads the gradients once more"""
    legs = a.legs.split(",")
    print("# fused tail, fp32, r = 20, 256 tensors, clip on | leg: median step [min .. max] us   (root: %s)" % _root)
    for N in ([4_000_000] if a.quick else [4_000_000, 100_000_000]):
        steps = a.steps if N <= 4_000_000 else max(5, a.steps // 4)
        for rnd in range(a.rounds):
            row = "N=%d r=20 k=256 float32 round %d |" % (N, rnd)
            for leg in legs:
                params, opt, closure = build(N, 20, 256, torch.float32, True, "fused", **GUARD_LEGS[leg])
                med, lo, hi = timed(lambda: opt.step(closure), steps, a.chunks, a.warm_seconds)
                assert getattr(opt, "skipped_steps", 0) == 0
                row += " %s: %.1f [%.1f .. %.1f] us |" % (leg, med * 1e6, lo * 1e6, hi * 1e6)
                del params, opt, closure
                torch.cuda.empty_cache()
            print(row, flush=True)


WHITENING_LEGS = {"whitening": {"preconditioner_fit": "whitening"}, "exact": {}, "fd": {"exact_hessian_vector_product": False},
                  "parent": {}}


def _parent_module(path):
    """the parent commit's UVd module, loaded as a sibling inside the package (its relative imports resolve to this checkout)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("psgd_tf_amd._parent_psgd", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def whitening_table(a):
    """the fused step with the whitening fit (one backward, one multi_randn launch) against the two Hessian steps (a double
    backward; a second closure call on perturbed parameters), in one job with the legs alternating.  The closure of this tool
    costs next to nothing, so the difference is the floor of what the second backward costs; "parent": the default step of the
    parent commit's module, which must equal "exact" to within the spread"""
    global psgd
    legs = a.legs.split(",")
    mine, parent = psgd, _parent_module(a.parent_module) if a.parent_module else None
    if parent is None:
        legs = [leg for leg in legs if leg != "parent"]
    print("# fused tail, fp32, r = 20, 256 tensors, clip on | leg: median step [min .. max] us   (root: %s)" % _root)
    for N in ([4_000_000] if a.quick else [4_000_000, 100_000_000]):
        steps = a.steps if N <= 4_000_000 else max(5, a.steps // 4)
        for rnd in range(a.rounds):
            row = "N=%d r=20 k=256 float32 round %d |" % (N, rnd)
            for leg in legs:
                psgd = parent if leg == "parent" else mine
                try:
                    params, opt, closure = build(N, 20, 256, torch.float32, True, "fused", **WHITENING_LEGS[leg])
                finally:
                    psgd = mine
                med, lo, hi = timed(lambda: opt.step(closure), steps, a.chunks, a.warm_seconds)
                row += " %s: %.1f [%.1f .. %.1f] us |" % (leg, med * 1e6, lo * 1e6, hi * 1e6)
                del params, opt, closure
                torch.cuda.empty_cache()
            print(row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tail", choices=["torch", "fused", "both"], default="both")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--chunks", type=int, default=7)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--trace", nargs=3, metavar=("N", "K", "TAIL"))
    ap.add_argument("--momentum", action="store_true", help="the momentum / weight-decay table instead of the tail table")
    ap.add_argument("--guard", action="store_true", help="the guarded-step table instead of the tail table")
    ap.add_argument("--whitening", action="store_true", help="the whitening-fit table instead of the tail table")
    ap.add_argument("--parent-module", default=None, help="with --whitening: the parent commit's UVd module file (leg 'parent')")
    ap.add_argument("--rounds", type=int, default=2, help="with --guard / --whitening: passes over the legs")
    ap.add_argument("--legs", default=None, help="with --momentum / --guard: which legs (comma-separated; default: all)")
    ap.add_argument("--root", default=None, help="import the package from this checkout instead of the tool's own")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    if a.legs is None:
        a.legs = ",".join(WHITENING_LEGS if a.whitening else GUARD_LEGS if a.guard else MOMENTUM_LEGS)
    if a.whitening:
        assert a.chunks >= 7 and all(leg in WHITENING_LEGS for leg in a.legs.split(","))
        return whitening_table(a)
    if a.guard:
        assert a.chunks >= 7 and all(leg in GUARD_LEGS for leg in a.legs.split(","))
        return guard_table(a)
    if a.momentum:
        assert a.chunks >= 7 and all(leg in MOMENTUM_LEGS for leg in a.legs.split(","))
        return momentum_table(a)
    if a.trace:
        N, k, tail = int(a.trace[0]), int(a.trace[1]), a.trace[2]
        params, opt, closure = build(N, 10 if N <= 1_000_000 else 20, k, torch.float32, True, tail)
        for _ in range(20):
            opt.step(closure)
        torch.cuda.synchronize()
        print("trace: 20 steps, N=%d k=%d tail=%s clip=on fp32" % (N, k, tail))
        return
    assert a.chunks >= 7
    tails = ["torch", "fused"] if a.tail == "both" else [a.tail]
    shapes = [(1_000_000, 10, 1), (1_000_000, 10, 16), (1_000_000, 10, 256)] + ([] if a.quick else [(100_000_000, 20, 256)])
    print("# N r k dtype clip | route: median step [min .. max] us, peak bytes over 3 steps | closure alone us")
    for N, r, k in shapes:
        steps = a.steps if N <= 1_000_000 else max(5, a.steps // 4)
        for dtype in (torch.float32, torch.bfloat16):
            for clip in (False, True):
                row = "N=%d r=%d k=%d %s clip=%s |" % (N, r, k, str(dtype).replace("torch.", ""), "on" if clip else "off")
                for tail in tails:
                    params, opt, closure = build(N, r, k, dtype, clip, tail)
                    med, lo, hi = timed(lambda: opt.step(closure), steps, a.chunks, a.warm_seconds)
                    peak = peak_delta(lambda: opt.step(closure))
                    row += " %s: %.1f [%.1f .. %.1f] us, peak +%d B |" % (tail, med * 1e6, lo * 1e6, hi * 1e6, peak)
                    if tail == tails[-1]:
                        c, _, _ = timed(lambda: closure_only(params, closure), steps, a.chunks, a.warm_seconds)
                        row += " closure: %.1f us" % (c * 1e6)
                    del params, opt, closure
                    torch.cuda.empty_cache()
                print(row, flush=True)


if __name__ == "__main__":
    main()
