"""Device time of the three-factor QUAD update and apply (psgd_kron_qnd.hip) on tensors [s0, s1, s2], beside the two-factor QUAD
(psgd_kron_quad.hip) on the folded view [s0, s1 s2] of the same gradient, fp32 on one GPU; writes profiles/kron_quad_nd_timing.txt.

The two are DIFFERENT preconditioners (three factors s0^2, s1^2, s2^2 against two, s0^2 and (s1 s2)^2): the table sets their cost
and their state bytes side by side, it ranks no kernel against another.

Method, that of tools/kron_quad_timing.py: hipEvents around chunks of --calls back-to-back calls (device time: the chunk ends in
an event synchronise), every leg warmed up first, the legs ALTERNATING chunk by chunk so that clock and neighbour drift fall on
all of them alike, the median over --chunks chunks per leg, with the smallest and largest chunk beside it.  The factors are reset
by nothing: QUAD rewrites them in place, so its step is small (1e-3) and L keeps every step bounded.

A folded layer whose state would pass --folded-cap bytes (12 x 768 x 64 folds to 12 x 49152: a 9.7 GB right factor and about
4.8e14 flops per update) is not run; its row records the state bytes it would need."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


def chunk_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def legs_for(shape, dev, folded_cap):
    """({leg: call}, {route: bytes of factors and L}); the folded legs are None when their state would pass folded_cap bytes"""
    A, B, C = shape
    gen = torch.Generator(device=dev).manual_seed(A * 7919 + B * 31 + C)
    G = torch.randn(A, B, C, device=dev, generator=gen)
    G2 = G.view(A, B * C)
    Qs, L3 = psgd.kron_quad_nd_initial_state(shape, device=dev)
    out, out2 = torch.empty_like(G), torch.empty_like(G2)
    state = {"three-factor": 4 * (sum(Q.numel() for Q in Qs) + 3), "folded": 4 * (A * A + (B * C) ** 2 + 2)}
    legs = {"three-factor update": lambda: psgd.update_precond_kron_quad_nd_(Qs, L3, G, 1e-3), "folded update": None,
            "three-factor apply": lambda: psgd.precond_grad_kron_quad_nd(Qs, G, out=out), "folded apply": None}
    if state["folded"] <= folded_cap:
        Ql, Qr, L2 = psgd.kron_quad_initial_state(A, B * C, device=dev)
        legs["folded update"] = lambda: psgd.update_precond_kron_quad_(Ql, Qr, L2, G2, 1e-3)
        legs["folded apply"] = lambda: psgd.precond_grad_kron_quad(Ql, Qr, G2, out=out2)
    return legs, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x64x9,256x256x9,512x512x9,12x768x64")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--folded-cap", type=int, default=2 ** 31, help="largest folded state, in bytes, that is still timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_quad_nd_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kron_quad_nd_timing needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = ["kron quad nd timing on %s: median (min .. max) of %d chunks of %d calls, legs alternating; folded = two-factor QUAD on "
             "[s0, s1 s2]" % (torch.cuda.get_device_name(dev), args.chunks, args.calls),
             "%-14s %-20s %10s %22s %14s" % ("s0 x s1 x s2", "call", "ms", "(min .. max)", "state bytes")]
    for shape in [tuple(int(n) for n in s.split("x")) for s in args.shapes.split(",")]:
        legs, state = legs_for(shape, dev, args.folded_cap)
        run = {k: fn for k, fn in legs.items() if fn is not None}
        times = {k: [] for k in run}
        for fn in run.values():                                        # warm-up: code objects, workspaces, clocks
            chunk_ms(fn, 2)
        for _ in range(args.chunks):
            for k, fn in run.items():
                times[k].append(chunk_ms(fn, args.calls))
        for k in legs:
            if k not in run:
                lines.append("%-14s %-20s %10s %22s %14d" % ("%d x %d x %d" % shape, k, "not run", "(state over the cap)", state["folded"]))
                print(lines[-1], flush=True)
                continue
            lines.append("%-14s %-20s %10.4f %22s %14d" % ("%d x %d x %d" % shape, k, statistics.median(times[k]),
                                                           "(%.4f .. %.4f)" % (min(times[k]), max(times[k])), state[k.split()[0]]))
            print(lines[-1], flush=True)
        del legs, run
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
