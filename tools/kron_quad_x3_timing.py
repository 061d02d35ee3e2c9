"""Device time of the QUAD Kronecker update and apply on the bf16 x 3 product core (products="bf16x3", psgd_kron_quad_x3.hip)
beside the fp32 route (psgd_kron_quad.hip) and the triangular update_precond_kron / precond_grad_kron, all from one library in
one job on one GPU; writes profiles/kron_quad_x3_timing.txt.

Method: hipEvents around chunks of --calls back-to-back calls (device time: the chunk ends in an event synchronise), every leg
warmed up first, the legs ALTERNATING chunk by chunk so that clock and neighbour drift fall on all of them alike; the median and
the spread (min .. max) over --chunks chunks per leg.  The flops are those of the algorithm, counted from the shapes as in
tools/kron_quad_timing.py; the bf16 x 3 core issues SIX bf16 MFMA flops for each, and "of bf16" is 6 x flops over the median time
over the bf16 matrix-core rate of the MI355X (16 x the fp32 one: 2516.8 TFLOP/s) -- a rate of the whole call, launches, the
one-workgroup Lipschitz kernel and the macro-tile padding of small shapes included, not of one kernel.  The ceiling of the speedup
over the fp32 route is 16 / 6.  A route WINS a shape when its slowest chunk of update + apply is faster than the other's fastest;
the last line names the smallest square size from which the new route wins: class Kron's default of quad_products_min_dim."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from tools.kron_quad_timing import chunk_ms, quad_flops  # noqa: E402

PEAK_BF16_MFMA = 16 * 157.3e12
ROUTES = ("fp32", "bf16x3", "triangular")


def legs_for(M, N, dev):
    gen = torch.Generator(device=dev).manual_seed(M * 7919 + N)
    G, V = (torch.randn(M, N, device=dev, generator=gen) for _ in range(2))
    state = {r: psgd.kron_quad_initial_state(M, N, device=dev) for r in ROUTES[:2]}
    Tl, Tr = torch.eye(M, device=dev), torch.eye(N, device=dev)
    out = torch.empty(M, N, device=dev)
    legs = {}
    for r, (Ql, Qr, L) in state.items():
        legs[(r, "update")] = lambda Ql=Ql, Qr=Qr, L=L, r=r: psgd.update_precond_kron_quad_(Ql, Qr, L, G, 1e-3, products=r)
        legs[(r, "apply")] = lambda Ql=Ql, Qr=Qr, r=r: psgd.precond_grad_kron_quad(Ql, Qr, G, out=out, products=r)
    legs[("triangular", "update")] = lambda: psgd.update_precond_kron(Tl, Tr, V, G, 1e-3)
    legs[("triangular", "apply")] = lambda: psgd.precond_grad_kron(Tl, Tr, G)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,512x512,1024x1024,2048x2048,768x3072,1024x4096,4096x4096")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_quad_x3_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kron_quad_x3_timing needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = ["kron quad bf16x3 timing on %s: median (min .. max) of %d chunks of %d calls, legs alternating; bf16 MFMA peak %.1f TFLOP/s"
             % (torch.cuda.get_device_name(dev), args.chunks, args.calls, PEAK_BF16_MFMA / 1e12),
             "%-12s %-11s %-7s %10s %22s %9s %9s" % ("M x N", "route", "call", "ms", "spread ms", "of bf16", "vs fp32")]
    wins = {}
    for M, N in [tuple(int(n) for n in s.split("x")) for s in args.shapes.split(",")]:
        legs = legs_for(M, N, dev)
        flops = dict(zip(("update", "apply"), quad_flops(M, N)))
        times = {k: [] for k in legs}
        for fn in legs.values():                                       # warm-up: code objects, workspaces, clocks
            chunk_ms(fn, 2)
        for _ in range(args.chunks):
            for k, fn in legs.items():
                times[k].append(chunk_ms(fn, args.calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        for (r, call), ms in med.items():
            share = "%8.1f%%" % (100 * 6 * flops[call] / (ms * 1e-3) / PEAK_BF16_MFMA) if r == "bf16x3" else "%9s" % "-"
            lines.append("%-12s %-11s %-7s %10.4f %10.4f .. %8.4f %s %8.2fx" % (
                "%d x %d" % (M, N), r, call, ms, min(times[(r, call)]), max(times[(r, call)]), share, med[("fp32", call)] / ms))
            print(lines[-1], flush=True)
        both = {r: [u + a for u, a in zip(times[(r, "update")], times[(r, "apply")])] for r in ROUTES[:2]}
        wins[(M, N)] = max(both["bf16x3"]) < min(both["fp32"])
        lines.append("%-12s update + apply: bf16x3 %.4f ms, fp32 %.4f ms, %.2fx (ceiling 2.67x): bf16x3 %s" % (
            "%d x %d" % (M, N), statistics.median(both["bf16x3"]), statistics.median(both["fp32"]),
            statistics.median(both["fp32"]) / statistics.median(both["bf16x3"]),
            "wins outside the spread" if wins[(M, N)] else "does NOT win outside the spread"))
        print(lines[-1], flush=True)
        del legs
        torch.cuda.empty_cache()
    squares = sorted(m for (m, n) in wins if m == n)
    from_ = next((m for m in squares if all(wins[(k, k)] for k in squares if k >= m)), None)
    lines.append("quad_products_min_dim: %s" % (from_ if from_ is not None else "none (the new route wins no square shape from here up)"))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
