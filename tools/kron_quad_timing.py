"""Device time of the QUAD Kronecker update and apply (psgd_kron_quad.hip) beside the triangular update_precond_kron /
precond_grad_kron on whitening inputs (dX = a probe, dG = the gradient), fp32 on one GPU; writes profiles/kron_quad_timing.txt.

Method: hipEvents around chunks of --calls back-to-back calls (device time: the chunk ends in an event synchronise), every leg
warmed up first, the legs ALTERNATING chunk by chunk so that clock and neighbour drift fall on all of them alike, the median
over --chunks chunks per leg.  The flops are those the QUAD kernels issue, counted from the shapes (quad_flops below: the Gram
launch computes the upper tiles only, the symmetrising launch every tile); "of peak" is that count over the median time over the
fp32 matrix-core rate of the MI355X, 157.3 TFLOP/s -- a rate of the whole call, launches and the one-workgroup Lipschitz kernel
included, not of one kernel.  The factors are reset by nothing: QUAD rewrites them in place, so its step is small (1e-3) and L
keeps every step bounded; the triangular legs return new tensors that are dropped."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def quad_flops(M, N):
    """(update, apply): two products for A, half of A A' and A' A, T Q and P1 T per side; four products"""
    return 2 * M * N * (M + N) + M * N * (M + N) + 4 * (M ** 3 + N ** 3), 4 * M * N * (M + N)


def chunk_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def legs_for(M, N, dev):
    gen = torch.Generator(device=dev).manual_seed(M * 7919 + N)
    G, V = (torch.randn(M, N, device=dev, generator=gen) for _ in range(2))
    Ql, Qr, L = psgd.kron_quad_initial_state(M, N, device=dev)
    Tl, Tr = torch.eye(M, device=dev), torch.eye(N, device=dev)
    out = torch.empty(M, N, device=dev)
    return {
        "quad update": lambda: psgd.update_precond_kron_quad_(Ql, Qr, L, G, 1e-3),
        "triangular update": lambda: psgd.update_precond_kron(Tl, Tr, V, G, 1e-3),
        "quad apply": lambda: psgd.precond_grad_kron_quad(Ql, Qr, G, out=out),
        "triangular apply": lambda: psgd.precond_grad_kron(Tl, Tr, G),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x256,1024x1024,768x3072,1024x4096,4096x4096")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_quad_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kron_quad_timing needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = ["kron quad timing on %s: median of %d chunks of %d calls, legs alternating; fp32 MFMA peak %.1f TFLOP/s"
             % (torch.cuda.get_device_name(dev), args.chunks, args.calls, PEAK_F32_MFMA / 1e12),
             "%-12s %-18s %10s %10s %8s" % ("M x N", "call", "ms", "GFLOP", "of peak")]
    for M, N in [tuple(int(n) for n in s.split("x")) for s in args.shapes.split(",")]:
        legs = legs_for(M, N, dev)
        flops = dict(zip(("quad update", "quad apply"), quad_flops(M, N)))
        times = {k: [] for k in legs}
        for fn in legs.values():                                       # warm-up: code objects, workspaces, clocks
            chunk_ms(fn, 2)
        for _ in range(args.chunks):
            for k, fn in legs.items():
                times[k].append(chunk_ms(fn, args.calls))
        for k in legs:
            ms = statistics.median(times[k])
            f = flops.get(k)
            tail = "%10.1f %7.1f%%" % (f / 1e9, 100 * f / (ms * 1e-3) / PEAK_F32_MFMA) if f else "%10s %8s" % ("-", "-")
            lines.append("%-12s %-18s %10.4f %s" % ("%d x %d" % (M, N), k, ms, tail))
            print(lines[-1], flush=True)
        del legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
