"""Device time of the QUAD Kronecker update and apply with one diagonal side (psgd_kron_qdiag.hip) beside the triangular
update_precond_kron / precond_grad_kron in the same format on whitening inputs (dX = a probe, dG = the gradient), fp32 on one GPU;
writes profiles/kron_quad_diag_timing.txt.

Method (tools/kron_quad_timing.py's): hipEvents around chunks of --calls back-to-back calls, every leg warmed up first, the legs
ALTERNATING chunk by chunk, the median over --chunks chunks per leg and the spread (max - min) between chunks.  The flops are those
the kernels issue (quad_diag_flops below); "of peak" is that count over the median time over the fp32 matrix-core rate of the
MI355X, 157.3 TFLOP/s -- a rate of the whole call, launches and the Lipschitz kernel included.  The longer extent of a shape is the diagonal
side: 32768x1024 runs in (scale, dense), 1024x32768 in (dense, scale).

The A/B of the slice rule: S is a compile-time rule, so the legs are libraries -- build psgd_kron_qdiag.hip with
-DPSGD_QDIAG_SLICE_TARGET=1 (S = 1) or another target into libraries of their own and run this tool once per library
with PSGD_HIP_LIB=<library> --label <name> --shapes 32768x1024 --append, the runs alternating in one job."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from psgd_tf_amd import kron_quad_diag  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def quad_diag_flops(D, n):
    """(update, apply): the scaled product, the upper tiles of the Gram, T Q and both tiles of P1 T; two products"""
    nb = -(-n // 64)
    return 2 * D * n * n + D * n * n * (nb + 1) // nb + 4 * n ** 3, 4 * D * n * n


def chunk_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def legs_for(M, N, dev):
    formats = ("scale", "dense") if M >= N else ("dense", "scale")
    gen = torch.Generator(device=dev).manual_seed(M * 7919 + N)
    G, V = (torch.randn(M, N, device=dev, generator=gen) for _ in range(2))
    Ql, Qr, L = psgd.kron_quad_initial_state(M, N, device=dev, formats=formats)
    Tl, Tr, _ = psgd.kron_quad_initial_state(M, N, device=dev, formats=formats)      # identity is upper triangular too
    out = torch.empty(M, N, device=dev)
    return {
        "quad update": lambda: psgd.update_precond_kron_quad_(Ql, Qr, L, G, 1e-3),
        "triangular update": lambda: psgd.update_precond_kron(Tl, Tr, V, G, 1e-3),
        "quad apply": lambda: psgd.precond_grad_kron_quad(Ql, Qr, G, out=out),
        "triangular apply": lambda: psgd.precond_grad_kron(Tl, Tr, G),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32768x1024,131072x1024,1024x32768,4096x64")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--label", default="")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_quad_diag_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "kron_quad_diag_timing needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = ["kron quad diag timing%s on %s: median of %d chunks of %d calls, legs alternating; fp32 MFMA peak %.1f TFLOP/s"
             % (" [%s]" % args.label if args.label else "", torch.cuda.get_device_name(dev), args.chunks, args.calls, PEAK_F32_MFMA / 1e12),
             "%-14s %-18s %3s %10s %10s %10s %8s" % ("M x N", "call", "S", "ms", "spread ms", "GFLOP", "of peak")]
    for M, N in [tuple(int(n) for n in s.split("x")) for s in args.shapes.split(",")]:
        legs = legs_for(M, N, dev)
        S = kron_quad_diag.slices(M, N, 0 if M >= N else 1)
        flops = dict(zip(("quad update", "quad apply"), quad_diag_flops(max(M, N), min(M, N))))
        times = {k: [] for k in legs}
        for fn in legs.values():                                       # warm-up: code objects, workspaces, clocks
            chunk_ms(fn, 2)
        for _ in range(args.chunks):
            for k, fn in legs.items():
                times[k].append(chunk_ms(fn, args.calls))
        for k in legs:
            ms, spread = statistics.median(times[k]), max(times[k]) - min(times[k])
            f = flops.get(k)
            tail = "%10.1f %7.1f%%" % (f / 1e9, 100 * f / (ms * 1e-3) / PEAK_F32_MFMA) if f else "%10s %8s" % ("-", "-")
            lines.append("%-14s %-18s %3s %10.4f %10.4f %s" % ("%d x %d" % (M, N), k, S if k == "quad update" else "-", ms, spread, tail))
            print(lines[-1], flush=True)
        del legs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
