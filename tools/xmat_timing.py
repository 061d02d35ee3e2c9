"""Device time of the X-shaped preconditioner's three calls (psgd_xmat.hip), with the fused UVd r = 20 step at the same N beside
them, fp32 on one GPU; writes profiles/xmat_timing.txt (--out).

Method: hipEvents around chunks of --calls back-to-back calls (device time: the chunk ends in an event synchronise), every
leg warmed up first, the legs ALTERNATING chunk by chunk so that clock and neighbour drift fall on all of them alike, the median
over --chunks chunks per leg.  Bytes per parameter are the algorithm's (apply: a, b, g read, out written = 16; update: a, b, v,
h read twice, a, b written = 40; fused = 48 with g and out); the diagonal form moves 12 / 28 / 36.  TB/s = those bytes over the
median time: a rate of the whole call, not of one kernel.  The last section runs the whitening fit of examples/xmat_class.py
and records the spread of diag(Q'Q) sigma_g after 500 steps."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from examples.xmat_class import whiten  # noqa: E402

TINY = float(torch.finfo(torch.float32).tiny)
BYTES = {"apply": (16, 12), "update": (40, 28), "fused": (48, 36)}     # per parameter: (X-shaped, diagonal)
REWRITE_RATE = "5.3-5.4 TB/s"                                          # README: the project's in-place rewrite of a large stream


def chunk_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def legs_for(N, dev, uvd_rank):
    gen = torch.Generator(device=dev).manual_seed(N)
    a = torch.exp(torch.rand(N, device=dev, generator=gen) * 2 - 1)
    b = 0.3 * torch.minimum(a, a.flip(0)) * (torch.rand(N, device=dev, generator=gen) * 2 - 1)
    v, h, g = (torch.randn(N, device=dev, generator=gen) for _ in range(3))
    out, ad = torch.empty(N, device=dev), a.clone()
    legs = {
        "apply": lambda: psgd.precond_grad_Xmat_math(a, b, g, out=out),
        "update": lambda: psgd.update_precond_Xmat_math_(a, b, v, h, 0.01, TINY),
        "fused": lambda: psgd.update_precond_grad_Xmat_math_(a, b, v, h, g, 0.01, TINY, out=out),
        "fused diagonal": lambda: psgd.update_precond_grad_Xmat_math_(ad, None, v, h, g, 0.01, TINY, out=out),
    }
    if uvd_rank:
        s = (1.0 / (N * uvd_rank)) ** 0.5
        U, V = (torch.randn(N, uvd_rank, device=dev, generator=gen) * s for _ in range(2))
        d, cols = torch.ones(N, 1, device=dev), [x[:, None] for x in (v, h, g)]
        legs["UVd r=%d fused" % uvd_rank] = lambda: psgd.update_precond_UVd_math_and_precond_grad(
            U, V, d, *cols, 0.01, TINY, balance=False, update_U=True, out=out[:, None])
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,4000000,100000000,100000001")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--uvd-rank", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xmat_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "xmat_timing needs a GPU: nothing here is measured without one"
    dev = torch.device("cuda:0")
    lines = ["xmat timing on %s: median of %d chunks of %d calls, legs alternating; in-place rewrite rate of the project: %s"
             % (torch.cuda.get_device_name(dev), args.chunks, args.calls, REWRITE_RATE),
             "%-10s %-18s %10s %8s %8s" % ("N", "call", "ms", "B/param", "TB/s")]
    for N in [int(s) for s in args.sizes.split(",")]:
        legs = legs_for(N, dev, args.uvd_rank)
        times = {k: [] for k in legs}
        for fn in legs.values():                                       # warm-up: code objects, workspaces, clocks
            chunk_ms(fn, 3)
        for _ in range(args.chunks):
            for k, fn in legs.items():
                times[k].append(chunk_ms(fn, args.calls))
        for k in legs:
            ms = statistics.median(times[k])
            key, diag = k.split()[0], k.endswith("diagonal")
            bpp = BYTES[key][diag] if key in BYTES else None
            rate = "%8.2f" % (bpp * N / (ms * 1e-3) / 1e12) if bpp else "%8s" % "-"
            lines.append("%-10d %-18s %10.4f %8s %s" % (N, k, ms, bpp if bpp else "-", rate))
            print(lines[-1], flush=True)
        del legs
        torch.cuda.empty_cache()
    for diagonal in (False, True):
        w, _ = whiten(diagonal=diagonal)
        lines.append("whitening fit, 256-element quadratic, curvature 0.01 .. 100, 500 steps%s: diag(Q'Q) sigma_g in [%.4f, %.4f], "
                     "median %.4f (1 = whitened)" % (", diagonal" if diagonal else "", float(w.min()), float(w.max()), float(w.median())))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
