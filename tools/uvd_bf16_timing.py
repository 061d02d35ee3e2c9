"""Device time per call of the UVd step on one GPU for the four ways to hold the state:
  fp32        U, V, d fp32, the fp32 kernels (psgd_uvd.hip)
  widen       U, V, d stored bf16; .float() x 3 -> the fp32 fused call -> copy_ x 3 (UVd.step with state_route="widen")
  native-rne  U, V, d stored bf16, the bf16-state kernels (psgd_uvd_bf16.hip), round to nearest
  native-sr   the same with stochastic rounding
Per call: hipEvents around each call, warm-up calls first, the median of --reps calls.  B/param is the traffic the native sweeps
are built to move (fused 16 r + 56, update 10 r + 32, apply 6 r + 26 bytes per row) and `of 8 TB/s` the fraction of the HBM peak that
time corresponds to; the other routes print the time only.  Per-kernel numbers: run under `rocprofv3 --kernel-trace --stats`
(e.g. --sizes 100000000 --ranks 20 --routes native-rne --ops fused)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

TINY = float(torch.finfo(torch.float32).tiny)
NATIVE_BYTES = {"fused": lambda r: 16 * r + 56, "update": lambda r: 10 * r + 32, "apply": lambda r: 6 * r + 26}


def time_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def make_ops(route, U, V, d, v, h, g):
    """{op: callable} for one route; step 0 keeps the state where it is over the repetitions (every sweep still runs)"""
    kw = dict(balance=False, update_U=True)
    if route == "widen":
        def fused():
            Uf, Vf, df = U.float(), V.float(), d.float()
            out = psgd.update_precond_UVd_math_and_precond_grad(Uf, Vf, df, v, h, g, 0.0, TINY, **kw)
            U.copy_(Uf); V.copy_(Vf); d.copy_(df)
            return out

        def update():
            Uf, Vf, df = U.float(), V.float(), d.float()
            psgd.update_precond_UVd_math_(Uf, Vf, df, v, h, 0.0, TINY, **kw)
            U.copy_(Uf); V.copy_(Vf); d.copy_(df)

        def apply():
            return psgd.precond_grad_UVd_math(U.float(), V.float(), d.float(), g)
        return {"fused": fused, "update": update, "apply": apply}
    if route.startswith("native"):
        kw.update(rounding="stochastic" if route == "native-sr" else "nearest", rounding_seed=1)
    return {"fused": lambda: psgd.update_precond_UVd_math_and_precond_grad(U, V, d, v, h, g, 0.0, TINY, **kw),
            "update": lambda: psgd.update_precond_UVd_math_(U, V, d, v, h, 0.0, TINY, **kw),
            "apply": lambda: psgd.precond_grad_UVd_math(U, V, d, g)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,20000000,100000000")
    ap.add_argument("--ranks", default="10,20,32")
    ap.add_argument("--routes", default="fp32,widen,native-rne,native-sr")
    ap.add_argument("--ops", default="fused,update,apply")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("%-10s %10s %3s %-6s %10s %8s %10s" % ("route", "N", "r", "op", "ms", "B/param", "of 8 TB/s"), flush=True)
    for N in [int(s) for s in args.sizes.split(",")]:
        for r in [int(s) for s in args.ranks.split(",")]:
            gen = torch.Generator(device=dev).manual_seed(N % 1000 + r)
            v, g = (torch.randn(N, 1, device=dev, generator=gen) for _ in range(2))
            h = v * torch.exp(torch.empty(N, 1, device=dev).uniform_(-2.0, 2.0, generator=gen))
            for route in args.routes.split(","):
                sdt = torch.float32 if route == "fp32" else torch.bfloat16
                U, V = ((torch.randn(N, r, device=dev, generator=gen) * (N * r) ** -0.5).to(sdt) for _ in range(2))
                d = torch.ones(N, 1, device=dev, dtype=sdt)
                ops = make_ops(route, U, V, d, v, h, g)
                for op in args.ops.split(","):
                    ms = time_ms(ops[op], args.warmup, args.reps)
                    if route.startswith("native"):
                        b = NATIVE_BYTES[op](r)
                        print("%-10s %10d %3d %-6s %10.4f %8d %10.3f" % (route, N, r, op, ms, b, b * N / (ms * 1e-3) / 8e12), flush=True)
                    else:
                        print("%-10s %10d %3d %-6s %10.4f %8s %10s" % (route, N, r, op, ms, "-", "-"), flush=True)
                del U, V, d, ops
                torch.cuda.empty_cache()
            del v, h, g
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
