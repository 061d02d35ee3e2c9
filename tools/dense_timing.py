"""Device time per call of the dense preconditioner (update_precond_dense, precond_grad_dense), native kernels against the
torch-op route (set_dense_route("torch")), fp32 on one GPU.  Per call: hipEvents around each call, warm-up calls first, the
median of --reps calls.  Per-kernel numbers: run under `rocprofv3 --kernel-trace --stats` (e.g. --sizes 8192) and read with
tools/rocpd_stats.py."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="400,1024,2048,4096,8192,16384")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--routes", default="native,torch")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("%-6s %6s %12s %12s" % ("route", "N", "update ms", "apply ms"), flush=True)
    res = {}
    for n in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator(device=dev).manual_seed(n)
        Q = torch.triu(torch.randn(n, n, device=dev, generator=g) * (0.3 / n ** 0.5), 1)
        Q += torch.diag(torch.exp(torch.empty(n, device=dev).uniform_(-1.0, 1.0, generator=g)))
        dx, dg, gr = (torch.randn(n, device=dev, generator=g) for _ in range(3))
        for route in args.routes.split(","):
            psgd.set_dense_route(route)
            upd = time_ms(lambda: psgd.update_precond_dense(Q, [dx], [dg], step=0.01), args.warmup, args.reps)
            app = time_ms(lambda: psgd.precond_grad_dense(Q, [gr]), args.warmup, args.reps)
            res[(route, n)] = (upd, app)
            print("%-6s %6d %12.4f %12.4f" % (route, n, upd, app), flush=True)
        psgd.set_dense_route("native")
        del Q
        torch.cuda.empty_cache()
    if "torch" in args.routes and "native" in args.routes:
        print("speed-up of the native route (torch / native):")
        for n in sorted({k[1] for k in res}):
            (tu, ta), (nu, na) = res[("torch", n)], res[("native", n)]
            print("  N=%6d  update %7.1fx  apply %7.1fx" % (n, tu / nu, ta / na))


if __name__ == "__main__":
    main()
