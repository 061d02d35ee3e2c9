"""Device time of the QUAD update and apply on LISTS of (dense, dense) layers: the grouped route of kron_quad_list.py
(psgd_kron_qlist.hip: six and four launches per group) beside the per-layer loop over kron_quad.py (six and four per layer), on
the same commit and library, fp32 on one GPU; and the whole Kron.step with quad_route="list" and "layer".  Writes
profiles/kron_quad_list_timing.txt.

Method (tools/kron_quad_diag_timing.py's): hipEvents around chunks of --calls back-to-back calls, every leg warmed up first, the
legs ALTERNATING chunk by chunk, the median over --chunks chunks per leg and the spread (max - min) between chunks.  A difference
between two legs that is smaller than the larger of their spreads is marked "not resolved".

Launch counts come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kron_quad_list_timing.py --launches
runs ONE update and ONE apply per route on the 48 x 256^2 set and nothing else; then
    python tools/kron_quad_list_timing.py --launch-stats <dir> --append
adds the calls of the grouped kernels (k_list_*) and of the per-layer ones to the profile."""
import argparse
import csv
import glob
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

LENET5 = [(26, 6), (151, 16), (257, 120), (121, 84), (85, 10)]
SETS = {
    "lenet5": LENET5,
    "48x256^2": [(256, 256)] * 48,
    "24x(256x1024)": [(256, 1024)] * 24,
    "12x(768x3072)": [(768, 3072)] * 12,
    "mixed": LENET5 + [(256, 256)] * 12 + [(256, 1024)] * 6 + [(768, 3072)] * 2,
}
CALLS = {"12x(768x3072)": 2, "mixed": 3}                   # fewer calls per chunk where one call is long


def chunk_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def function_legs(shapes, dev, caps=()):
    gen = torch.Generator(device=dev).manual_seed(len(shapes) * 7919 + shapes[0][0])
    Gs = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    a, b = ([psgd.kron_quad_initial_state(M, N, device=dev) for M, N in shapes] for _ in range(2))
    outs = [torch.empty(s, device=dev) for s in shapes]
    plan = psgd.KronQuadListPlan(shapes, dev)
    col = lambda state, j: [s[j] for s in state]

    def layer_update():
        for (Ql, Qr, L), G in zip(b, Gs):
            psgd.update_precond_kron_quad_(Ql, Qr, L, G, 1e-3)

    def layer_apply():
        for (Ql, Qr, _), G, out in zip(b, Gs, outs):
            psgd.precond_grad_kron_quad(Ql, Qr, G, out=out)

    legs = {
        "list update": lambda: psgd.update_precond_kron_quad_list_(col(a, 0), col(a, 1), col(a, 2), Gs, 1e-3, plan=plan),
        "layer update": layer_update,
        "list apply": lambda: psgd.precond_grad_kron_quad_list(col(a, 0), col(a, 1), Gs, outs, plan=plan),
        "layer apply": layer_apply,
    }
    for mib in caps:                                                   # --caps: the list legs again under other caps (state of their own)
        c = [psgd.kron_quad_initial_state(M, N, device=dev) for M, N in shapes]
        p = psgd.KronQuadListPlan(shapes, dev, max_group_bytes=mib << 20)
        legs["list@%dM update" % mib] = lambda c=c, p=p: psgd.update_precond_kron_quad_list_(col(c, 0), col(c, 1), col(c, 2), Gs, 1e-3, plan=p)
        legs["list@%dM apply" % mib] = lambda c=c, p=p: psgd.precond_grad_kron_quad_list(col(c, 0), col(c, 1), Gs, outs, plan=p)
    return plan, legs


def step_legs(shapes, dev):
    legs = {}
    for route in ("list", "layer"):
        gen = torch.Generator(device=dev).manual_seed(11)
        params = [torch.randn(s, device=dev, generator=gen).requires_grad_() for s in shapes]
        targets = [torch.randn(s, device=dev, generator=gen) for s in shapes]
        opt = psgd.Kron(params, "dense", 1.0, 1e-3, 1e-3, preconditioner_fit="whitening", probe_seed=3, preconditioner_update="quad",
                        generator=torch.Generator().manual_seed(1), quad_route=route)
        closure = lambda params=params, targets=targets: sum(((x - t) ** 2).sum() for x, t in zip(params, targets))
        legs["%s Kron.step" % route] = lambda opt=opt, closure=closure: opt.step(closure)
    return legs


def measure(name, legs, calls, chunks, lines):
    times = {k: [] for k in legs}
    for fn in legs.values():                                           # warm-up: code objects, workspaces, tables, clocks
        chunk_ms(fn, 2)
    for _ in range(chunks):
        for k, fn in legs.items():
            times[k].append(chunk_ms(fn, calls))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    for k in legs:
        note = ""
        if k.startswith("list"):
            other = "layer " + k.split(" ", 1)[1]
            diff, noise = med[other] - med[k], max(spread[k], spread[other])
            note = "layer / list = %.2f" % (med[other] / med[k]) if abs(diff) > noise else "not resolved"
        lines.append("%-15s %-18s %10.4f %10.4f   %s" % (name, k, med[k], spread[k], note))
        print(lines[-1], flush=True)


def one_call_per_route(dev):
    """what the kernel-stats run traces: no warm-up, one update and one apply per route"""
    _, legs = function_legs(SETS["48x256^2"], dev)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()


def launch_stats(directory):
    counts = {"list": 0, "layer": 0}
    names = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name, calls = row["Name"], int(row["Calls"])
            if "psgdq::k_" in name or "psgdq1" in name:                # demangled or mangled
                counts["list" if "k_list_" in name else "layer"] += calls
                names[name.split("(")[0]] = names.get(name.split("(")[0], 0) + calls
    assert names, "no QUAD kernel in the stats under %s" % directory
    lines = ["launches of one update + one apply on 48 x 256^2 (kernel-stats run, one call per route): list route %d, per-layer route %d"
             % (counts["list"], counts["layer"])]
    return lines + ["    %-40s %d" % kv for kv in sorted(names.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--caps", default="", help="further caps in MiB, comma-separated: extra list legs beside the default cap's")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--launch-stats", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_quad_list_timing.txt"))
    args = ap.parse_args()
    if args.launch_stats:
        lines = launch_stats(args.launch_stats)
    else:
        assert torch.cuda.is_available(), "kron_quad_list_timing needs a GPU: nothing here is measured without one"
        dev = torch.device("cuda:0")
        if args.launches:
            return one_call_per_route(dev)
        lines = ["kron quad list timing on %s: device ms per call (all layers of the set), median of %d chunks, legs alternating; cap %d MiB"
                 % (torch.cuda.get_device_name(dev), args.chunks, psgd.KronQuadListPlan([(1, 1)], dev).max_group_bytes >> 20),
                 "%-15s %-18s %10s %10s   %s" % ("set", "leg", "ms", "spread ms", "groups / verdict")]
        for name in args.sets.split(","):
            plan, legs = function_legs(SETS[name], dev, [int(c) for c in args.caps.split(",") if c])
            lines.append("%-15s %d layers in %d group(s) of %s" % (name, len(SETS[name]), len(plan.groups), [g1 - g0 for g0, g1 in plan.groups]))
            measure(name, legs, CALLS.get(name, args.calls), args.chunks, lines)
            del plan, legs
            torch.cuda.empty_cache()
        if not args.no_step:
            measure("48x256^2", step_legs(SETS["48x256^2"], dev), args.calls, args.chunks, lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
