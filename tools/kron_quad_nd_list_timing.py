"""Device time of the QUAD update and apply on LISTS of order-3 tensor layers: the grouped route of kron_quad_nd_list.py
(psgd_kron_qtlist.hip: at most eight and six launches per group, the Gram of a short side split along K) beside the per-layer loop
over kron_quad_nd.py (seven and six per layer), on the same commit and library, fp32 on one GPU.  Writes
profiles/kron_quad_nd_list_timing.txt.

Method (tools/kron_quad_list_timing.py's): hipEvents around chunks of --calls back-to-back calls, every leg warmed up first, the
legs ALTERNATING chunk by chunk, the median over --chunks chunks per leg and the spread (max - min) between chunks.  A difference
between two legs that is smaller than the larger of their spreads is marked "not resolved".  --slice-k adds the list update under
other values of gram_slice_k (state of their own) on the sets named by --slice-sets.

Launch counts come from a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/kron_quad_nd_list_timing.py --launches
runs ONE update and ONE apply per route on the 16 x (64 x 64 x 9) set and nothing else; then
    python tools/kron_quad_nd_list_timing.py --launch-stats <dir> --append
adds the calls of the grouped kernels (k_tl_*) and of the per-layer ones to the profile."""
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
from psgd_tf_amd import kron_quad_nd_list as qtl  # noqa: E402
from tools.kron_quad_list_timing import chunk_ms  # noqa: E402

# ResNet-18-like: the 3 x 3 kernels of the four stages and the 1 x 1 kernels of the three downsampling shortcuts
RESNET18 = ([(64, 64, 9)] * 4 + [(128, 64, 9), (128, 64, 1)] + [(128, 128, 9)] * 3 + [(256, 128, 9), (256, 128, 1)] + [(256, 256, 9)] * 3
            + [(512, 256, 9), (512, 256, 1)] + [(512, 512, 9)] * 3)
SETS = {
    "16x(64x64x9)": [(64, 64, 9)] * 16,
    "8x(128x128x9)": [(128, 128, 9)] * 8,
    "4x(256x256x9)": [(256, 256, 9)] * 4,
    "resnet18": RESNET18,
    "1x(512x512x9)": [(512, 512, 9)],
}
CALLS = {"resnet18": 2, "1x(512x512x9)": 3}                # fewer calls per chunk where one call is long


def function_legs(shapes, dev, slice_ks=()):
    gen = torch.Generator(device=dev).manual_seed(len(shapes) * 7919 + shapes[0][0])
    Gs = [torch.randn(s, device=dev, generator=gen) for s in shapes]
    state = lambda: [psgd.kron_quad_nd_initial_state(s, device=dev) for s in shapes]
    a, b = state(), state()
    outs = [torch.empty(s, device=dev) for s in shapes]
    plan = psgd.KronQuadTensorListPlan(shapes, dev)
    col = lambda st, j: [s[j] for s in st]

    def layer_update():
        for (Qs, L), G in zip(b, Gs):
            psgd.update_precond_kron_quad_nd_(Qs, L, G, 1e-3)

    def layer_apply():
        for (Qs, _), G, out in zip(b, Gs, outs):
            psgd.precond_grad_kron_quad_nd(Qs, G, out=out)

    legs = {
        "list update": lambda: psgd.update_precond_kron_quad_nd_list_(col(a, 0), col(a, 1), Gs, 1e-3, plan=plan),
        "layer update": layer_update,
        "list apply": lambda: psgd.precond_grad_kron_quad_nd_list(col(a, 0), Gs, outs, plan=plan),
        "layer apply": layer_apply,
    }
    for gsk in slice_ks:
        c, p = state(), psgd.KronQuadTensorListPlan(shapes, dev, gram_slice_k=gsk)
        legs["list@%d update" % gsk] = lambda c=c, p=p: psgd.update_precond_kron_quad_nd_list_(col(c, 0), col(c, 1), Gs, 1e-3, plan=p)
    return plan, legs


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


def launch_stats(directory):
    counts, names = {"list": 0, "layer": 0}, {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name, calls = row["Name"], int(row["Calls"])
            if "psgdq" in name and "k_" in name:                       # demangled or mangled: psgdqt::k_tl_*, psgdqn::k_*
                counts["list" if "k_tl_" in name else "layer"] += calls
                names[name.split("(")[0]] = names.get(name.split("(")[0], 0) + calls
    assert names, "no QUAD kernel in the stats under %s" % directory
    lines = ["launches of one update + one apply on 16 x (64 x 64 x 9) (kernel-stats run, one call per route): list route %d, "
             "per-layer route %d" % (counts["list"], counts["layer"])]
    return lines + ["    %-40s %d" % kv for kv in sorted(names.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--slice-k", default="", help="further values of gram_slice_k, comma-separated: extra list update legs")
    ap.add_argument("--slice-sets", default="resnet18,1x(512x512x9)")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--launch-stats", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kron_quad_nd_list_timing.txt"))
    args = ap.parse_args()
    if args.launch_stats:
        lines = launch_stats(args.launch_stats)
    else:
        assert torch.cuda.is_available(), "kron_quad_nd_list_timing needs a GPU: nothing here is measured without one"
        dev = torch.device("cuda:0")
        if args.launches:                                              # no warm-up, one update and one apply per route
            for fn in function_legs(SETS["16x(64x64x9)"], dev)[1].values():
                fn()
            return torch.cuda.synchronize()
        lines = ["kron quad nd list timing on %s: device ms per call (all layers of the set), median of %d chunks, legs alternating; "
                 "cap %d MiB, gram_slice_k %d unless a leg says @other" % (torch.cuda.get_device_name(dev), args.chunks,
                                                                          qtl.DEFAULT_GROUP_BYTES >> 20, qtl.DEFAULT_GRAM_SLICE_K),
                 "%-15s %-18s %10s %10s   %s" % ("set", "leg", "ms", "spread ms", "verdict")]
        for name in args.sets.split(","):
            ks = [int(c) for c in args.slice_k.split(",") if c] if name in args.slice_sets.split(",") else []
            plan, legs = function_legs(SETS[name], dev, ks)
            lines.append("%-15s %d layers in %d group(s); distinct (shape, slices): %s" % (
                name, len(SETS[name]), len(plan.groups), sorted(set(zip(plan.shapes, plan.slices)))))
            measure(name, legs, CALLS.get(name, args.calls), args.chunks, lines)
            del plan, legs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
