"""Step time of mixed_dtypes=True: the typed step-tail launches once per dtype present against one launch per role.

    python tools/mixed_dtypes_timing.py [--chunks 9] [--steps 50] [--parent DIR]

Whole steps of class UVd (N = 4 M over 256 tensors, r = 10, exact products, clipping and weight decay on); median [min .. max] of
`chunks` chunks of `steps` steps, events around a chunk, the legs alternating chunk by chunk in ONE job (the protocol of
tools/param_groups_timing.py):

  (a) a one-dtype (bfloat16) list, the switch off -- and, with --parent DIR (a checkout of the parent commit, which has no such
      keyword), the same optimizer built from THAT checkout's Python module on the library this process has loaded;
  (b) the same list with mixed_dtypes=True (a one-dtype plan: the launches of (a));
  (c) 256 tensors with D = 2 (bf16 / fp32 in turn) and D = 3 (bf16 / fp32 / fp16), fused tail against torch tail.

The results go to profiles/mixed_dtypes.txt; say there whether the spread of the legs resolves the differences."""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

DEV = torch.device("cuda:0")
BF16, F32, F16 = torch.bfloat16, torch.float32, torch.float16
N, K = 4 << 20, 256


def _parent_module(path):
    """the parent checkout's package under another name; its _lib is replaced by this process's, so both legs call one library"""
    spec = importlib.util.spec_from_file_location("psgd_tf_amd_parent", os.path.join(path, "psgd_tf_amd", "__init__.py"),
                                                  submodule_search_locations=[os.path.join(path, "psgd_tf_amd")])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["psgd_tf_amd_parent"] = pkg
    sys.modules["psgd_tf_amd_parent._lib"] = sys.modules["psgd_tf_amd._lib"]
    spec.loader.exec_module(pkg)
    return sys.modules["psgd_tf_amd_parent.preconditioned_stochastic_gradient_descent"]


def _leg(module, dtypes, tail, **kw):
    params = [torch.randn(N // K, device=DEV).to(T).requires_grad_(True) for T in dtypes]
    a = torch.rand(N, device=DEV) + 0.5
    opt = module.UVd(params, 10, lr_params=1e-3, grad_clip_max_norm=1.0, step_tail=tail, weight_decay=0.01, placement=None,
                     generator=torch.Generator().manual_seed(0), **kw)
    closure = lambda: 0.5 * torch.sum(a * torch.cat([p.reshape(-1).float() for p in params]) ** 2)
    return lambda: opt.step(closure)


def _timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    one, two, three = [BF16] * K, [(BF16, F32)[i % 2] for i in range(K)], [(BF16, F32, F16)[i % 3] for i in range(K)]
    legs = {}
    if args.parent:
        legs["(a) parent module, bf16 list, fused"] = _leg(_parent_module(args.parent), one, "fused")
    legs["(a) this module, bf16 list, switch off, fused"] = _leg(psgd, one, "fused")
    legs["(b) this module, bf16 list, mixed_dtypes=True, fused"] = _leg(psgd, one, "fused", mixed_dtypes=True)
    for name, dtypes in (("D = 2", two), ("D = 3", three)):
        for tail in ("fused", "torch"):
            legs["(c) %s, %s" % (name, tail)] = _leg(psgd, dtypes, tail, mixed_dtypes=True)
    for fn in legs.values():
        fn()                                                    # tables and sub-plans are made here, not in a timed chunk
    times = {name: [] for name in legs}
    for _ in range(args.chunks):
        for name, fn in legs.items():
            times[name].append(_timed(fn, args.steps))
    print("class UVd whole step, N = %.1f M over %d tensors, r = 10, %d chunks of %d steps" % (N / 1e6, K, args.chunks, args.steps))
    base = statistics.median(times[next(iter(legs))])
    for name, ts in times.items():
        print("  %-54s %9.1f us  [%8.1f .. %8.1f]   x%.3f" % (name, statistics.median(ts), min(ts), max(ts), statistics.median(ts) / base))


if __name__ == "__main__":
    main()
