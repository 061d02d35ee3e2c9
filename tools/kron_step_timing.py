"""Time one optimizer step around the Kron preconditioner, three legs in one job:

    hand     the hand-written reference step (mnist_with_lenet5.py:43-57): per-layer calls in kron.layer_batch() blocks, torch ops around them
    torch    class Kron, step_tail="torch"
    fused    class Kron, step_tail="fused"

on the LeNet5 layer set and on one 1024 x 4096 layer, exact Hessian-vector products and clipping on, quadratic loss (the closure is
the same in all legs, so it cancels in a difference).  Protocol: every leg warms up for at least 0.5 s of device time, then the
legs ALTERNATE chunk by chunk; a chunk is `--steps` steps between two synchronises on the host clock; reported are the median and
the range of the per-chunk step times over `--chunks` (>= 7) chunks.  A difference smaller than the spread of the legs is not
resolved, and the summary line says so.

    python tools/kron_step_timing.py [--chunks 9] [--steps 50] [--out profiles/kron_class.txt]

--features times the switches of class Kron instead, same shapes and protocol, legs:

    off       class Kron, step_tail="fused", momentum / weight decay / guard at their defaults
    parent    the same, on the kron_optimizer.py of another commit given with --parent-module FILE (loaded beside this tree's; it
              runs on this tree's library), when given: the cost of the switches while they are off
    on-torch  momentum 0.9, weight decay 0.01, nonfinite="skip", loss_scale 2^8, step_tail="torch"
    on-fused  the same with step_tail="fused"

    python tools/kron_step_timing.py --features [--parent-module FILE] [--out profiles/kron_class_features.txt]

--dtype bf16 | fp16 times class Kron on parameters of that type (the closure widens them and computes in float32), legs:

    torch     step_tail="torch", everything off          fused     the same with step_tail="fused"
    on-torch  the switches of --features, torch tail      on-fused  the same with step_tail="fused"
    fp32      class Kron on float32 parameters, fused tail, everything off (with --parent-module also "parent": the same on the
              kron_optimizer.py of another commit): whether the float32 path moved

    python tools/kron_step_timing.py --dtype bf16 [--parent-module FILE] [--out profiles/kron_class_half.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from psgd_tf_amd import kron  # noqa: E402

SETS = {"lenet5": [(26, 6), (151, 16), (257, 120), (121, 84), (85, 10)], "1024x4096": [(1024, 4096)]}
LR, LR_Q = 0.01, 0.01


DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def problem(shapes, dev, dtype=torch.float32):
    g = torch.Generator(device=dev).manual_seed(0)
    Hl = [torch.diag(torch.exp(torch.empty(m, device=dev).uniform_(-1.0, 1.0, generator=g))) for m, n in shapes]
    Hr = [torch.diag(torch.exp(torch.empty(n, device=dev).uniform_(-1.0, 1.0, generator=g))) for m, n in shapes]
    Ws = [torch.randn(m, n, device=dev, generator=g).to(dtype).requires_grad_(True) for m, n in shapes]

    def closure():                                  # (.float() of a float32 tensor is the tensor itself)
        return sum(0.5 * torch.sum(W.float() * (hl @ W.float() @ hr)) for W, hl, hr in zip(Ws, Hl, Hr))
    return Ws, closure, 0.1 * sum(W.numel() for W in Ws) ** 0.5


def hand_leg(shapes, dev):
    Ws, closure, clip = problem(shapes, dev)
    Qs = [[torch.eye(m, device=dev), torch.eye(n, device=dev)] for m, n in shapes]
    tiny = torch.finfo(torch.float32).tiny

    def step():
        with torch.enable_grad():
            grads = torch.autograd.grad(closure(), Ws, create_graph=True)
            vs = [torch.randn_like(W) for W in Ws]
            Hvs = torch.autograd.grad(grads, Ws, vs)
        with torch.no_grad():
            with kron.layer_batch():
                new = [psgd.update_precond_kron(q[0], q[1], v, h, LR_Q) for q, v, h in zip(Qs, vs, Hvs)]
            Qs[:] = [[a, b] for a, b in new]
            with kron.layer_batch():
                pre = [psgd.precond_grad_kron(q[0], q[1], g.detach()) for q, g in zip(Qs, grads)]
            norm = torch.sqrt(sum(torch.sum(g * g) for g in pre)) + tiny
            lr = LR * torch.clamp(clip / norm, max=1.0)
            for W, g in zip(Ws, pre):
                W.sub_(lr * g)
    return step


FEATURES_ON = dict(momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale=2.0 ** 8)


def class_leg(tail, cls=None, dtype=torch.float32, **kw):
    def make(shapes, dev):
        Ws, closure, clip = problem(shapes, dev, dtype)
        opt = (cls or psgd.Kron)(Ws, "dense", lr_params=LR, lr_preconditioner=LR_Q, grad_clip_max_norm=clip, step_tail=tail, **kw)
        return lambda: opt.step(closure)
    return make


def parent_class(path):
    """class Kron of the kron_optimizer.py at `path`, loaded as a sibling module of this tree's package"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("psgd_tf_amd._parent_kron_optimizer", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.Kron


def timed(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--features", action="store_true")
    ap.add_argument("--parent-module", default=None)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default=None)
    a = ap.parse_args()
    if a.chunks < 7:
        ap.error("--chunks must be at least 7")
    dev = torch.device("cuda:0")
    lines = ["# tools/kron_step_timing.py %s--chunks %d --steps %d on %s"
             % ("--features " if a.features else "--dtype %s " % a.dtype if a.dtype else "", a.chunks, a.steps,
                torch.cuda.get_device_name(0)),
             "# us per step (closure + preconditioner + tail), median [min .. max] over the chunks; legs alternate chunk by chunk"]
    for name, shapes in SETS.items():
        if a.dtype:
            T = DTYPES[a.dtype]
            legs = {"torch": class_leg("torch", dtype=T)(shapes, dev), "fused": class_leg("fused", dtype=T)(shapes, dev),
                    "on-torch": class_leg("torch", dtype=T, **FEATURES_ON)(shapes, dev),
                    "on-fused": class_leg("fused", dtype=T, **FEATURES_ON)(shapes, dev), "fp32": class_leg("fused")(shapes, dev)}
            pairs = [("torch", "fused"), ("on-torch", "on-fused"), ("fused", "fp32")]
            if a.parent_module:
                legs["parent"] = class_leg("fused", parent_class(a.parent_module))(shapes, dev)
                pairs.append(("parent", "fp32"))
        elif a.features:
            legs = {"off": class_leg("fused")(shapes, dev)}
            if a.parent_module:
                legs["parent"] = class_leg("fused", parent_class(a.parent_module))(shapes, dev)
            legs["on-torch"] = class_leg("torch", **FEATURES_ON)(shapes, dev)
            legs["on-fused"] = class_leg("fused", **FEATURES_ON)(shapes, dev)
            pairs = ([("parent", "off")] if a.parent_module else []) + [("on-torch", "on-fused"), ("on-fused", "off")]
        else:
            legs = {"hand": hand_leg(shapes, dev), "torch": class_leg("torch")(shapes, dev), "fused": class_leg("fused")(shapes, dev)}
            pairs = [("hand", "torch"), ("hand", "fused"), ("torch", "fused")]
        for step in legs.values():                                  # warm-up: at least 0.5 s each, measured with the device drained
            spent = 0.0
            while spent < 0.5:
                spent += timed(step, 20) * 20e-6
        times = {k: [] for k in legs}
        for _ in range(a.chunks):
            for k, step in legs.items():
                times[k].append(timed(step, a.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, v in times.items():
            lines.append("%-10s %-8s %9.1f  [%9.1f .. %9.1f]" % (name, k, med[k], min(v), max(v)))
        spread = max(max(v) - min(v) for v in times.values())
        for x, y in pairs:
            d = med[x] - med[y]
            lines.append("%-10s %s - %s = %+8.1f us: %s (largest range of a leg: %.1f us)"
                         % (name, x, y, d, "resolved" if abs(d) > spread else "NOT resolved by this protocol", spread))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
