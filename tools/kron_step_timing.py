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

With --parent-module FILE (the kron_optimizer.py of another commit, loaded beside this tree's; it runs on this tree's library and
on this tree's _StepFeatures) the hand leg gives way to that commit's class on each tail, TWICE ("parent-torch", "parent-torch-2",
...): whether the host layer of a step moved.  The bar is the parent in the same job, the margin the difference between the
medians of its own two legs.

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

--operands measures Kron(operands="bfloat16"), two tables:

    threshold   per layer shape (square and 1:4, short side 256 .. 2048), DEVICE time (events around a chunk of 20 rounds) of
                "bf16": one multi_narrow of dX and dG + the bf16-operand update + one multi_narrow of g + the bf16-operand apply,
                against "fp32": the fp32 update + apply; new factors every round, as on a step that updates them
    step        whole steps, fused tail, exact products, the switches off, an elementwise quadratic loss (so that the
                preconditioner dominates), float32 and bfloat16 parameters, legs "none" (operands=None), "bf16"
                (operands="bfloat16", operand_min_dim=1024) and, with --parent-module, "parent" (as "none", on the
                kron_optimizer.py of another commit)

    python tools/kron_step_timing.py --operands [--parent-module FILE] [--out profiles/kron_class_operands.txt]

--whitening compares the three fits of class Kron, fused tail, clipping on, everything else off, on the LeNet5 set, on one
1024 x 4096 layer and on 200 vectors of length 1024 + one 1024 x 4096 layer with any_rank=True, two tables:

    step     whole steps on the host clock, legs "exact" (exact_hessian_vector_product=True), "fd" (finite differences),
             "whitening" (preconditioner_fit="whitening") and, with --parent-module, "parent" (as "exact", on the
             kron_optimizer.py of another commit): whether the default path moved
    probe    DEVICE time (events around a chunk of 20 rounds) of ONE multi_randn launch against the k torch.randn launches it
             replaces, on the probe buffers of the same three parameter sets

    python tools/kron_step_timing.py --whitening [--parent-module FILE] [--out profiles/kron_whitening.txt]
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


OPERAND_SHORT_SIDES = (256, 512, 768, 1024, 2048)
OPERAND_SETS = {"4096x4096": [(4096, 4096)], "1024x4096": [(1024, 4096)],
                "8x(1024x4096)+8x(1024x1024)": [(1024, 4096)] * 8 + [(1024, 1024)] * 8}


def device_timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def alternate(legs, chunks, n, timer, warm):
    """warm every leg up for `warm` seconds, then `chunks` rounds over the legs of n calls each: {leg: [us per call]}"""
    for fn in legs.values():
        spent = 0.0
        while spent < warm:
            spent += timed(fn, 10) * 10e-6
    times = {k: [] for k in legs}
    for _ in range(chunks):
        for k, fn in legs.items():
            times[k].append(timer(fn, n))
    return times


def threshold_legs(M, N, dev):
    g = torch.Generator(device=dev).manual_seed(7 * M + N)
    dX, G = torch.randn(M, N, device=dev, generator=g), torch.randn(M, N, device=dev, generator=g)
    dG = dX * torch.exp(torch.empty(M, N, device=dev).uniform_(-1.0, 1.0, generator=g))
    Q = {k: [torch.eye(M, device=dev), torch.eye(N, device=dev)] for k in ("fp32", "bf16")}
    bg, bx, bh = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(3))

    def fp32():
        q = Q["fp32"]
        q[:] = psgd.update_precond_kron(q[0], q[1], dX, dG, LR_Q)
        psgd.precond_grad_kron(q[0], q[1], G)

    def bf16():
        q = Q["bf16"]
        psgd.multi_narrow([[dX], [dG]], [[bx], [bh]])
        q[:] = psgd.update_precond_kron(q[0], q[1], bx, bh, LR_Q)
        psgd.multi_narrow([[G]], [[bg]])
        psgd.precond_grad_kron(q[0], q[1], bg)
    return {"fp32": fp32, "bf16": bf16}


def operand_leg(shapes, dev, dtype, cls=None, **kw):
    g = torch.Generator(device=dev).manual_seed(0)
    H = [torch.exp(torch.empty(m, n, device=dev).uniform_(-1.0, 1.0, generator=g)) for m, n in shapes]
    Ws = [torch.randn(m, n, device=dev, generator=g).to(dtype).requires_grad_(True) for m, n in shapes]
    closure = lambda: sum(0.5 * torch.sum(h * W.float() * W.float()) for W, h in zip(Ws, H))
    clip = 0.1 * sum(W.numel() for W in Ws) ** 0.5
    opt = (cls or psgd.Kron)(Ws, "dense", lr_params=LR, lr_preconditioner=LR_Q, grad_clip_max_norm=clip, step_tail="fused", **kw)
    return lambda: opt.step(closure)


def report(lines, name, times, pairs):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append("%-28s %-7s %9.1f  [%9.1f .. %9.1f]" % (name, k, med[k], min(v), max(v)))
    spread = max(max(v) - min(v) for v in times.values())
    for x, y in pairs:
        d = med[x] - med[y]
        lines.append("%-28s %s - %s = %+8.1f us: %s (largest range of a leg: %.1f us)"
                     % (name, x, y, d, "resolved" if abs(d) > spread else "NOT resolved by this protocol", spread))
    print("\n".join(lines[-len(times) - len(pairs):]), flush=True)
    return med, spread


def operands_main(a, dev):
    lines = ["# tools/kron_step_timing.py --operands --chunks %d --steps %d on %s" % (a.chunks, a.steps, torch.cuda.get_device_name(0)),
             "# threshold: us of DEVICE time per round (narrow + update + narrow + apply on bf16 operands against the fp32 update + "
             "apply), median [min .. max] over the chunks of 20 rounds; legs alternate chunk by chunk"]
    wins = {}
    for short in OPERAND_SHORT_SIDES:
        for M, N in ((short, short), (short, 4 * short)):
            med, spread = report(lines, "threshold %dx%d" % (M, N), alternate(threshold_legs(M, N, dev), a.chunks, 20, device_timed, 0.2),
                                 [("fp32", "bf16")])
            wins.setdefault(short, []).append(med["fp32"] - med["bf16"] > spread)
            torch.cuda.empty_cache()
    ok = [s for s in OPERAND_SHORT_SIDES if all(all(wins[t]) for t in OPERAND_SHORT_SIDES if t >= s)]
    lines.append("# smallest short side from which the bf16 route wins by more than the spread on both shapes, and on every larger "
                 "side measured: %s" % (min(ok) if ok else "none"))
    lines.append("# step: us per step on the host clock (closure + preconditioner + tail), fused tail, exact products, median "
                 "[min .. max] over the chunks of %d steps; legs alternate chunk by chunk" % a.steps)
    parent = parent_class(a.parent_module) if a.parent_module else None
    for name, shapes in OPERAND_SETS.items():
        for tag, T in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            legs = {"none": operand_leg(shapes, dev, T), "bf16": operand_leg(shapes, dev, T, operands="bfloat16", operand_min_dim=1024)}
            pairs = [("none", "bf16")]
            if parent is not None:
                legs["parent"] = operand_leg(shapes, dev, T, parent)
                pairs.append(("parent", "none"))
            report(lines, "step %s %s" % (name, tag), alternate(legs, a.chunks, a.steps, timed, 0.5), pairs)
            del legs
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


WHITENING_SETS = {"lenet5": (SETS["lenet5"], False), "1024x4096": (SETS["1024x4096"], False),
                  "200x(1024,)+1024x4096": ([(1024,)] * 200 + [(1024, 4096)], True)}


def whitening_leg(shapes, any_rank, dev, cls=None, **kw):
    """an elementwise quadratic loss (any rank; its backward is cheap, so the legs differ by the passes they run, not by the model)"""
    g = torch.Generator(device=dev).manual_seed(0)
    H = [torch.exp(torch.empty(s, device=dev).uniform_(-1.0, 1.0, generator=g)) for s in shapes]
    Ws = [torch.randn(s, device=dev, generator=g).requires_grad_(True) for s in shapes]
    closure = lambda: sum(0.5 * torch.sum(h * W * W) for W, h in zip(Ws, H))
    clip = 0.1 * sum(W.numel() for W in Ws) ** 0.5
    if any_rank:
        kw = dict(kw, any_rank=True)
    opt = (cls or psgd.Kron)(Ws, "dense", lr_params=LR, lr_preconditioner=LR_Q, grad_clip_max_norm=clip, step_tail="fused", **kw)
    return lambda: opt.step(closure)


def whitening_main(a, dev):
    lines = ["# tools/kron_step_timing.py --whitening --chunks %d --steps %d on %s" % (a.chunks, a.steps, torch.cuda.get_device_name(0)),
             "# step: us per step on the host clock (closure + preconditioner + tail), fused tail, clipping on, median [min .. max] "
             "over the chunks of %d steps; legs alternate chunk by chunk" % a.steps]
    parent = parent_class(a.parent_module) if a.parent_module else None
    for name, (shapes, any_rank) in WHITENING_SETS.items():
        legs = {"exact": whitening_leg(shapes, any_rank, dev, exact_hessian_vector_product=True),
                "fd": whitening_leg(shapes, any_rank, dev, exact_hessian_vector_product=False),
                "whitening": whitening_leg(shapes, any_rank, dev, preconditioner_fit="whitening")}
        pairs = [("exact", "whitening"), ("fd", "whitening")]
        if parent is not None:
            legs["parent"] = whitening_leg(shapes, any_rank, dev, parent, exact_hessian_vector_product=True)
            pairs.append(("parent", "exact"))
        report(lines, "step %s" % name, alternate(legs, a.chunks, a.steps, timed, 0.5), pairs)
        del legs
        torch.cuda.empty_cache()
    lines.append("# probe: us of DEVICE time per round, ONE multi_randn launch over k float32 buffers against k torch.randn launches "
                 "(out=) into the same buffers; median [min .. max] over the chunks of 20 rounds; legs alternate chunk by chunk")
    for name, (shapes, _) in WHITENING_SETS.items():
        bufs = [torch.empty(s, device=dev) for s in shapes]
        legs = {"randn-k": lambda bufs=bufs: [torch.randn(b.shape, device=dev, out=b) for b in bufs],
                "multi-1": lambda bufs=bufs: psgd.multi_randn(bufs, 12345)}
        report(lines, "probe %s (k = %d)" % (name, len(bufs)), alternate(legs, a.chunks, 20, device_timed, 0.2), [("randn-k", "multi-1")])
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--whitening", action="store_true")
    ap.add_argument("--operands", action="store_true")
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
    if a.operands:
        return operands_main(a, dev)
    if a.whitening:
        return whitening_main(a, dev)
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
        elif a.parent_module:
            parent = parent_class(a.parent_module)
            legs, pairs = {}, []
            for tail in ("torch", "fused"):
                legs.update({tail: class_leg(tail)(shapes, dev), "parent-" + tail: class_leg(tail, parent)(shapes, dev),
                             "parent-%s-2" % tail: class_leg(tail, parent)(shapes, dev)})
                pairs += [(tail, "parent-" + tail), ("parent-%s-2" % tail, "parent-" + tail)]
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
            lines.append("%-10s %-14s %9.1f  [%9.1f .. %9.1f]" % (name, k, med[k], min(v), max(v)))
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
