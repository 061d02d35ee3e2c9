"""One sha256 per configuration of class UVd, class Kron, class SPLU and class Dense after 6 steps: a refactor of the classes'
host layer must leave every digest that repeats from run to run as it was.

    python tools/class_step_digest.py [--out FILE]

Three parameters of shapes (5, 7), (4, 3) and (7,) -- Kron(any_rank=True), UVd and SPLU(rank_of_modification=3), Dense -- a
seeded CPU generator behind the coin and preconditioner_update_probability=0.5.  The configurations are the cross product of

    class      UVd, Kron, SPLU, Dense          tail     torch, fused             hvp     exact, fd (finite differences)
    dtype      float32, bfloat16 with param_rounding="nearest", bfloat16 with param_rounding="stochastic"
    features   off, or momentum 0.9 + weight decay + nonfinite="skip" + loss_scale="dynamic" with an Inf gradient in step 3

and preconditioner_fit="whitening" of the four classes on every tail, dtype and feature setting; then class UVd on the three
routes of its state that the grid does not reach (EXTRA_UVD: a placed state, a bfloat16 state read and written natively, a
bfloat16 state widened every step), each on the fused tail with the features on, exact and whitening; then the two switches the
grid predates, on the four classes, both tails, exact and fd, with the features on (SWITCHES: "groups" = float32 with two
param_groups, lr_scale 0.5 with weight decay 0 over tensors 0 and 2, lr_scale 2.0 over tensor 1; "mixed" = mixed_dtypes=True over
float32, bfloat16, float32).  The digest covers the
parameters, the preconditioner state (U, V, d, the factors or Q), the momentum buffers, skipped_steps, the current loss scale and
the counters of the rounding and probe streams.  Before anything runs on the device the coins of every configuration are replayed on the CPU
from the generator alone, and a configuration whose coins (the step with the Inf gradient left out) do not hold both outcomes is
an error; after the run the replay is compared with what the steps did (a step updated the preconditioner when its state
changed), and a line that disagrees says so.

Run it twice on the commit before the change and once after, and compare the lines: this tool takes no part in the test suite.
"""
import argparse
import hashlib
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402

SHAPES = [(5, 7), (4, 3), (7,)]
STEPS, INF_STEP, P_UPDATE, SEED = 6, 2, 0.5, 1
FEATURES_ON = dict(momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale="dynamic")
EXTRA_UVD = {"UVd:packed": dict(placement="packed"), "UVd:bf16native": dict(state_dtype=torch.bfloat16, state_route="native"),
             "UVd:bf16widen": dict(state_dtype=torch.bfloat16)}
DTYPES = {"fp32": (torch.float32, "nearest"), "bf16": (torch.bfloat16, "nearest"), "bf16sr": (torch.bfloat16, "stochastic")}
SWITCHES = {"groups": [torch.float32] * 3, "mixed": [torch.float32, torch.bfloat16, torch.float32]}    # in the place of a dtype


def dtypes_of(dt):
    """(the dtype of each of the three parameters, param_rounding) of a line's dtype field"""
    if dt in SWITCHES:
        return SWITCHES[dt], "nearest"
    return [DTYPES[dt][0]] * len(SHAPES), DTYPES[dt][1]


def configurations():
    for cls, tail, hvp, dt, feat in itertools.product(("UVd", "Kron"), ("torch", "fused"), ("exact", "fd"), DTYPES, ("off", "on")):
        yield cls, tail, hvp, dt, feat
    for cls, tail, dt, feat in itertools.product(("Kron", "UVd"), ("torch", "fused"), DTYPES, ("off", "on")):
        yield cls, tail, "whitening", dt, feat
    for tail, hvp, dt, feat in itertools.product(("torch", "fused"), ("exact", "fd", "whitening"), DTYPES, ("off", "on")):
        yield "SPLU", tail, hvp, dt, feat
    for cls, hvp in itertools.product(EXTRA_UVD, ("exact", "whitening")):
        yield cls, "fused", hvp, "fp32", "on"
    for tail, hvp, dt, feat in itertools.product(("torch", "fused"), ("exact", "fd", "whitening"), DTYPES, ("off", "on")):
        yield "Dense", tail, hvp, dt, feat            # (the lines before it keep their places)
    for cls, tail, hvp, dt in itertools.product(("UVd", "Kron", "SPLU", "Dense"), ("torch", "fused"), ("exact", "fd"), SWITCHES):
        yield cls, tail, hvp, dt, "on"                # (last: a new line is added here, at the end)


def replayed_coins(cls, hvp, dt, feat):
    """the coins of the six steps, from the CPU generator alone: the draws of the constructor (the seed of a native bfloat16
    state, the seed of the parameters' rounding stream, then the probe seed), then per step the coin and what the class draws
    after it from the same generator -- class UVd the two branches of an update that runs, class Kron its probe vectors in the
    parameters' dtype, class SPLU and class Dense nothing"""
    gen = torch.Generator().manual_seed(SEED)
    dtypes, rounding = dtypes_of(dt)
    for _ in range((cls == "UVd:bf16native") + (rounding == "stochastic") + (hvp == "whitening")):
        torch.randint(0, 2 ** 62, (), generator=gen)
    coins = []
    for k in range(STEPS):
        update = bool(torch.rand((), generator=gen).item() < P_UPDATE)
        coins.append(update)
        if not update:
            continue
        if cls.startswith("UVd") and not (feat == "on" and k == INF_STEP):
            torch.rand((), generator=gen), torch.rand((), generator=gen)
        if cls == "Kron" and hvp != "whitening":
            for s, dtype in zip(SHAPES, dtypes):
                torch.randn(s, dtype=dtype, generator=gen)
    return coins


def raw(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


def state_tensors(opt):
    if isinstance(opt, psgd.Kron):
        return [q for pair in opt.factors for q in pair]
    if isinstance(opt, psgd.SPLU):
        return list(opt.factors)
    if isinstance(opt, psgd.Dense):
        return [opt.Q]
    return [opt._U, opt._V, opt._d]


def run(cls, tail, hvp, dt, feat, dev):
    dtypes, rounding = dtypes_of(dt)
    torch.manual_seed(1234)                       # the global device generator: UVd's initial U, V and its probe vectors
    init = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=init).to(dev, dtype).requires_grad_(True) for s, dtype in zip(SHAPES, dtypes)]
    hess = [torch.rand(s, generator=init).add_(0.5).to(dev) for s in SHAPES]
    step_no = [0]

    def closure():
        loss = sum(0.5 * torch.sum(h * p.float() * p.float()) for p, h in zip(params, hess)) + 0.1 * params[0].float().sum() ** 2
        if feat == "on" and step_no[0] == INF_STEP:
            loss = loss + params[1].float().sum() * float("inf")
        return loss
    kw = dict(lr_params=0.05, lr_preconditioner=0.1, grad_clip_max_norm=1.0, preconditioner_update_probability=P_UPDATE,
              exact_hessian_vector_product=hvp != "fd", step_tail=tail, generator=torch.Generator().manual_seed(SEED),
              param_rounding=rounding, **(FEATURES_ON if feat == "on" else {}))
    if dt == "groups":
        kw["param_groups"] = [dict(params=[params[0], params[2]], lr_scale=0.5, weight_decay=0.0), dict(params=[params[1]], lr_scale=2.0)]
    if dt == "mixed":
        kw["mixed_dtypes"] = True
    if cls.startswith("UVd"):                     # (its Hessian-fit lines are built without the keyword, as before it existed)
        kw.update(EXTRA_UVD.get(cls, {}), **({"preconditioner_fit": "whitening"} if hvp == "whitening" else {}))
        opt = psgd.UVd(params, rank_of_modification=3, **kw)
    elif cls == "SPLU":
        opt = psgd.SPLU(params, rank_of_modification=3, preconditioner_fit="whitening" if hvp == "whitening" else "hessian", **kw)
    elif cls == "Dense":
        opt = psgd.Dense(params, preconditioner_fit="whitening" if hvp == "whitening" else "hessian", **kw)
    else:
        opt = psgd.Kron(params, any_rank=True, preconditioner_fit="whitening" if hvp == "whitening" else "hessian", **kw)
    coins = ""
    for k in range(STEPS):
        step_no[0] = k
        before = [raw(t) for t in state_tensors(opt)]
        opt.step(closure)
        coins += "s" if opt.last_step_skipped else "01"[before != [raw(t) for t in state_tensors(opt)]]
    h = hashlib.sha256()
    # (a placed UVd keeps its momentum in the arena's g region and leaves _m at None: _momentum_buffer() is where it lives)
    moms = opt._m if isinstance(opt._m, list) else [opt._momentum_buffer()] if cls == "UVd:packed" else [] if opt._m is None else [opt._m]
    for t in params + state_tensors(opt) + moms:
        h.update(raw(t))
    # (a Hessian-fit UVd hashes None for the probe counter, as it did when the class had none: its lines stay comparable)
    probe_step = None if cls.startswith("UVd") and hvp != "whitening" else opt.probe_step
    h.update(repr((opt.skipped_steps, opt.loss_scale.value, opt._param_round_step, probe_step)).encode())
    return h.hexdigest(), coins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    replay = {}
    for c in configurations():
        coins = replay[c] = replayed_coins(c[0], c[2], c[3], c[4])
        if len({u for k, u in enumerate(coins) if k != INF_STEP}) != 2:           # (the step that may be skipped does not count)
            raise SystemExit("%s: the coins %r hold one outcome only; choose another SEED" % ("-".join(c), coins))
    dev = torch.device("cuda:0")
    lines = []
    for c in configurations():
        digest, coins = run(*c, dev)
        want = "".join("s" if c[4] == "on" and k == INF_STEP else "01"[u] for k, u in enumerate(replay[c]))
        lines.append("%-32s %s coins %s%s" % ("-".join(c), digest, coins, "" if coins == want else " (replayed: %s)" % want))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
