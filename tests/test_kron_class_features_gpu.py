"""Momentum, weight decay, the non-finite guard and the loss scale of class Kron on the GPU: fused tail against torch tail bit for
bit, the defaults as the old code path, the launch budget of the fused tail, skipped steps, loss scaling, parity with an fp64
restatement, and resume.  Shapes: the LeNet5 layers plus the six sparse pairs of tests/kron_class_cases.py; runs of 3-6 steps.
The Inf and NaN gradients here are data that the guard must catch, injected through a multiplier in the loss."""
import collections

import numpy as np
import pytest
import torch

from tests import kron_class_cases as kc
from tests import test_kron_class_gpu as kg

pytestmark = pytest.mark.gpu

SHAPES, FORMATS, LR, LR_Q, MAX_NORM = kg.SHAPES, kg.FORMATS, kg.LR, kg.LR_Q, kg.MAX_NORM
_dev, _gen, _bits_equal = kg._dev, kg._gen, kg._bits_equal
NEW = ("psgd_multi_blend_f32", "psgd_multi_scale_check_f32", "psgd_multi_param_update_wd_f32")
LAUNCHES = collections.defaultdict(lambda: 1, psgd_multi_sumsq_f32=2)          # launches of one call of a list-kernel entry point


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _make(psgd, tail, exact, *, clip=False, seed=11, shapes=SHAPES, formats=FORMATS, prob=1.0, lr=LR, **kw):
    """(params, optimizer, closure, mult): the quadratic of the class tests times mult, a device scalar that is 1 unless a test
    sets it to Inf or NaN for one step (a product with 1 changes no bit)"""
    Ws, _, _, Hl, Hr = kg._problem(shapes)
    params = kg._fresh_params(Ws)
    opt = psgd.Kron(params, formats, 1.0, lr, LR_Q, MAX_NORM if clip else None, prob, exact, step_tail=tail, generator=_gen(seed),
                    **kw)
    mult = torch.ones((), device=_dev())
    base = kg._quadratic_closure(params, Hl, Hr)
    return params, opt, (lambda: base() * mult), mult


def _state(params, opt):
    return dict(params=[p.detach().clone() for p in params], factors=[[q[0].clone(), q[1].clone()] for q in opt.factors],
                momentum=None if opt._m is None else [m.clone() for m in opt._m], momentum_step=opt._m_step)


def _assert_state(a, b, what):
    for i, (x, y) in enumerate(zip(a["params"], b["params"])):
        assert _bits_equal(x, y), "%s: parameter %d differs" % (what, i)
    for i, (x, y) in enumerate(zip(a["factors"], b["factors"])):
        assert _bits_equal(x[0], y[0]) and _bits_equal(x[1], y[1]), "%s: factors of layer %d differ" % (what, i)
    assert (a["momentum"] is None) == (b["momentum"] is None), what
    for i, (x, y) in enumerate(zip(a["momentum"] or (), b["momentum"] or ())):
        assert _bits_equal(x, y), "%s: momentum buffer %d differs" % (what, i)
    assert a["momentum_step"] == b["momentum_step"], what


def _run(psgd, tail, exact, steps, **kw):
    params, opt, closure, _ = _make(psgd, tail, exact, **kw)
    for _ in range(steps):
        opt.step(closure)
    return _state(params, opt), opt


class _Counting:
    """the loaded library with every entry-point call counted by name"""

    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("psgd_"):
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def counting(monkeypatch):
    from psgd_tf_amd import _lib
    proxy = _Counting(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    return proxy


# ---------------------------------------------------------------------------------------------------- fused against torch
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_fused_tail_equals_torch_tail_without_clipping(psgd, momentum, weight_decay, exact):
    a, _ = _run(psgd, "torch", exact, 4, momentum=momentum, weight_decay=weight_decay)
    b, _ = _run(psgd, "fused", exact, 4, momentum=momentum, weight_decay=weight_decay)
    _assert_state(b, a, "fused against torch, momentum %r, weight decay %r" % (momentum, weight_decay))
    assert (a["momentum"] is not None) == (momentum > 0.0)
    assert all(bool(torch.isfinite(p).all()) for p in a["params"])
    plain, _ = _run(psgd, "torch", exact, 4)
    if momentum or weight_decay:
        assert not _bits_equal(a["params"][0], plain["params"][0])                   # the switches did something
    else:
        _assert_state(a, plain, "zeros are the defaults")


def _dyadic_run(psgd, tail, steps=3):
    """a closure whose gradient is a fixed dyadic tensor, no factor update, identity factors, momentum 0.5 (beta_k = 0, 1/2, 1/2):
    the preconditioned gradient is dyadic and S is exact in any order, so both tails form the same lr_eff"""
    gen = torch.Generator().manual_seed(3)
    Ds = [(torch.randint(-64, 65, s, generator=gen).float() / 16.0).to(_dev()) for s in SHAPES]
    Ws, _, _, _, _ = kg._problem(SHAPES)
    params = kg._fresh_params(Ws)
    opt = psgd.Kron(params, FORMATS, 1.0, LR, LR_Q, MAX_NORM, 0.0, True, step_tail=tail, generator=_gen(5), momentum=0.5,
                    weight_decay=0.01)
    closure = lambda: sum(torch.sum(p * d) for p, d in zip(params, Ds))
    for _ in range(steps):
        opt.step(closure)
    return _state(params, opt)


def test_fused_tail_equals_torch_tail_with_clipping_on_dyadic_gradients(psgd):
    a, b = _dyadic_run(psgd, "torch"), _dyadic_run(psgd, "fused")
    _assert_state(b, a, "clipped step with momentum and weight decay on dyadic gradients")
    Ws, _, _, _, _ = kg._problem(SHAPES)
    assert not _bits_equal(a["params"][0], kg._fresh_params(Ws)[0].detach())


# -------------------------------------------------------------------------------------------------- the defaults: old path
@pytest.mark.parametrize("exact", [True, False])
def test_defaults_are_the_old_path(psgd, exact, counting, monkeypatch):
    """the new arguments at their defaults: the bits of an optimizer built without them and of the hand-written step, none of the
    three new entry points, no flag read, and no .item() but the coin's (a device generator draws the coin with one)"""
    items = []
    real_item = torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "item", lambda self: items.append(1) or real_item(self))
    a, oa = _run(psgd, "fused", exact, 3, clip=True, momentum=0.0, weight_decay=0.0, nonfinite="propagate", loss_scale=None,
                 loss_scale_growth_interval=2000)
    n_items = len(items)
    b, _ = _run(psgd, "fused", exact, 3, clip=True)
    _assert_state(a, b, "defaults spelled out against defaults")
    assert n_items == 3 and len(items) == 6                                          # one coin per step, nothing else
    assert not any(counting.calls[n] for n in NEW), dict(counting.calls)
    assert counting.calls["psgd_multi_param_update_f32"] == 2 * 3 * (1 if exact else 2)
    assert oa._tail.stamp == 0 and int(real_item(oa._tail.flag)) == 0 and oa._m is None
    assert oa.skipped_steps == 0 and oa.last_step_skipped is False
    t, _ = _run(psgd, "torch", exact, 3, momentum=0.0, weight_decay=0.0, nonfinite="propagate")
    ref_params, ref_Q = kg._run_reference(psgd, exact, False, True)
    for x, y in zip(t["params"], ref_params):
        assert _bits_equal(x, y.detach())
    for x, y in zip(t["factors"], ref_Q):
        assert _bits_equal(x[0], y[0]) and _bits_equal(x[1], y[1])


# ------------------------------------------------------------------------------------------------------------ launch count
def test_launch_budget_of_the_fused_tail_with_everything_on(psgd, counting):
    """finite differences, guard, loss scale, momentum, clipping and weight decay together: perturb 1, scale-check 1, diff-scale 1,
    blend 1, sum of squares 2, update 1 = 7 launches, whatever the number of layers"""
    params, opt, closure, _ = _make(psgd, "fused", False, clip=True, momentum=0.9, weight_decay=0.01, nonfinite="skip",
                                    loss_scale=2.0 ** 8)
    per_step = []
    for _ in range(3):
        before = collections.Counter(counting.calls)
        opt.step(closure)
        now = collections.Counter(counting.calls)
        now.subtract(before)
        per_step.append({k: v for k, v in now.items() if k.startswith("psgd_multi_") and v})
    want = {"psgd_multi_param_update_f32": 1, "psgd_multi_scale_check_f32": 1, "psgd_multi_diff_scale_f32": 1,
            "psgd_multi_blend_f32": 1, "psgd_multi_sumsq_f32": 1, "psgd_multi_param_update_wd_f32": 1}
    for calls in per_step:
        assert calls == want, calls
        assert sum(LAUNCHES[k] * v for k, v in calls.items()) == 7
    assert opt.skipped_steps == 0


# -------------------------------------------------------------------------------------------------------------------- skip
def _consume_step_draws(G, params, exact):
    """what a skipped step takes from the generator: the coin, then one randn per parameter (times delta on the
    finite-difference route).  Returns the probe vectors."""
    torch.rand((), generator=G, device=_dev())
    vs = [torch.randn(p.shape, device=_dev(), generator=G) for p in params]
    return vs if exact else [v * kc.DELTA32 for v in vs]


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("exact", [True, False])
def test_a_non_finite_gradient_skips_the_step(psgd, exact, tail, momentum, value):
    kw = dict(momentum=momentum, weight_decay=0.01, nonfinite="skip")
    params, opt, closure, mult = _make(psgd, tail, exact, **kw)
    for _ in range(2):
        opt.step(closure)
    assert opt.skipped_steps == 0 and not opt.last_step_skipped
    before = _state(params, opt)
    twin_G = torch.Generator(device=_dev())
    twin_G.set_state(opt._generator.get_state())
    mult.fill_(value)
    out = opt.step(closure)                                                          # step 3: every gradient is Inf or NaN
    mult.fill_(1.0)
    assert not bool(torch.isfinite(out))                                             # the closure's value is passed through
    assert opt.skipped_steps == 1 and opt.last_step_skipped
    after = _state(params, opt)
    vs = _consume_step_draws(twin_G, params, exact)
    want = dict(before)
    if not exact:                                                                    # the reference's own undo: p + v - v
        want["params"] = [(p + v) - v for p, v in zip(before["params"], vs)]
    _assert_state(after, want, "a skipped step")
    assert _bits_equal(torch.rand(3, generator=twin_G, device=_dev()),               # the coin and the probes, nothing else
                       torch.rand(3, generator=_clone_gen(opt._generator), device=_dev()))
    opt.step(closure)                                                                # step 4 proceeds
    assert opt.skipped_steps == 1 and not opt.last_step_skipped
    # the twin never sees step 3's data: two steps, the draws of a step by hand, the undo by hand, one more step
    t_params, t_opt, t_closure, _ = _make(psgd, tail, exact, **kw)
    for _ in range(2):
        t_opt.step(t_closure)
    t_vs = _consume_step_draws(t_opt._generator, t_params, exact)
    if not exact:
        with torch.no_grad():
            for p, v in zip(t_params, t_vs):
                p.copy_((p + v) - v)
    t_opt.step(t_closure)
    _assert_state(_state(params, opt), _state(t_params, t_opt), "the step after a skipped one")
    assert not _bits_equal(after["params"][0], params[0].detach())


def _clone_gen(G):
    twin = torch.Generator(device=G.device)
    twin.set_state(G.get_state())
    return twin


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_a_step_that_leaves_the_factors_alone_is_guarded_too(psgd, tail):
    params, opt, closure, mult = _make(psgd, tail, True, prob=0.0, momentum=0.9, nonfinite="skip")
    opt.step(closure)
    before = _state(params, opt)
    mult.fill_(float("nan"))
    opt.step(closure)
    mult.fill_(1.0)
    _assert_state(_state(params, opt), before, "a skipped step without a factor update")
    assert opt.skipped_steps == 1
    opt.step(closure)
    assert opt.skipped_steps == 1 and not _bits_equal(before["params"][0], params[0].detach())


# -------------------------------------------------------------------------------------------------------------- loss scale
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("exact", [True, False])
def test_a_power_of_two_loss_scale_changes_no_bit(psgd, exact, tail):
    """gradients of order 1: times 2^8 or 2^16 they stay finite and normal, so scaling by S and by 1 / S is exact"""
    kw = dict(momentum=0.9, weight_decay=0.01, nonfinite="skip")
    ref, _ = _run(psgd, tail, exact, 3, **kw)
    for S in (2.0 ** 8, 2.0 ** 16):
        got, opt = _run(psgd, tail, exact, 3, loss_scale=S, **kw)
        _assert_state(got, ref, "loss_scale=%r against None" % S)
        assert float(opt.loss_scale) == S and opt.skipped_steps == 0


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_the_dynamic_loss_scale_halves_and_doubles(psgd, tail):
    params, opt, closure, mult = _make(psgd, tail, True, nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=2)
    assert float(opt.loss_scale) == 2.0 ** 16
    opt.step(closure)
    assert float(opt.loss_scale) == 2.0 ** 16
    mult.fill_(float("inf"))
    opt.step(closure)
    mult.fill_(1.0)
    assert float(opt.loss_scale) == 2.0 ** 15 and opt.skipped_steps == 1
    opt.step(closure)
    assert float(opt.loss_scale) == 2.0 ** 15
    opt.step(closure)
    assert float(opt.loss_scale) == 2.0 ** 16 and opt.skipped_steps == 1
    assert all(bool(torch.isfinite(p).all()) for p in params)


# ------------------------------------------------------------------------------------------------------------ fp64 parity
PARITY_SHAPES, PARITY_MAX_NORM = kg.PARITY_SHAPES, kg.PARITY_MAX_NORM
PARITY_MOMENTUM = 0.9
# lr_eff is about 0.02 and |p| about 0.5 (see PARITY_MAX_NORM in tests/test_kron_class_gpu.py): the decay term lr_eff wd |p| is
# about 1e-3 against increments of about 1e-2, far above the 1e-3 of the increment that makes it visible to a 1e-5 bar
PARITY_WEIGHT_DECAY = 0.1


def _step_f64(W, Q, M, k, grad_fn, hvp_fn, vs, *, momentum, weight_decay, lr_params, lr_preconditioner, max_norm):
    """kron_step_f64 with momentum and decoupled weight decay: the blended buffer takes the gradient's place in the preconditioned
    gradient (grad_fn is asked once on the exact route), and the update subtracts lr_eff wd W as well"""
    beta = min(k / (k + 1.0), momentum)
    M = [beta * m + (1.0 - beta) * g for m, g in zip(M, grad_fn(W))]
    new, Q, pre, lr_eff = kc.kron_step_f64(W, Q, lambda _: M, hvp_fn, vs, lr_params=lr_params,
                                           lr_preconditioner=lr_preconditioner, max_norm=max_norm)
    decay = [lr_eff * weight_decay * w for w in W]
    return [n - d for n, d in zip(new, decay)], Q, M, pre, lr_eff, decay


@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("clip", [False, True])
def test_parity_with_the_fp64_restatement(psgd, clip, tail, monkeypatch):
    """exact Hessian-vector products and the same probe vectors: factors, preconditioned gradients and parameter increments within
    the bars of tests/test_kron_class_gpu.py (1e-5, relative and norm-wise, the increments on their own norm) after steps 1 and 5"""
    from psgd_tf_amd import kron_optimizer as ko
    Ws, Hls, Hrs, Hl, Hr = kg._problem(PARITY_SHAPES, seed=1)
    params = kg._fresh_params(Ws)
    G = _gen(31)
    twin = _clone_gen(G)
    opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, PARITY_MAX_NORM if clip else None, step_tail=tail, generator=G,
                    momentum=PARITY_MOMENTUM, weight_decay=PARITY_WEIGHT_DECAY)
    closure = kg._quadratic_closure(params, Hl, Hr)
    seen = []
    real = ko._psgd.precond_grad_kron
    monkeypatch.setattr(ko._psgd, "precond_grad_kron", lambda *a: seen.append(real(*a)) or seen[-1])
    W64 = [w.copy() for w in Ws]
    Q64 = [kc.initial_factors(s, ("dense", "dense")) for s in PARITY_SHAPES]
    M64 = [np.zeros(s) for s in PARITY_SHAPES]
    grad_fn = lambda W: kc.quadratic_grads(W, Hls, Hrs)
    hvp_fn = lambda vs: kc.quadratic_grads(vs, Hls, Hrs)
    n64 = lambda t: t.detach().double().cpu().numpy()
    f32 = lambda x: float(np.float32(x))
    for step in range(1, 6):
        del seen[:]
        opt.step(closure)
        torch.rand((), generator=twin, device=_dev())                                  # the coin
        vs = [n64(torch.randn(s, device=_dev(), generator=twin)) for s in PARITY_SHAPES]
        W_old = W64
        W64, Q64, M64, pre64, lr_eff, decay = _step_f64(
            W64, Q64, M64, step - 1, grad_fn, hvp_fn, vs, momentum=f32(PARITY_MOMENTUM), weight_decay=f32(PARITY_WEIGHT_DECAY),
            lr_params=f32(LR), lr_preconditioner=f32(LR_Q), max_norm=f32(PARITY_MAX_NORM) if clip else None)
        share = min(np.linalg.norm(d) / np.linalg.norm(w - w0) for d, w, w0 in zip(decay, W64, W_old))
        assert share >= 1e-3, "the decay term is %.1e of the step's increment: too small to be seen" % share
        if step in (1, 5):
            errs = {"factors": max(kc.rel(n64(q), r) for pair, ref in zip(opt.factors, Q64) for q, r in zip(pair, ref)),
                    "pre_grads": max(kc.rel(n64(g), r) for g, r in zip(seen, pre64)),
                    "momentum": max(kc.rel(n64(m), r) for m, r in zip(opt._m, M64)),
                    "increments": max(kc.rel(n64(p) - w0, w - w0) for p, w, w0 in zip(params, W64, Ws))}
            print("step %d, clip %s, decay share %.1e: %s" % (step, clip, share, {k: "%.2e" % v for k, v in errs.items()}))
            assert max(errs.values()) < 1e-5, (step, errs)


# ----------------------------------------------------------------------------------------------------------------- resume
@pytest.mark.parametrize("tail, exact", [("torch", True), ("fused", False), ("fused", True)])
def test_resume_with_momentum_and_the_dynamic_scale_is_bit_identical(psgd, tail, exact):
    """save after step 3 (step 2 was skipped), load into a fresh optimizer, compare through step 6"""
    kw = dict(clip=False, momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=2)

    def run(opt, closure, mult, first, last):
        for k in range(first, last + 1):
            mult.fill_(float("inf") if k == 2 else 1.0)
            opt.step(closure)
        mult.fill_(1.0)
    pa, oa, ca, ma = _make(psgd, tail, exact, seed=4, **kw)
    run(oa, ca, ma, 1, 6)
    pb, ob, cb, mb = _make(psgd, tail, exact, seed=4, **kw)
    run(ob, cb, mb, 1, 3)
    sd = ob.state_dict()
    assert sd["skipped_steps"] == 1 and sd["momentum_step"] == 2 and sd["loss_scale"] == 2.0 ** 15
    assert sd["loss_scale_good_steps"] == 1 and sd["hyper"]["momentum"] == 0.9 and len(sd["momentum_buffers"]) == len(SHAPES)
    saved = [p.detach().clone() for p in pb]
    pc, oc, cc, mc = _make(psgd, tail, exact, seed=999, **kw)                        # a fresh object: other generator state
    oc.step(cc)                                                                      # ... and a used momentum buffer
    with torch.no_grad():
        for p, s in zip(pc, saved):
            p.copy_(s)
    oc.load_state_dict(sd)
    assert oc.skipped_steps == 1 and float(oc.loss_scale) == 2.0 ** 15 and oc._m_step == 2
    run(oc, cc, mc, 4, 6)
    _assert_state(_state(pc, oc), _state(pa, oa), "3 + 3 resumed steps against 6")
    assert float(oc.loss_scale) == float(oa.loss_scale) and oc.skipped_steps == oa.skipped_steps == 1


def test_loading_a_dict_without_the_features_restarts_the_warm_up(psgd):
    _, plain, closure, _ = _make(psgd, "fused", True)
    plain.step(closure)
    sd = plain.state_dict()
    assert "momentum_buffers" not in sd and "nonfinite" not in sd
    del sd["hyper"]["momentum"], sd["hyper"]["weight_decay"]                         # as a dict from before them
    params, opt, closure, _ = _make(psgd, "fused", True, momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale=2.0 ** 8)
    for _ in range(2):
        opt.step(closure)
    opt.load_state_dict(sd)
    assert float(opt.momentum) == 0.9 and float(opt.weight_decay) == 0.01            # this object's values stay
    assert opt._m_step == 0 and all(not bool(m.any()) for m in opt._m)
    assert float(opt.loss_scale) == 2.0 ** 8 and opt.skipped_steps == 0
    opt.step(closure)
    assert opt._m_step == 1 and all(bool(torch.isfinite(p).all()) for p in params)
