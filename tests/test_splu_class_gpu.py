"""class SPLU on the GPU: bit for bit against the loop a user writes by hand from update_precond_splu / precond_grad_splu
(demo_usage_of_all_preconditioners.py:46-62 with the step tail of psgd.py:750-762), fused tail against torch tail, parity with the
fp64 oracle, the bf16-stored state, every switch of the shared step-feature layer, the whitening fit, resume, a first call on
poisoned buffers, the allocation condition of the in-place route and a convergence smoke.

Parameter shapes: N = 65 (a partial last tile, the r x r corner inside tile 0), N = 131 with rank 40 (the 64-row-tile kernels) and
N = 150 with rank 70 (the column chunks of splu_wide.py) and N = 5003 (several workgroups per sweep).  The initial scale is 1 unless stated, so that the clip is active."""
import math

import numpy as np
import pytest
import torch
from torch.autograd.function import once_differentiable

from oracle import psgd_oracle as orc
from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl
from tests.test_multi_randn_gpu import BAR as PROBE_BAR               # |kernel - counter_randn| per element, that file's bar
from tests.uvd_cases import rel_err

pytestmark = pytest.mark.gpu

S65 = [(7, 5), (5,), (3, 4, 2), ()]
S131 = S65 + [(11, 6)]
S150 = S131 + [(19,)]
S5003 = [(50, 60), (1000,), (7, 11, 13), (2,)]      # several blocks of the sweeps; in-place against pure beyond one block
LR, LR_Q, MAX_NORM = 0.05, 0.1, 2.0
TINY = float(np.finfo(np.float32).tiny)
DELTA = float(np.finfo(np.float32).eps) ** 0.5
STEPS = 3


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


_data = {}


def _problem(shapes):
    """initial parameters, the weights a of the loss (c: unused) and six steps of probe draws: float32 device tensors, made once"""
    key = tuple(shapes)
    if key not in _data:
        rng = np.random.default_rng(2027)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())
        _data[key] = ([f(rng.standard_normal(s) * 0.5) for s in shapes], [f(np.exp(rng.uniform(-1.0, 1.0, s))) for s in shapes],
                      [f(rng.standard_normal(s) * 0.05) for s in shapes], [f(rng.standard_normal(s)) for _ in range(6) for s in shapes])
    return _data[key]


class _OnceTanh(torch.autograd.Function):
    """tanh whose backward cannot be differentiated again: the stand-in for a fused kernel"""

    @staticmethod
    def forward(ctx, x):
        y = torch.tanh(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return gy * (1.0 - y * y)


def _closure(params, shapes, poison=None, once=False, calls=None):
    """sum_k sum a cosh(W) in float32: the gradient a sinh(W), a Hessian diag(a cosh(W)) that changes with W.  Every parameter
    enters the loss, the gradient and the Hessian-vector product through ONE elementwise chain: no reduction feeds them and
    autograd has no two contributions to add, so two evaluations fed the same draws give the same (v, h, g) bit for bit (closures
    with a coupling term or several terms per parameter gave Hessian-vector products that parted by an ulp between two
    evaluations).  once: sum a tanh(W)^2 / 4 through the once_differentiable Function.  poison: a dict whose "x" (when not 1)
    multiplies element 3 of the first parameter into the loss"""
    a_s = _problem(shapes)[1]

    def closure():
        if calls is not None:
            calls.append(1)
        loss = 0.0
        for p, a in zip(params, a_s):
            W = p.float()
            loss = loss + (0.25 * torch.sum(a * _OnceTanh.apply(W) ** 2) if once else torch.sum(a * torch.cosh(W)))
        if poison is not None and poison["x"] != 1.0:
            loss = loss + params[0].float().reshape(-1)[3] * poison["x"]
        return loss
    return closure


def _fresh(shapes, dtype=torch.float32):
    return [w.clone().to(dtype).requires_grad_(True) for w in _problem(shapes)[0]]


def _feed(monkeypatch, shapes):
    """the draws of psgd.py:713 / :721 come from the problem's list, in order, for whoever steps next"""
    it = iter(_problem(shapes)[3])
    monkeypatch.setattr(impl, "_randn_like", lambda p: next(it).to(p.dtype))


def _make(psgd, tail, shapes=S65, r=4, exact=True, clip=False, prob=1.0, seed=11, dtype=torch.float32, scale=1.0, poison=None,
          once=False, calls=None, **kw):
    params = _fresh(shapes, dtype)
    opt = psgd.SPLU(params, r, scale, LR, LR_Q, MAX_NORM if clip else None, prob, exact, generator=torch.Generator().manual_seed(seed),
                    step_tail=tail, **kw)
    assert (opt._tail is not None) == (tail == "fused")
    return params, opt, _closure(params, shapes, poison, once, calls)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy().copy()


def _state(params, opt):
    mom = opt._momentum_buffer() if float(opt.momentum) > 0.0 else None
    return {"tensors": [_bits(t) for t in list(params) + list(opt.factors) + ([mom] if mom is not None else [])],
            "counters": (opt._m_step, opt.probe_step, opt._param_round_step, getattr(opt, "_round_step", None), opt.skipped_steps)}


def _assert_same(a, b, what):
    assert len(a["tensors"]) == len(b["tensors"]), what
    for i, (x, y) in enumerate(zip(a["tensors"], b["tensors"])):
        assert x.tobytes() == y.tobytes(), "%s: tensor %d differs" % (what, i)
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])


def _run(psgd, monkeypatch, tail, steps=STEPS, **kw):
    _feed(monkeypatch, kw.get("shapes", S65))
    params, opt, closure = _make(psgd, tail, **kw)
    for _ in range(steps):
        opt.step(closure)
    assert all(bool(torch.isfinite(p.float()).all()) for p in params)
    return _state(params, opt), opt


# --------------------------------------------------------------------------------------------------- the hand-written loop
def _hand_step(psgd, params, state, closure, vs, k, exact, clip, mom, wd, m, whiten_dx=None):
    """One step of the loop a user writes from the two functions and torch ops.  whiten_dx: the flat probe of a whitening step
    ((dx, dg) = (probe, gradient), one backward).  Returns (state, m)."""
    undo = None
    if whiten_dx is not None:
        grads = torch.autograd.grad(closure(), params)
        dxs, dgs = [whiten_dx], list(grads)
    elif exact:
        grads = torch.autograd.grad(closure(), params, create_graph=True)
        Hvs = torch.autograd.grad(grads, params, vs)
        grads = [g.detach() for g in grads]
        dxs, dgs = vs, Hvs
    else:
        grads = torch.autograd.grad(closure(), params)
        undo = [v * DELTA for v in vs]
        with torch.no_grad():
            for p, v in zip(params, undo):
                p.add_(v)
        perturbed = torch.autograd.grad(closure(), params)
        dxs, dgs = [v / DELTA for v in undo], [(pg - g) / DELTA for pg, g in zip(perturbed, grads)]
    with torch.no_grad():
        state = psgd.update_precond_splu(*state, dxs, dgs, LR_Q)
        feed = list(grads)
        if mom != 0.0:                       # m <- beta_k m + (1 - beta_k) g, beta_k = min(k / (k + 1), momentum); m is preconditioned
            beta, omb = psgd.uvd_momentum_coefficients(k, mom)
            g = torch.cat([x.reshape(-1) for x in grads])
            m = g * omb if beta == 0.0 else m * beta + g * omb
            feed = [m]
        pre = torch.cat([x.reshape(-1) for x in psgd.precond_grad_splu(*state, feed)])
        decay = None
        if mom != 0.0 or wd != 0.0:          # lr_eff as the step-tail kernel forms it (UVd.step): fp64 from the fp32 squares, one rounding
            lr = torch.tensor(LR, dtype=torch.float32, device=_dev())
            if clip:
                f32 = lambda x: float(np.float32(x))
                ratio = f32(MAX_NORM) / (torch.sqrt(torch.sum((pre * pre).double())) + f32(TINY))
                lr = (lr.double() * torch.clamp(ratio, max=1.0)).float()
            if wd != 0.0:
                decay = lr * torch.tensor(wd, dtype=torch.float32, device=_dev())
        elif clip:                           # psgd.py:753-754
            lr = LR * torch.clamp(MAX_NORM / (torch.sqrt(torch.sum(pre * pre)) + TINY), max=1.0)
        else:
            lr = LR
        i = 0
        for j, p in enumerate(params):
            delta = lr * pre[i:i + p.numel()].reshape(p.shape)
            if undo is not None:
                delta = delta + undo[j]
            if decay is not None:
                delta = delta + decay * p
            p.sub_(delta)
            i += p.numel()
    return state, m


_hand_runs = {}


def _hand_run(psgd, shapes, r, exact, clip, mom=0.0, wd=0.0, steps=STEPS):
    """computed once per configuration, shared by the tests of both tails (never modified)"""
    key = (tuple(shapes), r, exact, clip, mom, wd, steps)
    if key not in _hand_runs:
        params = _fresh(shapes)
        closure = _closure(params, shapes)
        state = psgd.splu_initial_factors(sum(p.numel() for p in params), r, 1.0, device=_dev())
        draws, m = iter(_problem(shapes)[3]), None
        for k in range(steps):
            vs = [next(draws) for _ in params]
            state, m = _hand_step(psgd, params, state, closure, vs, k, exact, clip, mom, wd, m)
        tensors = [_bits(t) for t in list(params) + list(state) + ([m] if m is not None else [])]
        _hand_runs[key] = {"tensors": tensors, "counters": (steps if mom else 0, 0, 0, None, 0)}
    return _hand_runs[key]


ROUTES = [(S65, 4), (S65, 40), (S131, 4), (S131, 40), (S150, 70), (S5003, 7), (S5003, 40)]
ROUTE_IDS = ["N65-r4", "N65-r40", "N131-r4", "N131-r40", "N150-r70", "N5003-r7", "N5003-r40"]


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("shapes, r", ROUTES, ids=ROUTE_IDS)
def test_torch_tail_equals_the_hand_written_loop(psgd, monkeypatch, shapes, r, exact, clip):
    """3 steps; parameters and all four factors bit for bit.  For ranks up to 64 this is the in-place call (the *_new pointers of
    psgd_splu_update_f32 on the state itself) against the pure one."""
    got, opt = _run(psgd, monkeypatch, "torch", shapes=shapes, r=r, exact=exact, clip=clip)
    assert opt._in_place == (r <= 64)
    _assert_same(got, _hand_run(psgd, shapes, r, exact, clip), "SPLU(step_tail='torch') against the hand-written loop")


def test_in_place_route_keeps_its_tensors_and_the_wide_route_replaces_them(psgd, monkeypatch):
    for r, kept in ((40, True), (70, False)):
        _feed(monkeypatch, S150)
        params, opt, closure = _make(psgd, "fused", shapes=S150, r=r)
        before = [t.data_ptr() for t in opt.factors] + [opt._out.data_ptr()]
        pre = opt._precondition(None, None, opt._flat_bufs["g"].zero_())
        assert (pre.data_ptr() == opt._out.data_ptr()) == kept
        opt.step(closure)
        assert ([t.data_ptr() for t in opt.factors] + [opt._out.data_ptr()] == before) == kept


# ------------------------------------------------------------------------------------------------------ fused against torch
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("shapes, r", ROUTES, ids=ROUTE_IDS)
def test_fused_tail_without_clipping_is_bit_identical(psgd, monkeypatch, shapes, r, exact):
    got, _ = _run(psgd, monkeypatch, "fused", shapes=shapes, r=r, exact=exact)
    _assert_same(got, _hand_run(psgd, shapes, r, exact, False), "SPLU(step_tail='fused') without clipping")


def _dyadic_run(psgd, tail):
    """a closure whose gradient is a fixed dyadic tensor, no factor update, factors 0.5 I: the preconditioned gradient is that
    tensor / 16 and its sum of squares is exact in any order.  momentum 0.5 on a constant gradient leaves m = g exactly and puts
    both tails on the kernel's expression of lr_eff (UVd.step: fp64 from the fp32 squares, rounded once)"""
    gen = torch.Generator().manual_seed(3)
    Ds = [(torch.randint(-64, 65, s, generator=gen).float() / 16.0).to(_dev()) for s in S65]
    params = _fresh(S65)
    opt = psgd.SPLU(params, 4, 0.5, LR, LR_Q, 0.25, 0.0, True, step_tail=tail, generator=torch.Generator().manual_seed(5),
                    momentum=0.5)
    for _ in range(STEPS):
        opt.step(lambda: sum(torch.sum(p * d) for p, d in zip(params, Ds)))
    assert bool(torch.equal(opt._out, torch.cat([d.reshape(-1) for d in Ds]) / 16.0))
    assert float(opt._out.norm()) > 0.25                                           # the clip is active
    return _state(params, opt)


def test_fused_tail_with_clipping_on_dyadic_gradients_is_bit_identical(psgd):
    a, b = _dyadic_run(psgd, "torch"), _dyadic_run(psgd, "fused")
    _assert_same(b, a, "clipped step on dyadic gradients")
    assert a["tensors"][0].tobytes() != _bits(_fresh(S65)[0]).tobytes()            # the parameters did move


def _lr_eff(S):
    f64 = lambda x: torch.tensor(float(np.float32(x)), dtype=torch.float64, device=_dev())
    return (f64(LR) * torch.minimum(f64(MAX_NORM) / (torch.sqrt(S) + f64(TINY)), f64(1.0))).float()


@pytest.mark.parametrize("exact", [True, False])
def test_fused_tail_with_clipping_on_random_data(psgd, monkeypatch, exact):
    """The bar of test_fused_tail_with_clipping_on_random_data of class Kron (tests/test_kron_class_gpu.py), step by step: the two
    S agree within n 2^-53; where the two fl32(lr_eff) are equal the parameters are bit-identical, otherwise they differ by at most
    one ulp of lr_eff times |pg|.  That bar is stated for a torch tail that forms lr_eff as the kernel does; UVd.step, which
    class SPLU runs, does so when momentum or weight decay is on (here: momentum 0.9, pg = P m).  The plain torch tail keeps the
    reference's float32 expression of psgd.py:753-754 and is held to the bar class UVd has for it, in the test below."""
    n, runs, draws = 65, {}, {}
    for tail in ("torch", "fused"):
        runs[tail] = _make(psgd, tail, exact=exact, clip=True, momentum=0.9, seed=21)
        draws[tail] = iter(_problem(S65)[3])
    cases = []
    for step in range(STEPS):
        pre = {}
        for tail in ("torch", "fused"):
            monkeypatch.setattr(impl, "_randn_like", lambda p, it=draws[tail]: next(it).to(p.dtype))
            runs[tail][1].step(runs[tail][2])
            pre[tail] = runs[tail][1]._out.clone()
        assert _bits(pre["torch"]).tobytes() == _bits(pre["fused"]).tobytes()         # the same inputs so far: the same gradient
        S_t, S_f = float(torch.sum((pre["torch"] * pre["torch"]).double())), float(runs["fused"][1]._tail.sumsq[0])
        print("step %d: S torch %.17g, fused %.17g, relative difference %.3e (bound %.3e)"
              % (step, S_t, S_f, abs(S_t - S_f) / S_t, n * 2.0 ** -53))
        assert abs(S_t - S_f) <= n * 2.0 ** -53 * S_t
        lr_t = float(_lr_eff(torch.tensor(S_t, dtype=torch.float64, device=_dev())))
        lr_f = float(_lr_eff(torch.tensor(S_f, dtype=torch.float64, device=_dev())))
        assert lr_t < float(np.float32(LR))                                            # the clip is active
        if lr_t == lr_f:
            cases.append("equal")
            _assert_same(_state(*runs["fused"][:2]), _state(*runs["torch"][:2]), "clipped step %d with equal lr_eff" % step)
        else:
            cases.append("one ulp")
            ulp = float(np.spacing(np.float32(max(lr_t, lr_f))))
            assert abs(lr_t - lr_f) <= ulp
            p_t = torch.cat([p.detach().reshape(-1) for p in runs["torch"][0]]).double()
            p_f = torch.cat([p.detach().reshape(-1) for p in runs["fused"][0]]).double()
            assert bool(((p_t - p_f).abs() <= ulp * pre["torch"].double().abs()).all())
            break                                                                      # (the runs have parted: later steps compare nothing)
    print("lr_eff of the two tails per step: %s" % cases)


@pytest.mark.parametrize("exact", [True, False])
def test_plain_fused_tail_with_clipping_on_random_data(psgd, monkeypatch, exact):
    """no switch on: the torch tail is the float32 expression of psgd.py:753-754, the fused one the kernel's fp64 norm.  The bar
    of test_class_fused_tail_with_clipping of class UVd (tests/test_uvd_tail_gpu.py): 1e-6, relative and norm-wise."""
    a, _ = _run(psgd, monkeypatch, "torch", exact=exact, clip=True)
    b, _ = _run(psgd, monkeypatch, "fused", exact=exact, clip=True)
    x = np.concatenate([t.view(np.float32).reshape(-1) for t in b["tensors"][:4]]).astype(np.float64)
    y = np.concatenate([t.view(np.float32).reshape(-1) for t in a["tensors"][:4]]).astype(np.float64)
    rel = float(np.linalg.norm(x - y) / np.linalg.norm(y))
    print("clipped plain run, exact=%s: relative difference %.3g" % (exact, rel))
    assert rel <= 1e-6


# ------------------------------------------------------------------------------------------------------------- fp64 oracle
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("shapes, r", [(S65, 4), (S131, 40), (S150, 70)], ids=["N65-r4", "N131-r40", "N150-r70"])
def test_parity_with_the_fp64_oracle(psgd, monkeypatch, shapes, r, tail):
    """3 exact steps against an independent float64 trajectory: oracle/psgd_oracle.py's update_precond_splu / precond_grad_splu
    driven by a float64 restatement of the step -- float64 parameters, the closure's gradient a sinh(W) and Hessian-vector product
    a cosh(W) v in float64, the clip of psgd.py:753-754, the update -- that shares with the class only the initial values and the
    probe draws; nothing is resynchronised between the steps.  After every step, the third included: the four factors and the
    preconditioned gradient (captured at _precondition, on every route) within 1e-5, relative and norm-wise, and the parameter
    increments p_k - p_0 within 1e-5 of their own norm.  The clipped increment is about 0.1 k in norm, so 0.1 k / sqrt(N) per
    element, against float32 parameters of about 0.5 that are known to 2^-25 |p| / sqrt(3) = 9e-9: a rounding share of at most
    1e-6 at N <= 150.  (At N = 5003 that share alone is 6e-6 / k: the bar cannot be asked of float32 parameters there, and the
    shapes of that size are held bit for bit against the hand-written loop above instead.)"""
    _feed(monkeypatch, shapes)
    params, opt, closure = _make(psgd, tail, shapes=shapes, r=r, clip=True)
    n64 = lambda t: t.detach().float().cpu().numpy().astype(np.float64)
    flat64 = lambda ts: np.concatenate([n64(t).reshape(-1) for t in ts])[:, None]
    seen = []
    real = opt._precondition
    monkeypatch.setattr(opt, "_precondition", lambda *a: seen.append(real(*a).clone()) or seen[-1])
    state = [n64(t) for t in opt.factors]
    a64, W0 = flat64(_problem(shapes)[1]), flat64(params)
    W, draws = W0.copy(), iter(_problem(shapes)[3])
    for k in range(STEPS):
        v = flat64([next(draws) for _ in params])
        g, h = a64 * np.sinh(W), a64 * np.cosh(W) * v
        state = orc.update_precond_splu(*state, [v], [h], float(np.float32(LR_Q)))
        pre = orc.precond_grad_splu(*state, [g])[0].reshape(-1, 1)
        W = W - float(orc.uvd_clip_lr(pre, float(np.float32(LR)), MAX_NORM, TINY)) * pre
        opt.step(closure)
        errs = [rel_err(n64(got), ref) for got, ref in zip(opt.factors, state)]
        e_pre = rel_err(n64(seen[k]).reshape(-1, 1), pre)
        e_inc = rel_err(flat64(params) - W0, W - W0)
        print("step %d N=%d r=%d: L12 %.2e l3 %.2e U12 %.2e u3 %.2e, preconditioned gradient %.2e, increment %.2e"
              % (k, W.size, r, *errs, e_pre, e_inc))
        assert max(errs) < 1e-5 and e_pre < 1e-5 and e_inc < 1e-5, (k, errs, e_pre, e_inc)
    assert len(seen) == STEPS


# -------------------------------------------------------------------------------------------------------------- bf16 state
@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_bf16_state_equals_the_functional_update_with_the_same_seed_stream(psgd, monkeypatch, tail, rounding):
    _feed(monkeypatch, S131)
    params, opt, closure = _make(psgd, tail, shapes=S131, r=20, state_dtype=torch.bfloat16, state_rounding=rounding)
    assert all(t.dtype == torch.bfloat16 for t in opt.factors) and opt._state_rounding == rounding
    seed0, state = opt._round_seed0, [t.clone() for t in opt.factors]
    draws = iter(_problem(S131)[3])
    for k in range(STEPS):
        vs = [next(draws) for _ in params]
        with torch.enable_grad():
            grads = torch.autograd.grad(closure(), params, create_graph=True)
            Hvs = torch.autograd.grad(grads, params, vs)
        opt.step(closure)
        state = psgd.update_precond_splu(*state, vs, Hvs, LR_Q, rounding=rounding, rounding_seed=psgd.uvd_step_rounding_seed(seed0, k))
        for name, got, ref in zip(("L12", "l3", "U12", "u3"), opt.factors, state):
            assert got.dtype == torch.bfloat16 and _bits(got).tobytes() == _bits(ref).tobytes(), (k, name)
    assert opt._round_step == STEPS


def test_bf16_state_follows_the_parameters_and_refuses_rank_33(psgd):
    opt = psgd.SPLU(_fresh(S65, torch.bfloat16), 32, state_dtype="param")
    assert opt._L12.dtype == torch.bfloat16 and opt._state_rounding == "stochastic"
    with pytest.raises(ValueError, match="ranks up to 32"):
        psgd.SPLU(_fresh(S65), 33, state_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="float16 state"):
        psgd.SPLU(_fresh(S65), 4, state_dtype=torch.float16)


# ------------------------------------------------------------------------------------------------------------ every switch
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("exact, clip", [(True, False), (False, True)])
@pytest.mark.parametrize("mom, wd", [(0.9, 0.0), (0.0, 0.01), (0.9, 0.01)])
def test_momentum_and_weight_decay_equal_the_hand_written_loop(psgd, monkeypatch, mom, wd, exact, clip, tail):
    """momentum: the flat gradient is blended into m (beta_k = min(k / (k + 1), momentum)) and m is preconditioned; weight decay:
    delta gains fl32(fl32(lr_eff wd) p).  Both tails, bit for bit (with clipping on the fused tail: within the clip bar of the
    plain test above)."""
    got, opt = _run(psgd, monkeypatch, tail, exact=exact, clip=clip, momentum=mom, weight_decay=wd)
    want = _hand_run(psgd, S65, 4, exact, clip, mom, wd)
    assert opt._m_step == (STEPS if mom else 0)
    if tail == "fused" and clip:         # the two sums of squares may part by n 2^-53 and lr_eff by an ulp: class UVd's bar, 1e-6
        for i, (x, y) in enumerate(zip(got["tensors"], want["tensors"])):
            x, y = x.view(np.float32).astype(np.float64), y.view(np.float32).astype(np.float64)
            assert np.linalg.norm(x - y) <= 1e-6 * np.linalg.norm(y), "tensor %d" % i
        assert got["counters"] == want["counters"]
    else:
        _assert_same(got, want, "momentum %r, weight decay %r" % (mom, wd))


SWITCHES = {
    "momentum": dict(momentum=0.9),
    "weight decay": dict(weight_decay=0.01),
    "momentum, weight decay, finite differences": dict(momentum=0.9, weight_decay=0.01, exact=False),
    "bfloat16 parameters": dict(dtype=torch.bfloat16, momentum=0.5),
    "float16 parameters": dict(dtype=torch.float16, weight_decay=0.01),
    "float16 parameters, finite differences": dict(dtype=torch.float16, exact=False),
    "bfloat16, stochastic rounding": dict(dtype=torch.bfloat16, param_rounding="stochastic", param_rounding_seed=5, weight_decay=0.01),
    "bfloat16 state": dict(state_dtype=torch.bfloat16, momentum=0.9),
    "guarded": dict(nonfinite="skip", momentum=0.9),
    "rank 40": dict(shapes=S131, r=40, momentum=0.9),
    "rank 70": dict(shapes=S150, r=70, weight_decay=0.01),
    "rank N": dict(r=65),
}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_both_tails_bit_identical(psgd, monkeypatch, name):
    a, oa = _run(psgd, monkeypatch, "torch", **SWITCHES[name])
    b, ob = _run(psgd, monkeypatch, "fused", **SWITCHES[name])
    _assert_same(b, a, name)
    dtype = SWITCHES[name].get("dtype", torch.float32)
    assert all(p.dtype == dtype for p in oa._params + ob._params)
    assert all(t.dtype == SWITCHES[name].get("state_dtype", torch.float32) for t in ob.factors)
    if "param_rounding" in SWITCHES[name]:
        assert oa._param_round_step == STEPS
        c, _ = _run(psgd, monkeypatch, "fused", **dict(SWITCHES[name], param_rounding="nearest", param_rounding_seed=None))
        assert any(x.tobytes() != y.tobytes() for x, y in zip(b["tensors"][:4], c["tensors"][:4]))     # the rounding is another


@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("fit", ["hessian", "whitening"])
def test_a_skipped_step_keeps_every_bit_and_every_counter(psgd, monkeypatch, fit, tail, mom):
    """nonfinite="skip" with an Inf in one gradient element (exact products: nothing was perturbed, so the parameters keep their
    bits too): factors, parameters, momentum buffer and all counters as they were, skipped_steps == 1"""
    _feed(monkeypatch, S65)
    poison = {"x": 1.0}
    params, opt, closure = _make(psgd, tail, nonfinite="skip", momentum=mom, poison=poison, preconditioner_fit=fit, probe_seed=9,
                                 state_dtype=torch.bfloat16 if mom else None)
    for _ in range(2):
        opt.step(closure)
    before = _state(params, opt)
    poison["x"] = float("inf")
    loss = opt.step(closure)
    assert opt.last_step_skipped and opt.skipped_steps == 1 and not math.isfinite(float(loss))
    after = _state(params, opt)
    after["counters"] = after["counters"][:4] + (0,)
    _assert_same(after, before, "a skipped step")
    poison["x"] = 1.0
    opt.step(closure)
    assert not opt.last_step_skipped and opt.skipped_steps == 1
    assert _state(params, opt)["tensors"][0].tobytes() != before["tensors"][0].tobytes()


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_a_loss_scale_does_not_move_a_bit_of_a_float32_run(psgd, monkeypatch, tail, exact):
    plain, _ = _run(psgd, monkeypatch, tail, exact=exact, clip=True, momentum=0.9)
    guarded, _ = _run(psgd, monkeypatch, tail, exact=exact, clip=True, momentum=0.9, nonfinite="skip")
    scaled, opt = _run(psgd, monkeypatch, tail, exact=exact, clip=True, momentum=0.9, nonfinite="skip", loss_scale=2 ** 8)
    assert float(opt.loss_scale) == 256.0 and opt.skipped_steps == 0
    _assert_same(guarded, plain, "nonfinite='skip' on finite data")
    _assert_same(scaled, plain, "loss_scale=2**8")


# --------------------------------------------------------------------------------------------------------------- whitening
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("shapes, r", [(S65, 4), (S131, 40)], ids=["N65-r4", "N131-r40"])
def test_one_whitening_step_equals_the_hand_written_loop(psgd, shapes, r, tail):
    """(dx, dg) = (probe, raw gradient).  The flat probe is the multi_randn draw of (probe_seed0, step 0) and lies within that
    kernel's bar of counter_randn; the step equals the hand-written loop bit for bit when the loop is fed the kernel's probe and
    within 1e-5 (relative, norm-wise: counter_randn is the same draw to a few float32 ulps) when it is fed counter_randn's.
    The clip is on with the torch tail only: the plain fused tail forms the clipped lr_eff from the kernel's fp64 norm, not from the
    float32 expression of psgd.py:753-754 the loop writes, and is bit-identical without clipping (the tests above hold it to its
    clip bar)."""
    clip = tail == "torch"
    params, opt, closure = _make(psgd, tail, shapes=shapes, r=r, clip=clip, preconditioner_fit="whitening", probe_seed=77)
    N = sum(p.numel() for p in params)
    opt.step(closure)
    seed = psgd.uvd_step_rounding_seed(77, 0)
    want = torch.empty(N, device=_dev())
    psgd.multi_randn([want], seed, 0)
    v32 = psgd.counter_randn(seed, 0, N)
    assert _bits(opt._flat_bufs["v"]).tobytes() == _bits(want).tobytes() and opt.probe_step == 1
    assert float(np.max(np.abs(want.cpu().numpy().astype(np.float64) - v32.astype(np.float64)))) <= PROBE_BAR
    runs = []
    for dx in (want, torch.from_numpy(v32).to(_dev())):
        hp = _fresh(shapes)
        state = psgd.splu_initial_factors(N, r, 1.0, device=_dev())
        state, _ = _hand_step(psgd, hp, state, _closure(hp, shapes), None, 0, True, clip, 0.0, 0.0, None, whiten_dx=dx)
        runs.append(list(hp) + list(state))
    got = list(params) + list(opt.factors)
    for i, (a, b) in enumerate(zip(got, runs[0])):
        assert _bits(a).tobytes() == _bits(b).tobytes(), "tensor %d against the loop fed the kernel's probe" % i
    for i, (a, b) in enumerate(zip(got, runs[1])):
        assert rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 1e-5, "tensor %d against the loop fed counter_randn" % i


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_whitening_needs_one_backward_and_counts_updating_unskipped_steps(psgd, tail):
    calls, poison = [], {"x": 1.0}
    params, opt, closure = _make(psgd, tail, preconditioner_fit="whitening", probe_seed=3, once=True, calls=calls, poison=poison,
                                 nonfinite="skip")
    state = torch.cuda.get_rng_state()
    for k in range(2):
        opt.step(closure)                                                  # a once_differentiable closure runs: no second backward
        assert opt.probe_step == k + 1 and len(calls) == k + 1
    assert torch.equal(torch.cuda.get_rng_state(), state)                  # no global draw
    opt.preconditioner_update_probability.assign(0.0)
    opt.step(closure)
    assert opt.probe_step == 2 and not opt.last_step_skipped
    opt.preconditioner_update_probability.assign(1.0)
    poison["x"] = float("inf")
    opt.step(closure)
    assert opt.probe_step == 2 and opt.last_step_skipped
    poison["x"] = 1.0
    opt.step(closure)
    assert opt.probe_step == 3
    hp, ho, hc = _make(psgd, tail, once=True)
    with pytest.raises(RuntimeError):
        ho.step(hc)                                                        # the Hessian fit cannot differentiate it twice


# ------------------------------------------------------------------------------------------------------------------ resume
RESUME = dict(momentum=0.9, nonfinite="skip", loss_scale=2 ** 4, preconditioner_fit="whitening", probe_seed=5, clip=True,
              weight_decay=0.01)


@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("state_dtype", [None, torch.bfloat16])
def test_resume_is_bit_identical(psgd, tail, state_dtype):
    """save after 2 steps, load into a fresh optimizer, 2 more: the bits of 4 uninterrupted steps (momentum, guard and whitening on)"""
    kw = dict(RESUME, state_dtype=state_dtype)
    params, opt, closure = _make(psgd, tail, **kw)
    for _ in range(4):
        opt.step(closure)
    want = _state(params, opt)
    p1, o1, c1 = _make(psgd, tail, **kw)
    for _ in range(2):
        o1.step(c1)
    sd = o1.state_dict()
    saved = [p.detach().clone() for p in p1]
    p2, o2, c2 = _make(psgd, tail, seed=999, **dict(kw, probe_seed=123))
    o2.lr_params.assign(9.0)
    o2.load_state_dict(sd)
    with torch.no_grad():
        for p, s in zip(p2, saved):
            p.copy_(s)
    for _ in range(2):
        o2.step(c2)
    _assert_same(_state(p2, o2), want, "resumed run")
    assert float(o2.lr_params) == LR and o2.probe_seed0 == 5


def test_resume_on_the_hessian_route_with_the_coin(psgd, monkeypatch):
    """preconditioner_update_probability 0.5: the generator behind the coin travels with the checkpoint"""
    got = []
    for split in (False, True):
        _feed(monkeypatch, S65)
        params, opt, closure = _make(psgd, "fused", prob=0.5, seed=4)
        for k in range(6):
            if split and k == 3:
                sd, keep = opt.state_dict(), [p.detach().clone() for p in params]
                params, opt, closure = _make(psgd, "fused", prob=0.5, seed=77)
                opt.load_state_dict(sd)
                with torch.no_grad():
                    for p, s in zip(params, keep):
                        p.copy_(s)
            opt.step(closure)
        got.append(_state(params, opt))
    _assert_same(got[1], got[0], "resumed run with coins")


# ------------------------------------------------------------------------------------------------ probability and .assign
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_update_probability_zero_and_one_and_assign(psgd, monkeypatch, tail):
    _feed(monkeypatch, S65)
    params, opt, closure = _make(psgd, tail, prob=0.0)
    f0, p0 = [_bits(t) for t in opt.factors], _bits(params[0])
    ret = opt.step(lambda: [closure(), "aux"])                                     # the closure may return a list (psgd.py:711)
    assert ret[1] == "aux"
    assert all(a.tobytes() == _bits(t).tobytes() for a, t in zip(f0, opt.factors)) and _bits(params[0]).tobytes() != p0.tobytes()
    opt.preconditioner_update_probability.assign(1.0)                              # takes effect on the next step
    opt.step(closure)
    assert all(a.tobytes() != _bits(t).tobytes() for a, t in zip(f0, opt.factors))
    opt.lr_params.assign(0.0)
    p1 = _bits(params[0])
    opt.step(closure)
    assert _bits(params[0]).tobytes() == p1.tobytes()
    opt.lr_params.assign(LR)
    opt.exact_hessian_vector_product.assign(False)                                 # the finite-difference route from here on
    opt.step(closure)
    assert _bits(params[0]).tobytes() != p1.tobytes() and all(bool(torch.isfinite(t).all()) for t in opt.factors)


# ----------------------------------------------------------------------------------------------- first call, poisoned buffers
@pytest.mark.parametrize("shapes, r, kw", [(S65, 4, {}), (S131, 40, dict(momentum=0.9, nonfinite="skip")),
                                           (S131, 20, dict(state_dtype=torch.bfloat16, momentum=0.9)),
                                           (S65, 4, dict(preconditioner_fit="whitening", probe_seed=1, momentum=0.9))],
                         ids=["plain", "rank 40 guarded momentum", "bf16 state", "whitening"])
def test_first_fused_step_on_poisoned_buffers(psgd, monkeypatch, shapes, r, kw):
    """the flat vectors, the output, the momentum buffer, the plan's reduction scratch and the cached workspace hold NaN / 0xFF
    before the first step: nothing reads what it has not written"""
    want, _ = _run(psgd, monkeypatch, "fused", shapes=shapes, r=r, clip=True, **kw)
    _feed(monkeypatch, shapes)
    params, opt, closure = _make(psgd, "fused", shapes=shapes, r=r, clip=True, **kw)
    N = opt._out.numel()
    for t in list(opt._flat_bufs.values()) + [opt._out]:
        t.fill_(float("nan"))
    if float(opt.momentum) > 0.0:
        opt._momentum_buffer().fill_(float("nan"))
    opt._tail.ws.fill_(0xFF)
    opt._tail.sumsq.fill_(float("nan"))
    (impl._splu_bf16_workspace if opt._bf16 else impl._splu_workspace)(_dev(), N, r).fill_(0xFF)
    for _ in range(STEPS):
        opt.step(closure)
    _assert_same(_state(params, opt), want, "first step on poisoned buffers")


# ------------------------------------------------------------------------------------------- no state-sized allocation
def test_a_fused_step_allocates_less_than_one_factor(psgd):
    """N = 100 000 in 8 tensors, r = 32, fp32, fused tail, a quadratic closure with a diagonal Hessian.  After 2 warm-up steps one
    step's peak above its entry level stays below 4 N r bytes (one factor, 12.8 MB); the same problem as the hand-written
    functional loop exceeds twice that (its update returns four fresh state tensors).  A condition, not a measurement."""
    N, r, k = 100_000, 32, 8
    gen = torch.Generator().manual_seed(0)
    a = [(torch.rand(N // k, generator=gen) + 0.5).to(_dev()) for _ in range(k)]
    factor = 4 * N * r

    def peak_of(step):
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        entry = torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - entry

    params = [torch.randn(N // k, generator=gen).to(_dev()).requires_grad_(True) for _ in range(k)]
    closure = lambda: sum(0.5 * torch.sum(x * p * p) for x, p in zip(a, params))
    opt = psgd.SPLU(params, r, 1.0, LR, LR_Q, MAX_NORM, step_tail="fused")
    assert opt._in_place
    cls = peak_of(lambda: opt.step(closure))

    hp = [p.detach().clone().requires_grad_(True) for p in params]
    hclosure = lambda: sum(0.5 * torch.sum(x * p * p) for x, p in zip(a, hp))
    box = {"state": psgd.splu_initial_factors(N, r, 1.0, device=_dev())}

    def hand():
        vs = [torch.randn_like(p) for p in hp]
        box["state"], _ = _hand_step(psgd, hp, box["state"], hclosure, vs, 0, True, True, 0.0, 0.0, None)
    fun = peak_of(hand)
    print("peak over one step: class %.2f MB, functional loop %.2f MB, one factor %.2f MB" % (cls / 1e6, fun / 1e6, factor / 1e6))
    assert cls < factor
    assert fun > 2 * factor


# -------------------------------------------------------------------------------------------------------- convergence smoke
def test_the_example_converges():
    """examples/splu_class.py (the demo's tensor decomposition, 100 steps at the demo's settings) printed on its first run on an
    MI355X: loss 37728.8789 -> 3327.3694, a factor of 11.3, i.e. a ratio last / first of 0.0882; the bar leaves a factor of 10 on
    that ratio for other seeds"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "splu_class.py")
    spec = importlib.util.spec_from_file_location("splu_class_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.main(steps=100, quiet=True)
    assert all(math.isfinite(x) for x in losses)
    assert losses[-1] / losses[0] < 10 * 0.0882, (losses[0], losses[-1])
    assert all(b < a for a, b in zip(losses[::10], losses[10::10])), losses[::10]      # down over every ten steps, as on that run
    # the same steps with the preconditioner frozen at its initial 1e-4 I (update probability 0): what is gained is the fit's
    frozen = mod.main(steps=100, quiet=True, preconditioner_update_probability=0.0)
    print("fitted %.4f -> %.4f, frozen preconditioner %.4f -> %.4f" % (losses[0], losses[-1], frozen[0], frozen[-1]))
    assert losses[-1] < frozen[-1]
