"""class Kron on bfloat16 / float16 parameters: fused tail against torch tail bit for bit, one step against the fp64 restatement of
tests/kron_class_cases.py, the guard on an fp16 overflow, loss scaling, resume, the launch budget, and that float32 optimizers never
reach the typed kernels.  Shapes 5 x 7, 33 x 9 and 64 x 130: the quadratic problems of tests/kron_class_cases.py with the parameters
rounded to T.  The closure widens the parameters and computes in float32, so autograd hands back gradients rounded to T.
The Inf gradients here are data that the guard must catch (an fp16 gradient that overflows under its loss scale)."""
import collections

import numpy as np
import pytest
import torch

from tests import kron_class_cases as kc

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7), (33, 9), (64, 130)]
FORMAT_SETS = [[("dense", "dense"), ("dense", "norm"), ("dense", "scale")],
               [("norm", "dense"), ("norm", "scale"), ("scale", "dense")],
               [("scale", "norm"), ("dense", "dense"), ("norm", "dense")]]
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
LR, LR_Q, MAX_NORM = 0.05, 0.1, 2.0
ON = dict(momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale=2.0 ** 8)
LAUNCHES = collections.defaultdict(lambda: 1, psgd_multi_sumsq_f32=2)          # launches of one call of a list-kernel entry point


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _bits_equal(a, b):
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return a.dtype == b.dtype and bool(((a.view(v) == b.view(v)) | (torch.isnan(a) & torch.isnan(b))).all())


_problems = {}


def _problem(seed=0):
    """(Ws fp64, Hl, Hr fp32 on the device): made once"""
    if seed not in _problems:
        Ws, Hls, Hrs = kc.quadratic_problem(SHAPES, seed)
        f = lambda a: torch.from_numpy(a.astype(np.float32)).to(_dev())
        _problems[seed] = (Ws, [f(h) for h in Hls], [f(h) for h in Hrs])
    return _problems[seed]


def _fresh_params(dtype, seed=0):
    return [torch.from_numpy(w.astype(np.float32)).to(_dev()).to(dtype).requires_grad_(True) for w in _problem(seed)[0]]


def _closure(params, seed=0):
    _, Hl, Hr = _problem(seed)

    def closure():
        return sum(0.5 * torch.sum(W.float() * (hl @ W.float() @ hr)) for W, hl, hr in zip(params, Hl, Hr))
    return closure


def _make(psgd, dtype, tail, exact, *, formats=FORMAT_SETS[0], clip=False, seed=11, prob=1.0, **kw):
    params = _fresh_params(dtype)
    opt = psgd.Kron(params, formats, 1.0, LR, LR_Q, MAX_NORM if clip else None, prob, exact, step_tail=tail, generator=_gen(seed),
                    **kw)
    return params, opt, _closure(params)


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


def _run(psgd, dtype, tail, exact, steps, **kw):
    params, opt, closure = _make(psgd, dtype, tail, exact, **kw)
    for _ in range(steps):
        opt.step(closure)
    return _state(params, opt), opt


# ---------------------------------------------------------------------------------------------------- fused against torch
CASES = [(d, e, on) for d in DTYPES for e in (True, False) for on in (False, True)]


def test_the_cases_cover_the_seven_formats():
    used = {f for k in range(len(CASES)) for f in FORMAT_SETS[k % 3]}
    from psgd_tf_amd import kron_optimizer as ko
    assert used == set(ko.KRON_PAIRS)


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%s-%s" % (IDS[DTYPES.index(d)], "exact" if e else "fd", "on" if on else "off")
                                                        for d, e, on in CASES])
def test_fused_tail_equals_torch_tail(psgd, case):
    """6 steps; "on": momentum 0.9, weight decay 0.01, the guard and loss scale 2^8 (clipping: the dyadic test below)"""
    dtype, exact, on = CASES[case]
    kw = dict(formats=FORMAT_SETS[case % 3], **(ON if on else {}))
    a, oa = _run(psgd, dtype, "torch", exact, 6, **kw)
    b, ob = _run(psgd, dtype, "fused", exact, 6, **kw)
    _assert_state(b, a, "fused against torch")
    assert all(p.dtype == dtype and bool(torch.isfinite(p).all()) for p in a["params"])
    assert all(q.dtype == torch.float32 for pair in a["factors"] for q in pair)
    assert (a["momentum"] is not None) == on and all(m.dtype == torch.float32 for m in a["momentum"] or ())
    assert oa.skipped_steps == ob.skipped_steps == 0
    start = _fresh_params(dtype)
    assert not any(_bits_equal(p, s.detach()) for p, s in zip(a["params"], start))       # every parameter moved


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_tail_equals_torch_tail_with_clipping_on_dyadic_gradients(psgd, dtype):
    """a closure whose gradient is a fixed dyadic tensor (j / 16, |j| <= 64: exact in T), no factor update, identity factors,
    momentum 0.5 (beta_k = 0, 1/2, 1/2): the preconditioned gradient is dyadic and S is exact in any order, so both tails form the
    same lr_eff; with it weight decay, the guard and loss scale 2^8"""
    gen = torch.Generator().manual_seed(3)
    Ds = [(torch.randint(-64, 65, s, generator=gen).float() / 16.0).to(_dev()) for s in SHAPES]
    out = []
    for tail in ("torch", "fused"):
        params = _fresh_params(dtype)
        opt = psgd.Kron(params, FORMAT_SETS[1], 1.0, LR, LR_Q, MAX_NORM, 0.0, True, step_tail=tail, generator=_gen(5), momentum=0.5,
                        weight_decay=0.01, nonfinite="skip", loss_scale=2.0 ** 8)
        closure = lambda: sum(torch.sum(p.float() * d) for p, d in zip(params, Ds))
        for _ in range(6):
            opt.step(closure)
        assert opt.skipped_steps == 0
        out.append(_state(params, opt))
    _assert_state(out[1], out[0], "clipped step with everything on, dyadic gradients")
    assert not _bits_equal(out[0]["params"][0], _fresh_params(dtype)[0].detach())


# ------------------------------------------------------------------------------------------------------------ fp64 parity
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_step_against_the_fp64_restatement(psgd, dtype, tail, monkeypatch):
    """One exact-route step through kron_step_f64, fed the gradients, Hessian-vector products and probe vectors the run produced:
    what update_precond_kron and precond_grad_kron were handed, i.e. the T values widened exactly (no loss scale: inv = 1).
    Factors: the 1e-5 bar (relative, norm-wise) of tests/test_kron_class_gpu.py against the same model.
    Parameters: the model's fp64 preconditioned gradient goes through the chain of T roundings, delta = T(lr pg), p' = T(p - delta).
    The bound.  The run's pg is within 1e-5 (relative) of the model's, far below half a spacing of T (2^-9 for bfloat16, 2^-12 for
    float16, relative), so the two lr pg round to the same T value or to neighbours: the deltas differ by at most one spacing of T
    at |delta|, d.  p is the same T value in both, so the exact differences x = p - delta differ by 0 or d.  Let r be the spacing of
    T at the result.  Where d >= r, d is a multiple of r and rounding commutes with the shift: the results differ by d.  Where
    d < r, rounding is monotone and the results are the same grid point or neighbours: they differ by at most r.  Both d and r are
    at most the spacing U of T at max(|p|, |delta|) -- the bound asserted -- as long as the result stays in the binade of the larger
    operand or below, which a descent step (delta has the sign of p on most elements, |delta| < |p|) does; a result that
    carries into the next binade could be 2 U apart and would fail this test.  There is no v on the exact route.  The share of
    elements that differ at all is printed (profiles/kron_class_half.txt records it); it is not bounded."""
    from psgd_tf_amd import kron_optimizer as ko
    params = _fresh_params(dtype, seed=1)
    opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, None, 1.0, True, step_tail=tail, generator=_gen(31))
    closure = _closure(params, seed=1)
    fed = dict(dX=[], dG=[], g=[], pre=[])
    real_u, real_p = ko._psgd.update_precond_kron, ko._psgd.precond_grad_kron

    def update(ql, qr, dX, dG, lr):
        fed["dX"].append(dX.clone())
        fed["dG"].append(dG.clone())
        return real_u(ql, qr, dX, dG, lr)

    def apply(ql, qr, g):
        fed["g"].append(g.clone())
        fed["pre"].append(real_p(ql, qr, g))
        return fed["pre"][-1]
    monkeypatch.setattr(ko._psgd, "update_precond_kron", update)
    monkeypatch.setattr(ko._psgd, "precond_grad_kron", apply)
    p0 = [p.detach().clone() for p in params]
    opt.step(closure)
    n64 = lambda t: t.detach().double().cpu().numpy()
    for name in ("dX", "dG", "g"):                                # fp32 tensors that hold T values: the widening was exact
        assert all(t.dtype == torch.float32 and torch.equal(t, t.to(dtype).float()) for t in fed[name]), name
    lr32 = float(np.float32(LR))
    W64 = [n64(p) for p in p0]
    Q64 = [kc.initial_factors(s, ("dense", "dense")) for s in SHAPES]
    _, Q64, pre64, lr_eff = kc.kron_step_f64(W64, Q64, lambda _: [n64(g) for g in fed["g"]], lambda _: [n64(h) for h in fed["dG"]],
                                             [n64(v) for v in fed["dX"]], lr_params=lr32, lr_preconditioner=float(np.float32(LR_Q)))
    assert lr_eff == lr32
    errs = {"factors": max(kc.rel(n64(q), r) for pair, ref in zip(opt.factors, Q64) for q, r in zip(pair, ref)),
            "pre_grads": max(kc.rel(n64(g), r) for g, r in zip(fed["pre"], pre64))}
    print("%s, %s tail: %s" % (dtype, tail, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) < 1e-5, errs
    differ = total = 0
    eps = torch.finfo(dtype).eps
    for p, q, pg in zip(params, p0, pre64):
        delta = (torch.from_numpy(pg).to(_dev()) * lr32).to(dtype)
        want = q - delta
        big = torch.maximum(q.double().abs(), delta.double().abs())
        # the spacing of T at max(|p|, |delta|): 2^floor(log2(max)) eps (all values here are normal)
        spacing = torch.where(big > 0, 2.0 ** torch.floor(torch.log2(big.clamp_min(1e-300))) * eps, torch.zeros_like(big))
        err = (p.detach().double() - want.double()).abs()
        assert bool((err <= spacing).all()), (float(err.max()), float((err / spacing.clamp_min(1e-300)).max()))
        differ += int((err > 0).sum())
        total += err.numel()
    print("%s, %s tail: %d of %d parameter elements differ from the rounded fp64 model (share %.2e)"
          % (dtype, tail, differ, total, differ / total))


# ------------------------------------------------------------------------------------------------------------------- guard
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("exact", [True, False])
def test_an_fp16_overflow_under_the_loss_scale_skips_the_step(psgd, exact, tail):
    """loss scale 2^16 on gradients with an element of magnitude >= 1: that element is +-Inf in float16 as autograd returns it.
    The step is skipped: factors, momentum buffers and the warm-up counter keep their bits, the parameters too (exact route) or
    are fl16(fl16(p + v) - v) (finite differences); "dynamic" halves the scale until a step has finite gradients and proceeds."""
    dtype = torch.float16
    params, opt, closure = _make(psgd, dtype, tail, exact, formats=FORMAT_SETS[2], momentum=0.9, weight_decay=0.01,
                                 nonfinite="skip", loss_scale="dynamic")
    g = torch.autograd.grad(closure() * 2.0 ** 16, params)
    assert any(bool(torch.isinf(x).any()) for x in g) and not any(bool(torch.isnan(x).any()) for x in g)
    gmax = max(float(x.float().abs().max()) for x in torch.autograd.grad(closure(), params))
    assert 1.0 <= gmax < 2.0 ** 15 and float(opt.loss_scale) == 2.0 ** 16
    before = _state(params, opt)
    twin = torch.Generator(device=_dev())
    twin.set_state(opt._generator.get_state())
    opt.step(closure)
    assert opt.skipped_steps == 1 and opt.last_step_skipped and float(opt.loss_scale) == 2.0 ** 15
    torch.rand((), generator=twin, device=_dev())                                        # the coin, then the probes in T
    vs = [torch.randn(p.shape, dtype=dtype, device=_dev(), generator=twin) for p in params]
    want = dict(before)
    if not exact:
        delta = torch.finfo(dtype).eps ** 0.5
        want["params"] = [(p + v * delta) - v * delta for p, v in zip(before["params"], vs)]
        for p, q in zip(want["params"], before["params"]):                               # one rounding of the p - v undo
            assert float((p.float() - q.float()).abs().max()) <= float(np.spacing(np.float16(q.float().abs().max().item())))
    _assert_state(_state(params, opt), want, "a skipped fp16 step")
    skipped = 1
    while opt.last_step_skipped:
        assert skipped < 17
        scale = float(opt.loss_scale)
        held = _state(params, opt)
        opt.step(closure)
        if opt.last_step_skipped:
            skipped += 1
            assert float(opt.loss_scale) == scale / 2
            if exact:
                _assert_state(_state(params, opt), held, "a further skipped step")
    assert opt.skipped_steps == skipped and float(opt.loss_scale) * gmax < 2.0 ** 16
    assert not _bits_equal(held["params"][0], params[0].detach())                        # the first finite step proceeded
    assert opt._m_step == 1 and all(bool(torch.isfinite(p).all()) for p in params)


@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("exact", [True, False])
def test_a_bf16_loss_scale_changes_no_bit(psgd, exact, tail):
    """bfloat16 has float32's exponent range: times 2^8 nothing overflows and nothing is subnormal here (asserted on the first
    gradients and Hessian-vector products), so scaling by S and by 1 / S is exact and the runs are bit-identical"""
    dtype = torch.bfloat16
    params = _fresh_params(dtype)
    closure = _closure(params)
    fi = torch.finfo(dtype)
    with torch.enable_grad():
        g = torch.autograd.grad(closure(), params, create_graph=True)
        h = torch.autograd.grad(g, params, [torch.ones_like(p) for p in params])
    for x in list(g) + list(h):
        a = x.detach().float().abs()
        assert float(a.max()) * 2.0 ** 8 < fi.max and float(a[a > 0].min()) >= fi.smallest_normal
    kw = dict(momentum=0.9, weight_decay=0.01, nonfinite="skip")
    ref, _ = _run(psgd, dtype, tail, exact, 4, **kw)
    got, opt = _run(psgd, dtype, tail, exact, 4, loss_scale=2.0 ** 8, **kw)
    _assert_state(got, ref, "loss_scale=2^8 against None")
    assert opt.skipped_steps == 0 and float(opt.loss_scale) == 2.0 ** 8


# -------------------------------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("dtype, tail, exact", [(torch.bfloat16, "fused", False), (torch.float16, "fused", True),
                                                (torch.bfloat16, "torch", True)], ids=["bf16-fused-fd", "fp16-fused-exact", "bf16-torch"])
def test_resume_is_bit_identical(psgd, dtype, tail, exact):
    kw = dict(formats=FORMAT_SETS[1], clip=False, seed=4, **ON)
    a, _ = _run(psgd, dtype, tail, exact, 6, **kw)
    pb, ob, cb = _make(psgd, dtype, tail, exact, **kw)
    for _ in range(3):
        ob.step(cb)
    sd = ob.state_dict()
    assert set(sd) == {"format", "kind", "factors", "preconditioner_formats", "param_shapes", "hyper", "rng", "momentum_buffers",
                       "momentum_step", "nonfinite", "skipped_steps", "loss_scale", "loss_scale_good_steps"}      # no new key
    assert all(q.dtype == torch.float32 for pair in sd["factors"] for q in pair)
    assert all(m.dtype == torch.float32 for m in sd["momentum_buffers"])
    saved = [p.detach().clone() for p in pb]
    pc, oc, cc = _make(psgd, dtype, tail, exact, **dict(kw, seed=999))
    oc.step(cc)
    with torch.no_grad():
        for p, s in zip(pc, saved):
            p.copy_(s)
    oc.load_state_dict(sd)
    for _ in range(3):
        oc.step(cc)
    _assert_state(_state(pc, oc), a, "3 + 3 resumed steps against 6")


def test_a_float32_dict_loads_into_a_bfloat16_optimizer_and_back(psgd):
    kw = dict(formats=FORMAT_SETS[0], momentum=0.9)
    p32, o32, c32 = _make(psgd, torch.float32, "fused", True, **kw)
    for _ in range(2):
        o32.step(c32)
    sd = o32.state_dict()
    pb, ob, cb = _make(psgd, torch.bfloat16, "fused", True, seed=77, **kw)
    ob.load_state_dict(sd)
    assert all(_bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]) for a, b in zip(ob.factors, o32.factors))
    assert all(_bits_equal(a, b) for a, b in zip(ob._m, o32._m)) and ob._m_step == 2
    ob.step(cb)
    assert all(p.dtype == torch.bfloat16 and bool(torch.isfinite(p).all()) for p in pb)
    o32.load_state_dict(ob.state_dict())                                                # ... and the other way round
    assert all(_bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]) for a, b in zip(ob.factors, o32.factors))
    o32.step(c32)
    assert all(p.dtype == torch.float32 and bool(torch.isfinite(p).all()) for p in p32)


# ------------------------------------------------------------------------------------------------------------ launch count
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


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_launch_budget_of_the_fused_tail_with_everything_on(psgd, dtype, counting):
    """finite differences, guard, loss scale, momentum, clipping and weight decay together: perturbation 1, widen-check 1,
    difference 1, blend 1, sum of squares 2, update 1 = 7 launches per step whatever the number of layers.  The perturbation and
    the update are both calls of psgd_multi_param_update_t; the fp32 update and the in-place scale-check are never called."""
    params, opt, closure = _make(psgd, dtype, "fused", False, clip=True, **ON)
    for _ in range(3):
        before = collections.Counter(counting.calls)
        opt.step(closure)
        now = collections.Counter(counting.calls)
        now.subtract(before)
        calls = {k: v for k, v in now.items() if k.startswith("psgd_multi_") and v}
        assert calls == {"psgd_multi_param_update_t": 2, "psgd_multi_widen_check": 1, "psgd_multi_diff_scale_f32": 1,
                         "psgd_multi_blend_f32": 1, "psgd_multi_sumsq_f32": 1}, calls
        assert sum(LAUNCHES[k] * v for k, v in calls.items()) == 7
    assert opt.skipped_steps == 0


@pytest.mark.parametrize("exact", [True, False])
def test_a_float32_optimizer_never_calls_the_typed_entry_points(psgd, exact, counting):
    params, opt, closure = _make(psgd, torch.float32, "fused", exact, clip=True, **ON)
    for _ in range(2):
        opt.step(closure)
    assert counting.calls["psgd_multi_param_update_wd_f32"] == 2 and counting.calls["psgd_multi_scale_check_f32"] == 2
    assert not counting.calls["psgd_multi_widen_check"] and not counting.calls["psgd_multi_param_update_t"], dict(counting.calls)
    assert not hasattr(opt, "_wide")
