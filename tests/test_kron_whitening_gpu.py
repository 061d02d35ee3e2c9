"""Kron(preconditioner_fit="whitening") on the GPU: a closure that cannot be differentiated twice trains; the class against a
hand-written sequence of the public calls, bit for bit, on both step tails; parity with the fp64 oracle fed counter_randn's probe;
every switch of the class once, fused tail against torch tail; the guard; resume; the default path untouched."""
import numpy as np
import pytest
import torch
from torch.autograd.function import once_differentiable

from oracle import psgd_oracle as orc
from tests import kron_class_cases as kc

pytestmark = pytest.mark.gpu

SHAPES = kc.LENET5 + [s for s, _ in kc.SPARSE]                     # the LeNet5 set and the mixed-format set: all seven formats
FORMATS = [("dense", "dense")] * len(kc.LENET5) + [f for _, f in kc.SPARSE]
LR, LR_Q, MAX_NORM = 0.01, 0.1, 2.0
SEED0 = 0x5EED


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


_data = {}


def _problem(shapes):
    """per parameter: the initial value W, the Hessian factors Hl, Hr of the quadratic term (rank 2) or its diagonal a (any other
    rank, also the weights of the tanh term); float32 device tensors, made once per shape list"""
    key = tuple(shapes)
    if key not in _data:
        rng = np.random.default_rng(2026)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())
        d = {"W": [], "Hl": [], "Hr": [], "a": []}
        for s in shapes:
            d["W"].append(f(rng.standard_normal(s) * 0.5))
            d["Hl"].append(f(kc.spd(s[0], rng)) if len(s) == 2 else None)
            d["Hr"].append(f(kc.spd(s[1], rng)) if len(s) == 2 else None)
            d["a"].append(f(np.exp(rng.uniform(-1.0, 1.0, s))))
        _data[key] = d
    return _data[key]


def _fresh_params(shapes, dtype=torch.float32):
    return [w.clone().to(dtype).requires_grad_(True) for w in _problem(shapes)["W"]]


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


def _closure(params, shapes, once=False, calls=None):
    """the fixed quadratic-plus-tanh loss, computed in float32 whatever the parameters' dtype.  once: the tanh is the
    once_differentiable Function and the quadratic term is left out, so that every gradient comes out of that Function's backward
    alone -- the case in which the second autograd.grad of the exact route has no graph to walk and raises.  (Where a parameter
    reaches its gradient on another path too, torch.autograd.grad walks that path alone and silently leaves the Function's
    curvature out: no error, a wrong Hessian-vector product.)"""
    d = _problem(shapes)
    tanh = _OnceTanh.apply if once else torch.tanh

    def closure():
        if calls is not None:
            calls.append(1)
        loss = 0.0
        for p, hl, hr, a in zip(params, d["Hl"], d["Hr"], d["a"]):
            W = p.float()
            if once:
                quad = 0.0
            else:
                quad = 0.5 * torch.sum(W * (hl @ W @ hr)) if hl is not None else 0.5 * torch.sum(a * W * W)
            loss = loss + quad + 0.25 * torch.sum(a * tanh(W) ** 2)
        return loss
    return closure


def _bits_equal(a, b):
    a, b = a.detach(), b.detach()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    a, b = a.contiguous(), b.contiguous()
    return bool(((a.view(view) == b.view(view)) | (torch.isnan(a) & torch.isnan(b))).all())


def _state(params, opt):
    return {"params": [p.detach().clone() for p in params], "factors": [[q.clone() for q in pair] for pair in opt.factors],
            "momentum": None if opt._m is None else [m.clone() for m in opt._m], "m_step": opt._m_step,
            "probe_step": opt.probe_step, "skipped": opt.skipped_steps}


def _assert_state(a, b, what):
    for k in ("params", "momentum"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        for i, (x, y) in enumerate(zip(a[k] or (), b[k] or ())):
            assert _bits_equal(x, y), "%s: %s %d differs" % (what, k, i)
    for i, (x, y) in enumerate(zip(a["factors"], b["factors"])):
        assert _bits_equal(x[0], y[0]) and _bits_equal(x[1], y[1]), "%s: factors of layer %d differ" % (what, i)
    assert (a["m_step"], a["probe_step"]) == (b["m_step"], b["probe_step"]), what


def _make(psgd, tail, *, shapes=SHAPES, formats=FORMATS, dtype=torch.float32, clip=False, prob=1.0, seed=11, once=False, calls=None,
          fit="whitening", **kw):
    params = _fresh_params(shapes, dtype)
    if fit is not None:
        kw = dict(kw, preconditioner_fit=fit)
        if fit == "whitening":
            kw.setdefault("probe_seed", SEED0)
    opt = psgd.Kron(params, formats, 1.0, LR, LR_Q, MAX_NORM if clip else None, prob, True, step_tail=tail, generator=_gen(seed), **kw)
    return params, opt, _closure(params, shapes, once, calls)


def _run(psgd, tail, steps, **kw):
    params, opt, closure = _make(psgd, tail, **kw)
    for _ in range(steps):
        opt.step(closure)
    return _state(params, opt), opt


# ---------------------------------------------------------------------------------------------------------- the feature itself
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_a_once_differentiable_closure_trains_with_one_closure_call_per_step(psgd, tail):
    calls = []
    params, opt, closure = _make(psgd, tail, once=True, calls=calls)
    losses = []
    for k in range(5):
        losses.append(float(opt.step(closure).detach()))
        assert len(calls) == k + 1                                       # exactly one closure call per step
    assert opt.probe_step == 5 and all(bool(torch.isfinite(p).all()) for p in params)
    assert losses[-1] < losses[0]
    # the same closure on the exact Hessian-vector route cannot be differentiated a second time
    params, opt, closure = _make(psgd, tail, once=True, fit="hessian")
    with pytest.raises(RuntimeError):                                    # (the text is autograd's and differs between versions)
        opt.step(closure)


# ------------------------------------------------------------------------------------------ against a hand-written sequence
_hand = {}


def _hand_written(psgd, prob, steps=10, seed=11):
    """one multi_randn, per-layer update_precond_kron(Ql, Qr, v, g), precond_grad_kron, multi_param_update; the coin drawn as the
    class draws it.  Computed once per probability, shared by the tests of both tails."""
    if prob not in _hand:
        from psgd_tf_amd import kron
        params = _fresh_params(SHAPES)
        closure = _closure(params, SHAPES)
        Qs = [psgd.kron_initial_factors(s, f, 1.0, _dev()) for s, f in zip(SHAPES, FORMATS)]
        vs = [torch.empty_like(p, requires_grad=False) for p in params]
        G, k = _gen(seed), 0
        for _ in range(steps):
            update = bool(torch.rand((), generator=G, device=_dev()).item() < prob)
            with torch.enable_grad():
                grads = torch.autograd.grad(closure(), params)
            with torch.no_grad():
                if update:
                    psgd.multi_randn(vs, psgd.uvd_step_rounding_seed(SEED0, k))
                    k += 1
                    with kron.layer_batch():
                        Qs = [list(psgd.update_precond_kron(q[0], q[1], v, g, LR_Q)) for q, v, g in zip(Qs, vs, grads)]
                with kron.layer_batch():
                    pre = [psgd.precond_grad_kron(q[0], q[1], g) for q, g in zip(Qs, grads)]
                psgd.multi_param_update(params, [g.contiguous() for g in pre], None, LR)      # (mirrored formats: transposed views)
        _hand[prob] = ({"params": [p.detach().clone() for p in params], "factors": Qs, "momentum": None, "m_step": 0,
                        "probe_step": k, "skipped": 0}, k)
    return _hand[prob]


@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("prob", [1.0, 0.5])
def test_class_equals_the_hand_written_sequence(psgd, prob, tail):
    want, updates = _hand_written(psgd, prob)
    got, opt = _run(psgd, tail, 10, prob=prob)
    assert opt.probe_step == updates                                     # the counter advances on updating steps only
    assert updates == 10 if prob == 1.0 else 0 < updates < 10
    _assert_state(got, want, "Kron(whitening, step_tail=%r, p=%g) against the hand-written sequence" % (tail, prob))
    assert all(bool(torch.isfinite(p).all()) for p in got["params"])


def test_tails_agree_with_clipping_on_dyadic_gradients(psgd):
    """as the class tests construct it: a fixed dyadic gradient, identity factors, no factor update -- S is exact in any order"""
    gen = torch.Generator().manual_seed(3)
    Ds = [(torch.randint(-64, 65, s, generator=gen).float() / 16.0).to(_dev()) for s in SHAPES]
    out = []
    for tail in ("torch", "fused"):
        params, opt, _ = _make(psgd, tail, clip=True, prob=0.0)
        closure = lambda: sum(torch.sum(p * d) for p, d in zip(params, Ds))
        for _ in range(3):
            opt.step(closure)
        assert opt.probe_step == 0
        out.append(_state(params, opt))
    _assert_state(out[1], out[0], "clipped whitening step on dyadic gradients")
    assert not _bits_equal(out[0]["params"][0], _fresh_params(SHAPES)[0])


# ------------------------------------------------------------------------------------------------------------- oracle parity
def test_parity_with_the_fp64_oracle_fed_counter_randn(psgd, monkeypatch):
    """20 steps on the LeNet5 set: the oracle's update_precond_kron / precond_grad_kron in fp64 on the CPU, fed counter_randn's v
    and the gradients of the GPU run; factors and preconditioned gradients within 1e-5, relative and norm-wise.  The kernel's
    probe differs from counter_randn's by a few 1e-7 per element (profiles/kron_whitening.txt), far below that bar."""
    from psgd_tf_amd import kron_optimizer as ko
    shapes = kc.LENET5
    params, opt, closure = _make(psgd, "fused", shapes=shapes, formats="dense")
    seen = []
    real = ko._psgd.precond_grad_kron
    monkeypatch.setattr(ko._psgd, "precond_grad_kron", lambda *a: seen.append(real(*a)) or seen[-1])
    n64 = lambda t: t.detach().double().cpu().numpy()
    Q64 = [kc.initial_factors(s, ("dense", "dense")) for s in shapes]
    sizes = [a * b for a, b in shapes]
    worst = {"factors": 0.0, "pre_grads": 0.0}
    for step in range(20):
        with torch.enable_grad():
            g64 = [n64(g) for g in torch.autograd.grad(closure(), params)]          # the gradients the step is about to take
        del seen[:]
        opt.step(closure)
        flat = psgd.counter_randn(psgd.uvd_step_rounding_seed(SEED0, step), 0, sum(sizes)).astype(np.float64)
        vs = [v.reshape(s) for v, s in zip(np.split(flat, np.cumsum(sizes)[:-1]), shapes)]
        Q64 = [list(orc.update_precond_kron(q[0], q[1], v, g, float(np.float32(LR_Q)))) for q, v, g in zip(Q64, vs, g64)]
        pre64 = [orc.precond_grad_kron(q[0], q[1], g) for q, g in zip(Q64, g64)]
        errs = {"factors": max(kc.rel(n64(q), r) for pair, ref in zip(opt.factors, Q64) for q, r in zip(pair, ref)),
                "pre_grads": max(kc.rel(n64(g), r) for g, r in zip(seen, pre64))}
        worst = {k: max(worst[k], errs[k]) for k in worst}
    print("20 steps: worst relative error %s" % {k: "%.2e" % v for k, v in worst.items()})
    assert opt.probe_step == 20
    assert max(worst.values()) < 1e-5, worst


# ----------------------------------------------------------------------------------------------- every switch, fused == torch
ANY_RANK_SHAPES = [(4, 3, 3, 3), (4,), (12, 7), (12,), (7,), (16, 12)]         # a rank-4 kernel, vectors, matrices
SWITCHES = {
    "bfloat16": dict(dtype=torch.bfloat16),
    "float16": dict(dtype=torch.float16),
    "momentum and weight decay": dict(momentum=0.9, weight_decay=0.01),
    "stochastic parameter rounding": dict(dtype=torch.bfloat16, param_rounding="stochastic", param_rounding_seed=5),
    "any_rank, vectors on the list route": dict(shapes=ANY_RANK_SHAPES, formats="dense", any_rank=True, vector_route="list"),
    "any_rank, vectors on the layer route": dict(shapes=ANY_RANK_SHAPES, formats="dense", any_rank=True, vector_route="layer"),
    "bf16 operands": dict(shapes=ANY_RANK_SHAPES, formats="dense", any_rank=True, operands="bfloat16", operand_min_dim=8),
}


@pytest.mark.parametrize("name", list(SWITCHES))
def test_every_switch_fused_tail_equals_torch_tail(psgd, name):
    kw = SWITCHES[name]
    a, oa = _run(psgd, "torch", 3, **kw)
    b, ob = _run(psgd, "fused", 3, **kw)
    _assert_state(b, a, "whitening with %s" % name)
    assert oa.probe_step == ob.probe_step == 3
    assert all(bool(torch.isfinite(p.float()).all()) for p in a["params"])
    if "operands" in kw:
        assert ob.operand_layers == [5]                                 # the 16 x 12 layer qualifies at operand_min_dim=8
    shapes = kw.get("shapes", SHAPES)
    assert not _bits_equal(a["params"][0], _fresh_params(shapes, kw.get("dtype", torch.float32))[0])


# -------------------------------------------------------------------------------------------------------------------- guard
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_a_skipped_step_changes_nothing_and_keeps_its_probe_stream(psgd, tail):
    """an Inf in one gradient on step 3: factors, parameters, momentum buffers and probe_step keep their bits, skipped_steps
    counts, and the next step draws the stream the skipped one would have drawn -- the run equals one without the bad step"""
    kw = dict(nonfinite="skip", loss_scale=2.0 ** 8, momentum=0.5)
    params, opt, good = _make(psgd, tail, **kw)
    bad = lambda: good() + params[1].sum() * float("inf")
    for _ in range(2):
        opt.step(good)
    before = _state(params, opt)
    opt.step(bad)
    assert opt.last_step_skipped and opt.skipped_steps == 1 and opt.probe_step == 2
    _assert_state(_state(params, opt), before, "a skipped whitening step")
    opt.step(good)
    assert not opt.last_step_skipped and opt.probe_step == 3
    want, _ = _run(psgd, tail, 3, **kw)                                  # three good steps: probe streams 0, 1, 2
    _assert_state(_state(params, opt), want, "the step after a skipped one")


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_the_loss_scale_does_not_move_a_bit_of_a_float32_run(psgd, tail):
    a, _ = _run(psgd, tail, 4)
    b, ob = _run(psgd, tail, 4, nonfinite="skip", loss_scale=2.0 ** 8)
    assert ob.skipped_steps == 0
    _assert_state(b, a, "float32 whitening run with loss_scale 2^8")


# --------------------------------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_resume_is_bit_identical(psgd, tail):
    kw = dict(prob=0.7, momentum=0.9)
    want, _ = _run(psgd, tail, 8, **kw)
    params, opt, closure = _make(psgd, tail, **kw)
    for _ in range(4):
        opt.step(closure)
    sd = opt.state_dict()
    assert sd["probe_seed0"] == SEED0 and sd["probe_step"] == opt.probe_step and "preconditioner_fit" not in sd["hyper"]
    saved = [p.detach().clone() for p in params]
    p2, o2, c2 = _make(psgd, tail, **dict(kw, seed=999, probe_seed=1))    # another generator state, another probe seed
    with torch.no_grad():
        for p, s in zip(p2, saved):
            p.copy_(s)
    o2.load_state_dict(sd)
    assert o2.probe_seed0 == SEED0 and o2.probe_step == sd["probe_step"]
    for _ in range(4):
        o2.step(c2)
    _assert_state(_state(p2, o2), want, "4 + 4 steps against 8")


def test_a_hessian_fit_dict_loads_into_a_whitening_optimizer(psgd):
    ph, oh, ch = _make(psgd, "fused", fit="hessian")
    oh.step(ch)
    sd = oh.state_dict()
    assert "probe_seed0" not in sd and "probe_step" not in sd
    pw, ow, cw = _make(psgd, "fused")
    ow.step(cw)
    assert ow.probe_step == 1
    ow.load_state_dict(sd)
    assert ow.probe_seed0 == SEED0 and ow.probe_step == 0               # the seed is kept, the counter starts again
    for a, b in zip(ow.factors, oh.factors):
        assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])
    oh.load_state_dict(ow.state_dict())                                  # ... and a hessian-fit optimizer ignores the keys
    assert oh.probe_seed0 is None and oh.probe_step == 0


def test_the_probe_seed_is_drawn_from_the_generator_behind_the_coin(psgd):
    seeds = []
    for _ in range(2):
        params = _fresh_params(kc.LENET5[:1])
        seeds.append(psgd.Kron(params, "dense", generator=_gen(4), preconditioner_fit="whitening").probe_seed0)
    twin = _gen(4)
    assert seeds[0] == seeds[1] == int(torch.randint(0, 2 ** 62, (), generator=twin, device=_dev()).item())


# ---------------------------------------------------------------------------------------------------- default path untouched
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_hessian_spelled_out_is_the_default_bit_for_bit(psgd, tail, monkeypatch):
    from psgd_tf_amd import kron_optimizer as ko
    called = []
    real = ko.multi_randn
    monkeypatch.setattr(ko, "multi_randn", lambda *a, **k: called.append(1) or real(*a, **k))
    a, oa = _run(psgd, tail, 5, fit=None, clip=True)
    b, ob = _run(psgd, tail, 5, fit="hessian", clip=True)
    _assert_state(b, a, "preconditioner_fit='hessian' against the default")
    assert not called and oa.probe_seed0 is None and ob.probe_seed0 is None and oa._probe is None
    assert torch.equal(oa.state_dict()["rng"], ob.state_dict()["rng"])


# ------------------------------------------------------------------------------------------------------------------ example
def test_the_example_trains_and_reports_the_error_of_the_exact_route():
    """examples/kron_whitening.py, 60 steps: the exact route raises on the once_differentiable activation, whitening trains"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "kron_whitening.py")
    spec = importlib.util.spec_from_file_location("kron_whitening_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    error, first, last = mod.main(60)
    assert error is not None
    assert np.isfinite(last) and last < first
