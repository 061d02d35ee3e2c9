"""Kron(any_rank=True) on the GPU, on the parameters of a small module: a conv 3 x 3 x 3 x 4 kernel and its bias, a 12 x 7 linear
layer and its bias, and the two vectors of a LayerNorm of length 7.  Five steps against the fp64 oracle applied per layer on the same
coin and perturbations, for both vector routes and both step tails; everything on in bfloat16 with the two tails bit for bit; a
guarded step that changes nothing; resume."""
import numpy as np
import pytest
import torch

from tests import kron_class_cases as kc

pytestmark = pytest.mark.gpu

SHAPES = [(4, 3, 3, 3), (4,), (12, 7), (12,), (7,), (7,)]            # conv kernel, conv bias, linear, its bias, LayerNorm weight, bias
LAYER_SHAPES = [(4, 27), (1, 4), (12, 7), (1, 12), (1, 7), (1, 7)]
LAYER_FORMATS = [("dense", "dense"), ("dense", "scale")] * 2 + [("dense", "scale")] * 2
LR, LR_Q, MAX_NORM, PROB = 0.05, 0.1, 1.0, 0.7
BATCH = 5


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


_data = {}


def _problem():
    """the data of the module as float32 values held in fp64 on the CPU: initial parameters, the unfolded 3 x 3 patches of a batch of
    3 x 6 x 6 inputs (the convolution is then one product with the folded kernel), a fixed 64 -> 7 projection and the targets"""
    if not _data:
        rng = np.random.default_rng(0)
        f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32).astype(np.float64))
        x = torch.from_numpy(rng.standard_normal((BATCH, 3, 6, 6)))
        _data["cols"] = f32(torch.nn.functional.unfold(x, 3).numpy())                          # [B, 27, 16]
        _data["proj"] = f32(rng.standard_normal((64, 7)) / 8.0)
        _data["target"] = f32(rng.standard_normal((BATCH, 12)))
        scales = (0.3, 0.2, 0.4, 0.2, 0.3, 0.2)
        _data["params"] = [f32(rng.standard_normal(s) * c + (1.0 if i == 4 else 0.0)) for i, (s, c) in enumerate(zip(SHAPES, scales))]
    return _data


def _loss(params, data):
    """conv (as a product with the unfolded patches) + bias, tanh, projection, LayerNorm, linear + bias, tanh, squared error"""
    Wc, bc, W, b, ln_w, ln_b = params
    h = torch.tanh(torch.einsum("ok,bkl->bol", Wc.reshape(4, 27), data["cols"]) + bc[None, :, None])      # [B, 4, 16]
    h = h.reshape(h.shape[0], 64) @ data["proj"]                                                            # [B, 7]
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    h = (h - mu) / torch.sqrt(var + 1e-5) * ln_w + ln_b
    y = torch.tanh(h @ W.t() + b)
    return 0.5 * torch.sum((y - data["target"]) ** 2) / BATCH


def _device_setup(dtype=torch.float32):
    d = _problem()
    data = {k: d[k].to(_dev(), dtype) for k in ("cols", "proj", "target")}
    params = [p.to(_dev(), dtype).requires_grad_(True) for p in d["params"]]
    return params, data


_reference = {}
_seeds = {}


def _seed_with_both_branches(steps, first=31):
    """the first seed from `first` on whose coins over `steps` steps, drawn as class Kron draws them (the coin, then one randn per
    parameter on a step that updates), come out both ways"""
    if steps not in _seeds:
        seed = first
        while True:
            G, coins = _gen(seed), []
            for _ in range(steps):
                coins.append(bool(torch.rand((), generator=G, device=_dev()).item() < PROB))
                if coins[-1]:
                    for s in SHAPES:
                        torch.randn(s, device=_dev(), generator=G)
            if any(coins) and not all(coins):
                break
            seed += 1
        _seeds[steps] = seed
    return _seeds[steps]


def _fp64_trajectory(seed, steps, clip):
    """the hand-written loop: the coin and the probe vectors drawn as class Kron draws them from a device generator of this seed,
    gradients and Hessian-vector products by autograd in fp64, the oracle per layer (kc.kron_step_f64).  Made once per key."""
    key = (seed, steps, clip)
    if key in _reference:
        return _reference[key]
    d = _problem()
    G = _gen(seed)
    to_params = lambda Ws: [torch.from_numpy(np.ascontiguousarray(w)).reshape(s).requires_grad_(True) for w, s in zip(Ws, SHAPES)]
    to_layers = lambda ts: [t.detach().numpy().reshape(s).copy() for t, s in zip(ts, LAYER_SHAPES)]
    holder = {}

    def grad_fn(Ws):
        ps = to_params(Ws)
        return to_layers(torch.autograd.grad(_loss(ps, d), ps))

    def hvp_fn(vs):
        ps = to_params(holder["W"])
        grads = torch.autograd.grad(_loss(ps, d), ps, create_graph=True)
        return to_layers(torch.autograd.grad(grads, ps, [torch.from_numpy(v).reshape(s) for v, s in zip(vs, SHAPES)]))
    Ws = to_layers(d["params"])
    Qs = [kc.initial_factors(s, f) for s, f in zip(LAYER_SHAPES, LAYER_FORMATS)]
    updates = []
    for _ in range(steps):
        update = bool(torch.rand((), generator=G, device=_dev()).item() < PROB)
        updates.append(update)
        vs = None
        if update:
            vs = [torch.randn(s, device=_dev(), generator=G).double().cpu().numpy().reshape(ls) for s, ls in zip(SHAPES, LAYER_SHAPES)]
        holder["W"] = Ws
        Ws, Qs, _, _ = kc.kron_step_f64(Ws, Qs, grad_fn, hvp_fn, vs, lr_params=float(np.float32(LR)),
                                        lr_preconditioner=float(np.float32(LR_Q)),
                                        max_norm=float(np.float32(MAX_NORM)) if clip else None, update=update)
    _reference[key] = (Ws, Qs, updates)
    return _reference[key]


def _bits_equal(a, b):
    a, b = a.detach(), b.detach()
    if a.dtype != torch.float32:
        return bool((a.view(torch.int16) == b.view(torch.int16)).all())
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _assert_same(opt_a, params_a, opt_b, params_b, what):
    for i, (a, b) in enumerate(zip(params_a, params_b)):
        assert _bits_equal(a, b), "%s: parameter %d differs" % (what, i)
    for i, (a, b) in enumerate(zip(opt_a.factors, opt_b.factors)):
        assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]), "%s: factors of layer %d differ" % (what, i)
    if opt_a._m is not None or opt_b._m is not None:
        for i, (a, b) in enumerate(zip(opt_a._m, opt_b._m)):
            assert _bits_equal(a, b), "%s: momentum buffer %d differs" % (what, i)


# ------------------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("step_tail", ["torch", "fused"])
@pytest.mark.parametrize("vector_route", ["list", "layer"])
def test_five_steps_against_the_fp64_oracle_per_layer(psgd, vector_route, step_tail):
    """parameters and all factors within 1e-5 (relative, norm-wise) of the hand-written fp64 loop after five steps with a clipped
    update and a coin of probability 0.7"""
    steps = 5
    seed = _seed_with_both_branches(steps)
    W64, Q64, updates = _fp64_trajectory(seed, steps, True)
    assert any(updates) and not all(updates)                                       # both branches of the coin ran
    params, data = _device_setup()
    opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, MAX_NORM, PROB, True, step_tail=step_tail, generator=_gen(seed), any_rank=True,
                    vector_route=vector_route)
    assert [tuple(q.shape) for q in opt.factors[1]] == [(1, 1), (1, 4)] and [tuple(q.shape) for q in opt.factors[0]] == [(4, 4), (27, 27)]
    held = [(q[0], q[1]) for q in opt.factors]
    for _ in range(steps):
        opt.step(lambda: _loss(params, data))
    n64 = lambda t: t.detach().double().cpu().numpy()
    e_par = [kc.rel(n64(p).reshape(ls), w) for p, w, ls in zip(params, W64, LAYER_SHAPES)]
    e_fac = [max(kc.rel(n64(q[0]), r[0]), kc.rel(n64(q[1]), r[1])) for q, r in zip(opt.factors, Q64)]
    print("%s / %s: parameters %s, factors %s" % (vector_route, step_tail, ["%.1e" % e for e in e_par], ["%.1e" % e for e in e_fac]))
    assert max(e_par) < 1e-5 and max(e_fac) < 1e-5, (e_par, e_fac)
    assert [tuple(p.shape) for p in params] == SHAPES and all(p.is_leaf for p in params)
    # the list route updates the vector factors in place; every other factor is rebound, as it always was
    for i, (a, b) in enumerate(held):
        in_place = vector_route == "list" and len(SHAPES[i]) == 1
        assert (opt.factors[i][0] is a and opt.factors[i][1] is b) == in_place, i
    sd = opt.state_dict()
    assert sd["param_shapes"] == [list(s) for s in SHAPES] and sd["preconditioner_formats"] == [list(f) for f in LAYER_FORMATS]


@pytest.mark.parametrize("step_tail", ["torch", "fused"])
def test_finite_difference_route_and_the_two_vector_routes(psgd, step_tail):
    """finite-difference products, no clipping, a rank-0 parameter included: the list route and the layer route end within 1e-3 of
    each other.  They round differently, and the fp64 oracle is not the reference of this route: dG = (g' - g) / delta carries the
    rounding of g' and g, eps / delta ~ 3e-4 of its size, as noise that depends on the last bits of the parameters.  Two runs whose
    parameters differ in those bits therefore see pairs that differ by ~3e-4, their factors part by lr_preconditioner * 3e-4 = 3e-5
    a step, 1e-4 after three steps; the bar is ten times that."""
    runs = []
    for route in ("list", "layer"):
        params, data = _device_setup()
        extra = torch.full((), 0.5, device=_dev(), requires_grad=True)            # a rank-0 parameter: a [1, 1] layer
        opt = psgd.Kron(params + [extra], "dense", 1.0, LR, LR_Q, None, 1.0, False, step_tail=step_tail, generator=_gen(5),
                        any_rank=True, vector_route=route)
        for _ in range(3):
            opt.step(lambda: _loss(params, data) + 0.5 * (extra - 1.0) ** 2)
        assert [tuple(q.shape) for q in opt.factors[-1]] == [(1, 1), (1, 1)]
        runs.append((params + [extra], opt))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert bool(torch.isfinite(a).all()) and kc.rel(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 1e-3
    for qa, qb in zip(runs[0][1].factors, runs[1][1].factors):
        assert all(kc.rel(x.cpu().numpy(), y.cpu().numpy()) < 1e-3 for x, y in zip(qa, qb))
    assert float((runs[0][0][-1].detach() - 0.5).abs()) > 1e-3                     # the scalar moved


# -------------------------------------------------------------------------------------------------------------- every switch
def _everything_on(psgd, step_tail, exact, steps=4, dtype=torch.bfloat16, seed=17):
    params, data = _device_setup(dtype)
    opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, None, PROB, exact, step_tail=step_tail, generator=_gen(seed), any_rank=True,
                    momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale=2.0 ** 8)
    for _ in range(steps):
        opt.step(lambda: _loss(params, data).float())
    return params, opt


@pytest.mark.parametrize("exact", [True, False])
def test_everything_on_in_bfloat16_both_tails_bit_for_bit(psgd, exact):
    pa, oa = _everything_on(psgd, "torch", exact)
    pb, ob = _everything_on(psgd, "fused", exact)
    _assert_same(oa, pa, ob, pb, "momentum, weight decay, guard and loss scale in bfloat16, torch tail against fused tail")
    assert oa.skipped_steps == ob.skipped_steps == 0
    d = _problem()
    assert all(p.dtype == torch.bfloat16 and bool(torch.isfinite(p).all()) for p in pa)
    assert any(not torch.equal(p.detach().cpu(), q.to(torch.bfloat16)) for p, q in zip(pa, d["params"]))      # the parameters moved
    assert all(q.dtype == torch.float32 for pair in oa.factors for q in pair)


@pytest.mark.parametrize("step_tail", ["torch", "fused"])
def test_guarded_step_with_an_inf_bias_gradient_changes_nothing(psgd, step_tail):
    params, data = _device_setup()
    opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, MAX_NORM, 1.0, True, step_tail=step_tail, generator=_gen(3), any_rank=True,
                    momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale=2.0 ** 8)
    for _ in range(2):
        opt.step(lambda: _loss(params, data))
    before = ([p.detach().clone() for p in params], [[q.clone() for q in pair] for pair in opt.factors], [m.clone() for m in opt._m])
    held = [(q[0], q[1]) for q in opt.factors]
    opt.step(lambda: _loss(params, data) + params[3][0] * float("inf"))           # the gradient of one bias element is Inf
    assert opt.last_step_skipped and opt.skipped_steps == 1
    assert all(_bits_equal(p, q) for p, q in zip(params, before[0]))
    assert all(a[0] is b[0] and a[1] is b[1] for a, b in zip(opt.factors, held))
    assert all(_bits_equal(x, y) for pa, pb in zip(opt.factors, before[1]) for x, y in zip(pa, pb))
    assert all(_bits_equal(m, n) for m, n in zip(opt._m, before[2]))
    opt.step(lambda: _loss(params, data))                                          # ... and the next step is an ordinary one
    assert not opt.last_step_skipped and not _bits_equal(opt.factors[1][1], before[1][1][1])


# -------------------------------------------------------------------------------------------------------------------- resume
@pytest.mark.parametrize("step_tail, exact", [("torch", True), ("fused", False)])
def test_resume_is_bit_identical(psgd, step_tail, exact):
    def make(seed):
        params, data = _device_setup()
        opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, MAX_NORM, PROB, exact, step_tail=step_tail, generator=_gen(seed),
                        any_rank=True, momentum=0.5)
        return params, opt, (lambda: _loss(params, data))
    pa, oa, ca = make(4)
    for _ in range(4):
        oa.step(ca)
    pb, ob, cb = make(4)
    for _ in range(2):
        ob.step(cb)
    sd = ob.state_dict()
    assert [tuple(q.shape) for q in sd["factors"][4]] == [(1, 1), (1, 7)] and sd["factors"][4][1].device.type == "cpu"
    saved = [p.detach().clone() for p in pb]
    pc, oc, cc = make(999)                                   # a fresh object: other generator state, initial factors
    with torch.no_grad():
        for p, s in zip(pc, saved):
            p.copy_(s)
    oc.load_state_dict(sd)
    for _ in range(2):
        oc.step(cc)
    _assert_same(oc, pc, oa, pa, "2 + 2 resumed steps against 4")
    # an optimizer of other shapes refuses the checkpoint
    other = [torch.zeros(s, device=_dev(), requires_grad=True) for s in SHAPES[:5] + [(8,)]]
    with pytest.raises(ValueError, match="param_shapes"):
        psgd.Kron(other, any_rank=True).load_state_dict(sd)
