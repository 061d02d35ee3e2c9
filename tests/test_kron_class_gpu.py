"""class Kron on the GPU: bit for bit against the hand-written reference step (mnist_with_lenet5.py:43-57 with the finite-difference
route of psgd.py:716-727), fused tail against torch tail, parity with the fp64 restatement of tests/kron_class_cases.py, the branches
of the step, resume, a first call on poisoned buffers and a convergence smoke."""
import contextlib
import math

import numpy as np
import pytest
import torch

from tests import kron_class_cases as kc

pytestmark = pytest.mark.gpu

SHAPES = kc.LENET5 + [s for s, _ in kc.SPARSE]
FORMATS = [("dense", "dense")] * len(kc.LENET5) + [f for _, f in kc.SPARSE]
TINY = kc.TINY32
LR, LR_Q, MAX_NORM = 0.05, 0.1, 2.0


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


_problems = {}


def _problem(shapes, seed=0):
    """(Ws, Hls, Hrs) as fp64 NumPy arrays of float32 values and the Hessian factors on the device: made once per shape list"""
    key = (tuple(shapes), seed)
    if key not in _problems:
        Ws, Hls, Hrs = kc.quadratic_problem(shapes, seed)
        f = lambda a: torch.from_numpy(a.astype(np.float32)).to(_dev())
        _problems[key] = (Ws, Hls, Hrs, [f(h) for h in Hls], [f(h) for h in Hrs])
    return _problems[key]


def _fresh_params(Ws):
    return [torch.from_numpy(w.astype(np.float32)).to(_dev()).requires_grad_(True) for w in Ws]


def _quadratic_closure(params, Hl, Hr):
    def closure():
        return sum(0.5 * torch.sum(W * (hl @ W @ hr)) for W, hl, hr in zip(params, Hl, Hr))
    return closure


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _bits_equal(a, b):
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def _assert_same(run_a, run_b, what):
    (pa, qa), (pb, qb) = run_a, run_b
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert _bits_equal(a.detach(), b.detach()), "%s: parameter %d differs" % (what, i)
    for i, (a, b) in enumerate(zip(qa, qb)):
        assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]), "%s: factors of layer %d differ" % (what, i)


def _run_class(psgd, step_tail, exact, clip, layer_batch, steps=3, seed=11, shapes=SHAPES, formats=FORMATS, prob=1.0):
    Ws, _, _, Hl, Hr = _problem(shapes)
    params = _fresh_params(Ws)
    opt = psgd.Kron(params, formats, 1.0, LR, LR_Q, MAX_NORM if clip else None, prob, exact, layer_batch=layer_batch,
                    step_tail=step_tail, generator=_gen(seed))
    closure = _quadratic_closure(params, Hl, Hr)
    for _ in range(steps):
        opt.step(closure)
    return params, opt.factors


def _reference_step(psgd, params, Qs, closure, G, exact, clip, layer_batch, prob=1.0):
    """The hand-written step: the draws of class Kron from G (the coin, then one randn per parameter), the public per-layer
    calls inside the same layer_batch blocks, steps 6-7 in torch."""
    from psgd_tf_amd import kron
    block = kron.layer_batch if layer_batch else contextlib.nullcontext
    update = bool(torch.rand((), generator=G, device=G.device).item() < prob)
    delta = kc.DELTA32
    s = float(np.float32(1.0) / np.float32(delta))
    undo = None
    if update and exact:
        with torch.enable_grad():
            grads = torch.autograd.grad(closure(), params, create_graph=True)
            vs = [torch.randn(p.shape, device=p.device, generator=G) for p in params]
            Hvs = torch.autograd.grad(grads, params, vs)
        grads = [g.detach() for g in grads]
        dXs, dGs = vs, Hvs
    elif update:
        with torch.enable_grad():
            grads = torch.autograd.grad(closure(), params)
        undo = vs = [torch.randn(p.shape, device=p.device, generator=G) * delta for p in params]
        with torch.no_grad():
            for p, v in zip(params, vs):
                p.add_(v)
        with torch.enable_grad():
            perturbed = torch.autograd.grad(closure(), params)
        dGs = [(a - b) * s for a, b in zip(perturbed, grads)]
        dXs = [v * s for v in vs]
    else:
        with torch.enable_grad():
            grads = torch.autograd.grad(closure(), params)
    with torch.no_grad():
        if update:
            with block():
                new = [psgd.update_precond_kron(q[0], q[1], dX, dG, LR_Q) for q, dX, dG in zip(Qs, dXs, dGs)]
            Qs = [[a, b] for a, b in new]
        with block():
            pre = [psgd.precond_grad_kron(q[0], q[1], g) for q, g in zip(Qs, grads)]
        lr = float(np.float32(LR))
        if clip:
            lr = _lr_eff(_sumsq_torch(pre))
        for k, (p, g) in enumerate(zip(params, pre)):
            p.sub_(g * lr if undo is None else g * lr + undo[k])
    return Qs


def _sumsq_torch(pre):
    S = None
    for g in pre:
        s = torch.sum((g * g).double())
        S = s if S is None else S + s
    return S


def _lr_eff(S):
    f64 = lambda x: torch.tensor(float(np.float32(x)), dtype=torch.float64, device=_dev())
    return (f64(LR) * torch.minimum(f64(MAX_NORM) / (torch.sqrt(S) + f64(TINY)), f64(1.0))).float()


_reference_runs = {}


def _run_reference(psgd, exact, clip, layer_batch, steps=3, seed=11):
    """computed once per configuration, shared by the tests of both tails"""
    key = (exact, clip, layer_batch, steps, seed)
    if key not in _reference_runs:
        Ws, _, _, Hl, Hr = _problem(SHAPES)
        params = _fresh_params(Ws)
        Qs = [psgd.kron_initial_factors(s, f, 1.0, _dev()) for s, f in zip(SHAPES, FORMATS)]
        closure = _quadratic_closure(params, Hl, Hr)
        G = _gen(seed)                                 # "a clone of G": the same seed, the same state
        for _ in range(steps):
            Qs = _reference_step(psgd, params, Qs, closure, G, exact, clip, layer_batch)
        _reference_runs[key] = (params, Qs)
    return _reference_runs[key]


CONFIGS = [(exact, clip, lb) for exact in (True, False) for clip in (False, True) for lb in (True, False)]


# ------------------------------------------------------------------------------------------------ equals the hand-written step
@pytest.mark.parametrize("exact, clip, layer_batch", CONFIGS)
def test_torch_tail_equals_the_hand_written_step(psgd, exact, clip, layer_batch):
    ref = _run_reference(psgd, exact, clip, layer_batch)
    got = _run_class(psgd, "torch", exact, clip, layer_batch)
    _assert_same(got, ref, "Kron(step_tail='torch') against the hand-written step")
    assert all(bool(torch.isfinite(p).all()) for p in got[0])


# ------------------------------------------------------------------------------------------------------ fused against torch
@pytest.mark.parametrize("exact, layer_batch", [(e, lb) for e in (True, False) for lb in (True, False)])
def test_fused_tail_without_clipping_is_bit_identical(psgd, exact, layer_batch):
    ref = _run_reference(psgd, exact, False, layer_batch)
    got = _run_class(psgd, "fused", exact, False, layer_batch)
    _assert_same(got, ref, "Kron(step_tail='fused') without clipping")


def _dyadic_run(psgd, step_tail, steps=3):
    """a closure whose gradient is a fixed dyadic tensor, no factor update, identity factors: the preconditioned gradient is that
    tensor and S is exact in any order"""
    gen = torch.Generator().manual_seed(3)
    Ds = [(torch.randint(-64, 65, s, generator=gen).float() / 16.0).to(_dev()) for s in SHAPES]
    Ws, _, _, _, _ = _problem(SHAPES)
    params = _fresh_params(Ws)
    opt = psgd.Kron(params, FORMATS, 1.0, LR, LR_Q, MAX_NORM, 0.0, True, step_tail=step_tail, generator=_gen(5))
    closure = lambda: sum(torch.sum(p * d) for p, d in zip(params, Ds))
    q0 = [[q[0], q[1]] for q in opt.factors]
    for _ in range(steps):
        opt.step(closure)
    assert all(a[0] is b[0] and a[1] is b[1] for a, b in zip(q0, opt.factors))
    return (params, opt.factors), Ds


def test_fused_tail_with_clipping_on_dyadic_gradients_is_bit_identical(psgd):
    a, Ds = _dyadic_run(psgd, "torch")
    b, _ = _dyadic_run(psgd, "fused")
    _assert_same(b, a, "clipped step on dyadic gradients")
    Ws, _, _, _, _ = _problem(SHAPES)
    assert not _bits_equal(a[0][0].detach(), _fresh_params(Ws)[0].detach())          # the parameters did move


@pytest.mark.parametrize("exact", [True, False])
def test_fused_tail_with_clipping_on_random_data(psgd, exact, monkeypatch):
    """step by step: the two S agree within n 2^-53; where the two fl32(lr_eff) are equal the parameters are bit-identical,
    otherwise they differ by at most one ulp of lr_eff times |pg|"""
    from psgd_tf_amd import kron_optimizer as ko
    Ws, _, _, Hl, Hr = _problem(SHAPES)
    n = sum(a * b for a, b in SHAPES)
    runs = {}
    for tail in ("torch", "fused"):
        params = _fresh_params(Ws)
        runs[tail] = (params, psgd.Kron(params, FORMATS, 1.0, LR, LR_Q, MAX_NORM, 1.0, exact, step_tail=tail, generator=_gen(21)),
                      _quadratic_closure(params, Hl, Hr))
    seen = []
    real = ko._psgd.precond_grad_kron
    monkeypatch.setattr(ko._psgd, "precond_grad_kron", lambda *a: seen.append(real(*a)) or seen[-1])
    cases = []
    for step in range(3):
        pre = {}
        for tail in ("torch", "fused"):
            del seen[:]
            runs[tail][1].step(runs[tail][2])
            pre[tail] = [g.clone() for g in seen]
        for a, b in zip(pre["torch"], pre["fused"]):
            assert _bits_equal(a, b)                                               # the same inputs so far: the same gradients
        S_t, S_f = float(_sumsq_torch(pre["torch"])), float(runs["fused"][1]._tail.sumsq[0])
        print("step %d: S torch %.17g, fused %.17g, relative difference %.3e (bound %.3e)"
              % (step, S_t, S_f, abs(S_t - S_f) / S_t, n * 2.0 ** -53))
        assert abs(S_t - S_f) <= n * 2.0 ** -53 * S_t
        lr_t = float(_lr_eff(torch.tensor(S_t, dtype=torch.float64, device=_dev())))
        lr_f = float(_lr_eff(torch.tensor(S_f, dtype=torch.float64, device=_dev())))
        assert lr_t < float(np.float32(LR))                                        # the clip is active
        if lr_t == lr_f:
            cases.append("equal")
            _assert_same((runs["fused"][0], runs["fused"][1].factors), (runs["torch"][0], runs["torch"][1].factors),
                         "clipped step %d with equal lr_eff" % step)
        else:
            cases.append("one ulp")
            ulp = float(np.spacing(np.float32(max(lr_t, lr_f))))
            assert abs(lr_t - lr_f) <= ulp
            for p_t, p_f, g in zip(runs["torch"][0], runs["fused"][0], pre["torch"]):
                assert bool(((p_t.detach().double() - p_f.detach().double()).abs() <= ulp * g.double().abs()).all())
            break                                                                  # (the runs have parted: later steps compare nothing)
    print("lr_eff of the two tails per step: %s" % cases)


# ------------------------------------------------------------------------------------------------------------- oracle parity
PARITY_SHAPES = kc.LENET5 + [(16, 40)]
# The clip of the parity runs: active (the norm of the first preconditioned gradient is about 150) and mild.  The parameters are
# float32: an increment is known only to the rounding of p, about 2^-25 |p| / sqrt(3) per element, so it can be held to 1e-5 of
# its own norm only where it is larger than about 2e-3 |p|; with |p| ~ 0.5 and lr_eff ~ 0.4 * 0.05 the increments here are ~ 1e-2.
PARITY_MAX_NORM = 60.0


@pytest.mark.parametrize("step_tail", ["torch", "fused"])
@pytest.mark.parametrize("clip", [False, True])
def test_parity_with_the_fp64_restatement(psgd, clip, step_tail, monkeypatch):
    """exact Hessian-vector products, the same probe vectors: factors and preconditioned gradients within 1e-5 (relative, norm-wise)
    and the parameter increments p_k - p_0 within 1e-5 of their own norm, after one step and after five.  (The finite-difference
    route is not compared with fp64: its dG carries the cancellation error eps / delta ~ 3e-4 of fp32 differences by design.)"""
    from psgd_tf_amd import kron_optimizer as ko
    Ws, Hls, Hrs, Hl, Hr = _problem(PARITY_SHAPES, seed=1)
    params = _fresh_params(Ws)
    G = _gen(31)
    twin = torch.Generator(device=_dev())
    twin.set_state(G.get_state())
    opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, PARITY_MAX_NORM if clip else None, step_tail=step_tail, generator=G)
    closure = _quadratic_closure(params, Hl, Hr)
    seen = []
    real = ko._psgd.precond_grad_kron
    monkeypatch.setattr(ko._psgd, "precond_grad_kron", lambda *a: seen.append(real(*a)) or seen[-1])
    W64 = [w.copy() for w in Ws]
    Q64 = [kc.initial_factors(s, ("dense", "dense")) for s in PARITY_SHAPES]
    grad_fn = lambda W: kc.quadratic_grads(W, Hls, Hrs)
    hvp_fn = lambda vs: kc.quadratic_grads(vs, Hls, Hrs)
    n64 = lambda t: t.detach().double().cpu().numpy()
    for step in range(1, 6):
        del seen[:]
        opt.step(closure)
        torch.rand((), generator=twin, device=_dev())                                  # the coin
        vs = [n64(torch.randn(s, device=_dev(), generator=twin)) for s in PARITY_SHAPES]
        W64, Q64, pre64, lr_eff = kc.kron_step_f64(W64, Q64, grad_fn, hvp_fn, vs, lr_params=float(np.float32(LR)),
                                                   lr_preconditioner=float(np.float32(LR_Q)),
                                                   max_norm=float(np.float32(PARITY_MAX_NORM)) if clip else None)
        if step in (1, 5):
            if step == 1 or not clip:
                assert (lr_eff < float(np.float32(LR))) == clip                        # the clip, where there is one, is active
            errs = {"factors": max(kc.rel(n64(q), r) for pair, ref in zip(opt.factors, Q64) for q, r in zip(pair, ref)),
                    "pre_grads": max(kc.rel(n64(g), r) for g, r in zip(seen, pre64)),
                    "increments": max(kc.rel(n64(p) - w0, w - w0) for p, w, w0 in zip(params, W64, Ws))}
            print("step %d, clip %s: %s" % (step, clip, {k: "%.2e" % v for k, v in errs.items()}))
            assert max(errs.values()) < 1e-5, (step, errs)


# ------------------------------------------------------------------------------------------------------------------ branches
@pytest.mark.parametrize("step_tail", ["torch", "fused"])
def test_update_probability_zero_and_one(psgd, step_tail):
    shapes, formats = SHAPES[:2] + SHAPES[5:7], FORMATS[:2] + FORMATS[5:7]
    Ws, _, _, Hl, Hr = _problem(shapes)
    params = _fresh_params(Ws)
    opt = psgd.Kron(params, formats, 1.0, LR, LR_Q, None, 0.0, step_tail=step_tail, generator=_gen(1))
    closure = _quadratic_closure(params, Hl, Hr)
    before = [(q[0], q[1], q[0].clone(), q[1].clone()) for q in opt.factors]
    for _ in range(3):
        opt.step(closure)
    for (a, b, a0, b0), q in zip(before, opt.factors):
        assert q[0] is a and q[1] is b and torch.equal(a, a0) and torch.equal(b, b0)       # the same objects, the same bits
    opt.preconditioner_update_probability.assign(1.0)
    for _ in range(2):
        held = [(q[0], q[1]) for q in opt.factors]
        opt.step(closure)
        for (a, b), q in zip(held, opt.factors):
            assert q[0] is not a and q[1] is not b                                          # always rebound, never copied into
            assert q[0].data_ptr() != a.data_ptr() and q[1].data_ptr() != b.data_ptr()


@pytest.mark.parametrize("step_tail", ["torch", "fused"])
def test_finite_difference_route_leaves_no_perturbation(psgd, step_tail):
    """lr_params = 0: the parameters after a step are fl32(fl32(p + v) - v) for the drawn v, the reference's p - v undo"""
    Ws, _, _, Hl, Hr = _problem(SHAPES)
    params = _fresh_params(Ws)
    G = _gen(8)
    twin = torch.Generator(device=_dev())
    twin.set_state(G.get_state())
    opt = psgd.Kron(params, FORMATS, 1.0, 0.0, LR_Q, None, 1.0, False, step_tail=step_tail, generator=G)
    p0 = [p.detach().clone() for p in params]
    opt.step(_quadratic_closure(params, Hl, Hr))
    torch.rand((), generator=twin, device=_dev())
    for p, q in zip(params, p0):
        v = torch.randn(q.shape, device=_dev(), generator=twin) * kc.DELTA32
        want = (q + v) - v                         # the update subtracts fl32(fl32(0 pg) + v) = v for a finite pg
        assert _bits_equal(p.detach(), want)
        assert float((p.detach() - q).abs().max()) <= float(np.spacing(np.float32(q.abs().max().item())))


def test_hyper_assign_takes_effect_on_the_next_step(psgd):
    Ws, _, _, Hl, Hr = _problem(SHAPES[:2])
    outs = []
    for assign in (False, True):
        params = _fresh_params(Ws)
        opt = psgd.Kron(params, "dense", 1.0, LR, LR_Q, None, step_tail="fused", generator=_gen(2))
        closure = _quadratic_closure(params, Hl, Hr)
        opt.step(closure)
        mid = [p.detach().clone() for p in params]
        if assign:
            opt.lr_params.assign(0.0)
            opt.lr_preconditioner.assign(0.5)
        fac = [q[0].clone() for q in opt.factors]
        opt.step(closure)
        outs.append((mid, [p.detach().clone() for p in params], fac, [q[0].clone() for q in opt.factors]))
    (mid_a, end_a, _, fac_a), (mid_b, end_b, _, fac_b) = outs
    assert all(torch.equal(a, b) for a, b in zip(mid_a, mid_b))
    assert all(torch.equal(m, e) for m, e in zip(mid_b, end_b))                    # lr_params = 0: the parameters stand still
    assert not any(torch.equal(m, e) for m, e in zip(mid_a, end_a))
    assert not any(torch.equal(a, b) for a, b in zip(fac_a, fac_b))                # another preconditioner step size


# -------------------------------------------------------------------------------------------------------------------- resume
@pytest.mark.parametrize("step_tail, exact", [("torch", True), ("fused", False)])
def test_resume_is_bit_identical(psgd, step_tail, exact):
    Ws, _, _, Hl, Hr = _problem(SHAPES)

    def make(seed):
        params = _fresh_params(Ws)
        opt = psgd.Kron(params, FORMATS, 1.0, LR, LR_Q, MAX_NORM, 0.7, exact, step_tail=step_tail, generator=_gen(seed))
        return params, opt, _quadratic_closure(params, Hl, Hr)
    pa, oa, ca = make(4)
    for _ in range(4):
        oa.step(ca)
    pb, ob, cb = make(4)
    for _ in range(2):
        ob.step(cb)
    sd = ob.state_dict()
    saved = [p.detach().clone() for p in pb]
    pc, oc, cc = make(999)                                   # a fresh object: other generator state, initial factors
    with torch.no_grad():
        for p, s in zip(pc, saved):
            p.copy_(s)
    oc.lr_params.assign(123.0)
    oc.load_state_dict(sd)
    assert float(oc.lr_params) == float(np.float64(LR))
    for _ in range(2):
        oc.step(cc)
    _assert_same((pc, oc.factors), (pa, oa.factors), "2 + 2 resumed steps against 4")


# ----------------------------------------------------------------------------------------------------------------- first call
@pytest.mark.parametrize("exact", [True, False])
def test_first_fused_step_on_poisoned_buffers(psgd, exact):
    """the workspace of the sum of squares, its result and the outputs of the difference kernel hold 0xFF bytes (NaN) before the first
    fused step: nothing reads them before it writes them"""
    ref = _run_reference(psgd, exact, True, True, steps=2)
    Ws, _, _, Hl, Hr = _problem(SHAPES)
    params = _fresh_params(Ws)
    opt = psgd.Kron(params, FORMATS, 1.0, LR, LR_Q, MAX_NORM, 1.0, exact, step_tail="fused", generator=_gen(11))
    opt._tail.ws.fill_(0xFF)
    opt._tail.sumsq.view(torch.int64).fill_(-1)
    for t in opt._fd_h + opt._fd_x:
        t.view(torch.int32).fill_(-1)
    closure = _quadratic_closure(params, Hl, Hr)
    for _ in range(2):
        opt.step(closure)
    # with clipping the two sums may differ in the last bits; the reference of this test is the torch arithmetic, so compare
    # as test_fused_tail_with_clipping_on_random_data does: equal lr_eff (checked there for this data family) means equal bits
    assert all(bool(torch.isfinite(p).all()) for p in params)
    _assert_same((params, opt.factors), ref, "two fused steps after poisoning")


# --------------------------------------------------------------------------------------------------------------- convergence
def test_convergence_smoke(psgd):
    Ws, Hls, Hrs, Hl, Hr = _problem(kc.LENET5, seed=2)
    params = _fresh_params(Ws)
    opt = psgd.Kron(params, "dense", 1.0, 0.05, 0.1, 10.0, step_tail="fused", generator=_gen(6))
    closure = _quadratic_closure(params, Hl, Hr)
    loss0 = float(closure().detach())
    for _ in range(200):
        opt.step(closure)
    loss1 = float(closure().detach())
    print("quadratic on the LeNet5 shapes: loss %.4e -> %.4e after 200 fused-tail steps" % (loss0, loss1))
    assert math.isfinite(loss1) and loss1 < loss0
    assert all(bool(torch.isfinite(p).all()) for p in params)
    assert all(bool(torch.isfinite(q).all()) for pair in opt.factors for q in pair)
