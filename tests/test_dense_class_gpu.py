"""class Dense on the GPU: bit for bit against the loop a user writes by hand from update_precond_dense / precond_grad_dense
(demo_usage_of_all_preconditioners.py:30-41 with the step tail of psgd.py:750-762), fused tail against torch tail, a 20-step
trajectory against the fp64 oracle, the allocation condition, the two buffers of Q, a first call on poisoned buffers, every
switch of the shared step-feature layer, the whitening fit, resume, and hello_psgd.py's Rosenbrock run.

Parameter sets, named by their total N, chosen for the edges of the kernels of psgd_dense.hip:

    hello   two 0-d scalars                       N = 2      hello_psgd.py's own problem
    N35     (3,), (4, 5), (2, 3, 2)               N = 35     the one-workgroup route (N <= 64)
    N64     (8, 8)                                N = 64     the last N on that route
    N65     (5, 13)                               N = 65     the first N on the large route, scalar loads
    N117    (7, 9), (33,), (2, 2, 2, 2), (5,)     N = 117    N % 4 = 1, the second 64-row tile partial
    N132    (16, 8), (4,)                         N = 132    N % 4 = 0: the 4-wide loads, three tiles, the last one of 4 rows
    N1028   (32, 32), (4,)                        N = 1028   Q is 4.2 MB: allocations can be told apart

The closures are one elementwise chain per parameter (tests/test_splu_class_gpu.py: richer closures gave Hessian-vector
products that parted by an ulp between two evaluations).  The initial scale is 1 unless stated."""
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

SETS = {"N35": [(3,), (4, 5), (2, 3, 2)], "N64": [(8, 8)], "N65": [(5, 13)], "N117": [(7, 9), (33,), (2, 2, 2, 2), (5,)],
        "N132": [(16, 8), (4,)], "N1028": [(32, 32), (4,)]}
LR, LR_Q, MAX_NORM = 0.05, 0.1, 2.0
TINY = float(np.finfo(np.float32).tiny)
DELTA = float(np.finfo(np.float32).eps) ** 0.5
DENSE_TOL = 1e-5                                                       # tests/test_dense_gpu.py, test_update_and_apply_match_fp64
STEPS = 3
DRAWS = 20                                                             # steps of probe draws a problem holds


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    m.set_dense_route("native")
    return m


def _dev():
    return torch.device("cuda:0")


def _n(name):
    return sum(int(np.prod(s)) for s in SETS[name])


_data = {}


def _problem(name):
    """initial parameters, the weights a of the loss and DRAWS steps of probe draws: float32 device tensors, made once"""
    if name not in _data:
        rng = np.random.default_rng(2028)
        shapes = SETS[name]
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())
        _data[name] = ([f(rng.standard_normal(s) * 0.5) for s in shapes], [f(np.exp(rng.uniform(-1.0, 1.0, s))) for s in shapes],
                       [f(rng.standard_normal(s)) for _ in range(DRAWS) for s in shapes])
    return _data[name]


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


def _closure(params, name, poison=None, once=False, calls=None):
    """sum_k sum a cosh(W) in float32: the gradient a sinh(W), a Hessian diag(a cosh(W)) that changes with W; one elementwise
    chain per parameter.  once: sum a tanh(W)^2 / 4 through the once_differentiable Function.  poison: a dict whose "x" (when not
    1) multiplies element 3 of the first parameter into the loss"""
    a_s = _problem(name)[1]

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


def _fresh(name, dtype=torch.float32):
    return [w.clone().to(dtype).requires_grad_(True) for w in _problem(name)[0]]


def _feed(monkeypatch, name):
    """the draws of psgd.py:713 / :721 come from the problem's list, in order, for whoever steps next"""
    it = iter(_problem(name)[2])
    monkeypatch.setattr(impl, "_randn_like", lambda p: next(it).to(p.dtype))


def _make(psgd, tail, name="N117", exact=True, clip=False, prob=1.0, seed=11, dtype=torch.float32, scale=1.0, poison=None,
          once=False, calls=None, **kw):
    params = _fresh(name, dtype)
    opt = psgd.Dense(params, scale, LR, LR_Q, MAX_NORM if clip else None, prob, exact, generator=torch.Generator().manual_seed(seed),
                     step_tail=tail, **kw)
    assert (opt._tail is not None) == (tail == "fused")
    return params, opt, _closure(params, name, poison, once, calls)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy().copy()


def _state(params, opt):
    mom = opt._momentum_buffer() if float(opt.momentum) > 0.0 else None
    return {"tensors": [_bits(t) for t in list(params) + [opt.Q] + ([mom] if mom is not None else [])],
            "counters": (opt._m_step, opt.probe_step, opt._param_round_step, opt.skipped_steps)}


def _assert_same(a, b, what):
    assert len(a["tensors"]) == len(b["tensors"]), what
    for i, (x, y) in enumerate(zip(a["tensors"], b["tensors"])):
        assert x.tobytes() == y.tobytes(), "%s: tensor %d differs" % (what, i)
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])


def _run(psgd, monkeypatch, tail, steps=STEPS, **kw):
    _feed(monkeypatch, kw.get("name", "N117"))
    params, opt, closure = _make(psgd, tail, **kw)
    for _ in range(steps):
        opt.step(closure)
    assert all(bool(torch.isfinite(p.float()).all()) for p in params)
    return _state(params, opt), opt


# --------------------------------------------------------------------------------------------------- the hand-written loop
def _hand_step(psgd, params, Q, closure, vs, k, exact, clip, mom=0.0, wd=0.0, m=None, whiten_dx=None):
    """One step of the loop a user writes from the two functions and torch ops (the loop of tests/test_splu_class_gpu.py with the
    dense pair in the middle).  whiten_dx: the flat probe of a whitening step ((dx, dg) = (probe, gradient), one backward).
    Returns (Q, m)."""
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
        Q = psgd.update_precond_dense(Q, dxs, dgs, LR_Q)
        feed = list(grads)
        if mom != 0.0:                       # m <- beta_k m + (1 - beta_k) g, beta_k = min(k / (k + 1), momentum); m is preconditioned
            beta, omb = psgd.uvd_momentum_coefficients(k, mom)
            g = torch.cat([x.reshape(-1) for x in grads])
            m = g * omb if beta == 0.0 else m * beta + g * omb
            feed = [m]
        pre = torch.cat([x.reshape(-1) for x in psgd.precond_grad_dense(Q, feed)])
        decay = None
        if mom != 0.0 or wd != 0.0:          # lr_eff as the step-tail kernel forms it (_FlatStep.step): fp64 from the fp32 squares, one rounding
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
    return Q, m


_hand_runs = {}


def _hand_run(psgd, name, exact, clip=False, mom=0.0, wd=0.0, steps=STEPS):
    """the state after every step; computed once per configuration, shared by the tests of both tails (never modified)"""
    key = (name, exact, clip, mom, wd, steps)
    if key not in _hand_runs:
        params = _fresh(name)
        closure = _closure(params, name)
        Q = psgd.dense_initial_factor(_n(name), 1.0, device=_dev())
        draws, m, per_step = iter(_problem(name)[2]), None, []
        for k in range(steps):
            vs = [next(draws) for _ in params]
            Q, m = _hand_step(psgd, params, Q, closure, vs, k, exact, clip, mom, wd, m)
            per_step.append({"tensors": [_bits(t) for t in list(params) + [Q] + ([m] if m is not None else [])],
                             "counters": (k + 1 if mom else 0, 0, 0, 0)})
        _hand_runs[key] = per_step
    return _hand_runs[key]


@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fd"])
@pytest.mark.parametrize("name", ["N35", "N64", "N65", "N117", "N132"])
def test_class_equals_the_hand_written_loop(psgd, monkeypatch, name, exact, tail):
    """a. 3 steps, the parameters and Q bit for bit after EVERY step: the two-buffer update against the function's fresh tensors"""
    want = _hand_run(psgd, name, exact)
    _feed(monkeypatch, name)
    params, opt, closure = _make(psgd, tail, name=name, exact=exact)
    assert opt.Q.shape == (_n(name), _n(name))
    for k in range(STEPS):
        opt.step(closure)
        _assert_same(_state(params, opt), want[k], "Dense(step_tail=%r) against the hand-written loop, step %d" % (tail, k))
    assert _bits(opt.Q).tobytes() != _bits(psgd.dense_initial_factor(_n(name), 1.0, device=_dev())).tobytes()     # Q did move


@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("name", ["N117", "N132"])
def test_momentum_and_weight_decay_equal_the_hand_written_loop(psgd, monkeypatch, name, tail):
    got, opt = _run(psgd, monkeypatch, tail, name=name, momentum=0.9, weight_decay=0.01)
    assert opt._m_step == STEPS
    _assert_same(got, _hand_run(psgd, name, True, False, 0.9, 0.01)[-1], "momentum and weight decay")


# ------------------------------------------------------------------------------------------------------ fused against torch
SWITCHES = {
    "float32": dict(),
    "float32, finite differences": dict(exact=False),
    "bfloat16 parameters": dict(dtype=torch.bfloat16),
    "float16 parameters": dict(dtype=torch.float16),
    "float16 parameters, finite differences": dict(dtype=torch.float16, exact=False),
    "momentum and weight decay": dict(momentum=0.9, weight_decay=0.01),
    "bfloat16, momentum and weight decay, finite differences": dict(dtype=torch.bfloat16, momentum=0.5, weight_decay=0.01, exact=False),
    "guarded": dict(nonfinite="skip", momentum=0.9),
}


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", ["N117", "N132"])
def test_both_tails_bit_identical(psgd, monkeypatch, name, switch):
    """b. the parameters and Q after every one of 3 steps"""
    kw = dict(SWITCHES[switch], name=name)
    runs = {}
    for tail in ("torch", "fused"):
        _feed(monkeypatch, name)
        params, opt, closure = _make(psgd, tail, **kw)
        runs[tail] = []
        for _ in range(STEPS):
            opt.step(closure)
            runs[tail].append(_state(params, opt))
        assert all(p.dtype == kw.get("dtype", torch.float32) for p in params) and opt.Q.dtype == torch.float32
        assert all(bool(torch.isfinite(p.float()).all()) for p in params)
    for k in range(STEPS):
        _assert_same(runs["fused"][k], runs["torch"][k], "%s, step %d" % (switch, k))
    assert runs["torch"][0]["tensors"][0].tobytes() != _bits(_fresh(name, kw.get("dtype", torch.float32))[0]).tobytes()


def _dyadic_run(psgd, tail, name):
    """a closure whose gradient is a fixed dyadic tensor, no update of Q, Q = 0.5 I: the preconditioned gradient is that tensor / 4
    and its sum of squares is exact in any order.  momentum 0.5 on a constant gradient leaves m = g exactly and puts both tails on
    the kernel's expression of lr_eff (_FlatStep.step: fp64 from the fp32 squares, rounded once)"""
    gen = torch.Generator().manual_seed(3)
    Ds = [(torch.randint(-64, 65, s, generator=gen).float() / 16.0).to(_dev()) for s in SETS[name]]
    params = _fresh(name)
    opt = psgd.Dense(params, 0.5, LR, LR_Q, 0.25, 0.0, True, step_tail=tail, generator=torch.Generator().manual_seed(5), momentum=0.5)
    for _ in range(STEPS):
        opt.step(lambda: sum(torch.sum(p * d) for p, d in zip(params, Ds)))
    assert bool(torch.equal(opt._out, torch.cat([d.reshape(-1) for d in Ds]) / 4.0))
    assert float(opt._out.norm()) > 0.25                                           # the clip is active
    return _state(params, opt)


@pytest.mark.parametrize("name", ["N117", "N132"])
def test_fused_tail_with_clipping_on_dyadic_gradients_is_bit_identical(psgd, name):
    a, b = _dyadic_run(psgd, "torch", name), _dyadic_run(psgd, "fused", name)
    _assert_same(b, a, "clipped step on dyadic gradients")
    assert a["tensors"][0].tobytes() != _bits(_fresh(name)[0]).tobytes()           # the parameters did move


# ------------------------------------------------------------------------------------------------------------- fp64 oracle
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("name", ["N117", "N132"])
def test_twenty_steps_track_the_fp64_oracle(psgd, monkeypatch, name, tail):
    """c. 20 updating steps.  The oracle's update_precond_dense / precond_grad_dense run in float64 on the class's own v, h and g,
    read from its flat buffers after each step; the oracle's Q starts at the class's initial Q and is never resynchronised.  After
    every step Q and the preconditioned gradient are within DENSE_TOL, relative and norm-wise."""
    _feed(monkeypatch, name)
    params, opt, closure = _make(psgd, tail, name=name)
    n64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    Q = n64(opt.Q)
    worst = [0.0, 0.0]
    for k in range(20):
        ptr = opt.Q.data_ptr()
        opt.step(closure)
        assert opt.Q.data_ptr() != ptr                                             # an updating step
        v, h, g = (n64(opt._flat_bufs[x]).reshape(-1, 1) for x in ("v", "h", "g"))
        Q = orc.update_precond_dense(Q, [v], [h], float(np.float32(LR_Q)))
        pre = orc.precond_grad_dense(Q, [g])[0]
        e_q, e_pre = rel_err(n64(opt.Q), Q), rel_err(n64(opt._out).reshape(-1, 1), pre)
        worst = [max(worst[0], e_q), max(worst[1], e_pre)]
        assert e_q < DENSE_TOL and e_pre < DENSE_TOL, (k, e_q, e_pre)
    print("%s %s: 20 steps, worst relative error of Q %.2e, of the preconditioned gradient %.2e" % (name, tail, *worst))
    assert rel_err(Q, np.eye(_n(name))) > 0.05                                     # the trajectory went somewhere


# ------------------------------------------------------------------------------------------- no N^2-sized allocation
def test_a_step_makes_no_allocation_of_the_size_of_q(psgd):
    """d. N = 1028.  After 2 warm-up steps one step's peak above its entry level stays below 4 N^2 bytes (one Q) on either tail; the
    hand-written functional loop under the same protocol reaches 4 N^2 (its update returns a fresh Q while the old one is alive).
    A condition, not a measurement."""
    name, N = "N1028", 1028
    one_q = 4 * N * N

    def peak_of(step):
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        entry = torch.cuda.max_memory_allocated()
        assert entry == torch.cuda.memory_allocated()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - entry

    peaks = {}
    for tail in ("torch", "fused"):
        params, opt, closure = _make(psgd, tail, name=name)
        assert opt.Q.numel() * 4 == one_q
        peaks[tail] = peak_of(lambda: opt.step(closure))
        del params, opt, closure
    hp = _fresh(name)
    hclosure = _closure(hp, name)
    box = {"Q": psgd.dense_initial_factor(N, 1.0, device=_dev())}

    def hand():
        vs = [torch.randn_like(p) for p in hp]
        box["Q"], _ = _hand_step(psgd, hp, box["Q"], hclosure, vs, 0, True, False)
    peaks["functional"] = peak_of(hand)
    print("peak over one step: class, torch tail %d B; class, fused tail %d B; functional loop %d B; one Q %d B"
          % (peaks["torch"], peaks["fused"], peaks["functional"], one_q))
    assert peaks["torch"] < one_q and peaks["fused"] < one_q
    assert peaks["functional"] >= one_q


# ------------------------------------------------------------------------------------------------------------ two buffers
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_q_alternates_between_two_buffers(psgd, monkeypatch, tail):
    """e. the data_ptr of Q alternates on updating steps; a step with preconditioner_update_probability = 0 keeps it, and the bits"""
    _feed(monkeypatch, "N132")
    params, opt, closure = _make(psgd, tail, name="N132")
    a, b = opt._Qs[0].data_ptr(), opt._Qs[1].data_ptr()
    assert a != b and opt.Q.data_ptr() == a
    seen = []
    for _ in range(4):
        opt.step(closure)
        seen.append(opt.Q.data_ptr())
    assert seen == [b, a, b, a]
    opt.step(closure)
    assert opt.Q.data_ptr() == b
    opt.preconditioner_update_probability.assign(0.0)
    q, p0 = _bits(opt.Q), _bits(params[0])
    both = [_bits(t) for t in opt._Qs]
    for _ in range(2):
        opt.step(closure)
        assert opt.Q.data_ptr() == b and _bits(opt.Q).tobytes() == q.tobytes()
    assert all(x.tobytes() == _bits(t).tobytes() for x, t in zip(both, opt._Qs))   # neither buffer was touched
    assert _bits(params[0]).tobytes() != p0.tobytes()                              # the parameters went on
    opt.preconditioner_update_probability.assign(1.0)
    opt.step(closure)
    assert opt.Q.data_ptr() == a and _bits(opt.Q).tobytes() != q.tobytes()
    assert [t.data_ptr() for t in opt._Qs] == [a, b]                               # the same two buffers for the life of the object


# ----------------------------------------------------------------------------------------------- first call, poisoned buffers
def _poison(t):
    t.view(torch.uint8).fill_(0xFF)


@pytest.mark.parametrize("name, kw", [("N35", {}), ("N117", dict(momentum=0.9, nonfinite="skip")), ("N132", dict(exact=False)),
                                      ("N132", dict(preconditioner_fit="whitening", probe_seed=1, momentum=0.9))],
                         ids=["N35", "N117 guarded momentum", "N132 finite differences", "N132 whitening"])
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_first_step_on_poisoned_buffers(psgd, monkeypatch, tail, name, kw):
    """f. the output, the momentum buffer, the three flat vectors, the spare buffer of Q, the kernels' workspace and the plan's
    scratch hold 0xFF bytes before the first step: nothing reads what it has not written"""
    want, _ = _run(psgd, monkeypatch, tail, name=name, clip=True, **kw)
    _feed(monkeypatch, name)
    params, opt, closure = _make(psgd, tail, name=name, clip=True, **kw)
    for t in list(opt._flat_bufs.values()) + [opt._out, opt._Qs[1 - opt._cur], impl._dense_workspace(_dev(), _n(name))]:
        _poison(t)
    if float(opt.momentum) > 0.0:
        _poison(opt._momentum_buffer())
    if opt._tail is not None:
        _poison(opt._tail.ws)
        _poison(opt._tail.sumsq)
    assert bool(torch.isnan(opt._Qs[1]).all()) and bool(torch.isnan(opt._out).all())
    for _ in range(STEPS):
        opt.step(closure)
    _assert_same(_state(params, opt), want, "first step on poisoned buffers")


# ------------------------------------------------------------------------------------------------------------ every switch
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("fit", ["hessian", "whitening"])
def test_a_skipped_step_keeps_every_bit_and_every_counter(psgd, monkeypatch, fit, tail):
    """g. nonfinite="skip" with a NaN in one gradient element (exact products: nothing was perturbed, so the parameters keep their
    bits too): Q (its bits and its data_ptr), the spare buffer, the parameters, the momentum buffer and all counters as they were"""
    _feed(monkeypatch, "N117")
    poison = {"x": 1.0}
    params, opt, closure = _make(psgd, tail, nonfinite="skip", momentum=0.9, poison=poison, preconditioner_fit=fit, probe_seed=9)
    for _ in range(2):
        opt.step(closure)
    before, ptr, spare = _state(params, opt), opt.Q.data_ptr(), _bits(opt._Qs[1 - opt._cur])
    poison["x"] = float("nan")
    loss = opt.step(closure)
    assert opt.last_step_skipped and opt.skipped_steps == 1 and math.isnan(float(loss.detach()))
    assert opt.Q.data_ptr() == ptr and _bits(opt._Qs[1 - opt._cur]).tobytes() == spare.tobytes()
    after = _state(params, opt)
    after["counters"] = after["counters"][:3] + (0,)
    _assert_same(after, before, "a skipped step")
    poison["x"] = 1.0
    opt.step(closure)
    assert not opt.last_step_skipped and opt.skipped_steps == 1 and opt.Q.data_ptr() != ptr
    assert _state(params, opt)["tensors"][0].tobytes() != before["tensors"][0].tobytes()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fd"])
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_a_loss_scale_does_not_move_a_bit_of_a_float32_run(psgd, monkeypatch, tail, exact):
    plain, _ = _run(psgd, monkeypatch, tail, exact=exact, clip=True, momentum=0.9)
    guarded, _ = _run(psgd, monkeypatch, tail, exact=exact, clip=True, momentum=0.9, nonfinite="skip")
    scaled, opt = _run(psgd, monkeypatch, tail, exact=exact, clip=True, momentum=0.9, nonfinite="skip", loss_scale=2 ** 8)
    assert float(opt.loss_scale) == 256.0 and opt.skipped_steps == 0
    _assert_same(guarded, plain, "nonfinite='skip' on finite data")
    _assert_same(scaled, plain, "loss_scale=2**8")


def _stalling_run(psgd, tail, rounding, steps=60):
    """examples/kron_bf16_stochastic_params.py (the case of tests/test_param_rounding_class_gpu.py) at N = 132: bfloat16 weights at
    1, loss |W - T|^2 / 2 with T = 1 + 0.05 randn, lr_params 2e-3, Q = I.  Every update is below half a bfloat16 spacing at 1."""
    gen = torch.Generator().manual_seed(0)
    targets = [(1.0 + 0.05 * torch.randn(s, generator=gen)).to(_dev()) for s in SETS["N132"]]
    params = [torch.ones(s, device=_dev(), dtype=torch.bfloat16, requires_grad=True) for s in SETS["N132"]]
    opt = psgd.Dense(params, 1.0, lr_params=2e-3, lr_preconditioner=0.05, step_tail=tail, generator=torch.Generator().manual_seed(1),
                     param_rounding=rounding, param_rounding_seed=2 if rounding == "stochastic" else None)
    closure = lambda: sum(0.5 * torch.sum((p.float() - t) ** 2) for p, t in zip(params, targets))
    torch.manual_seed(4)
    first, moved = float(closure().detach()), 0
    for _ in range(steps):
        before = [p.detach().clone() for p in params]
        opt.step(closure)
        moved += sum(int((p.detach() != b).sum()) for p, b in zip(params, before))
    return first, float(closure().detach()), moved, opt


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_stochastic_rounding_moves_weights_that_round_to_nearest_leaves_alone(psgd, tail):
    first, last, moved, opt = _stalling_run(psgd, tail, "nearest")
    assert moved == 0 and last == first and opt._param_round_step == 0
    first, last, moved, opt = _stalling_run(psgd, tail, "stochastic")
    print("stochastic rounding, %s tail: loss %.4e -> %.4e, %d weight changes written" % (tail, first, last, moved))
    assert moved > 0 and last < 0.9 * first and opt._param_round_step == 60


def test_stochastic_rounding_is_the_same_on_both_tails(psgd, monkeypatch):
    kw = dict(name="N132", dtype=torch.bfloat16, param_rounding="stochastic", param_rounding_seed=5, weight_decay=0.01)
    a, oa = _run(psgd, monkeypatch, "torch", **kw)
    b, _ = _run(psgd, monkeypatch, "fused", **kw)
    _assert_same(b, a, "stochastic rounding of the parameters")
    c, _ = _run(psgd, monkeypatch, "fused", **dict(kw, param_rounding="nearest", param_rounding_seed=None))
    assert oa._param_round_step == STEPS and any(x.tobytes() != y.tobytes() for x, y in zip(b["tensors"][:2], c["tensors"][:2]))


# --------------------------------------------------------------------------------------------------------------- whitening
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("name", ["N117", "N132"])
def test_one_whitening_step_equals_the_hand_written_loop(psgd, name, tail):
    """(dx, dg) = (probe, raw gradient).  The flat probe is the multi_randn draw of (probe_seed0, step 0) and lies within that
    kernel's bar of counter_randn; the step equals the hand-written loop bit for bit when the loop is fed the kernel's probe and
    within 1e-5 (relative, norm-wise) when it is fed counter_randn's.  The clip is on with the torch tail only: the plain fused
    tail forms the clipped lr_eff from the kernel's fp64 norm, not from the float32 expression of psgd.py:753-754 the loop
    writes."""
    clip = tail == "torch"
    params, opt, closure = _make(psgd, tail, name=name, clip=clip, preconditioner_fit="whitening", probe_seed=77)
    N = _n(name)
    opt.step(closure)
    seed = psgd.uvd_step_rounding_seed(77, 0)
    want = torch.empty(N, device=_dev())
    psgd.multi_randn([want], seed, 0)
    v32 = psgd.counter_randn(seed, 0, N)
    assert _bits(opt._flat_bufs["v"]).tobytes() == _bits(want).tobytes() and opt.probe_step == 1
    assert float(np.max(np.abs(want.cpu().numpy().astype(np.float64) - v32.astype(np.float64)))) <= PROBE_BAR
    runs = []
    for dx in (want, torch.from_numpy(v32).to(_dev())):
        hp = _fresh(name)
        Q, _ = _hand_step(psgd, hp, psgd.dense_initial_factor(N, 1.0, device=_dev()), _closure(hp, name), None, 0, True, clip,
                          whiten_dx=dx)
        runs.append(list(hp) + [Q])
    got = list(params) + [opt.Q]
    for i, (a, b) in enumerate(zip(got, runs[0])):
        assert _bits(a).tobytes() == _bits(b).tobytes(), "tensor %d against the loop fed the kernel's probe" % i
    for i, (a, b) in enumerate(zip(got, runs[1])):
        assert rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 1e-5, "tensor %d against the loop fed counter_randn" % i


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_whitening_needs_one_backward_per_step(psgd, tail):
    calls = []
    params, opt, closure = _make(psgd, tail, preconditioner_fit="whitening", probe_seed=3, once=True, calls=calls)
    state = torch.cuda.get_rng_state()
    for k in range(3):
        ptr = opt.Q.data_ptr()
        opt.step(closure)                                                  # a once_differentiable closure runs: no second backward
        assert opt.probe_step == k + 1 and len(calls) == k + 1 and opt.Q.data_ptr() != ptr
    assert torch.equal(torch.cuda.get_rng_state(), state)                  # no global draw
    hp, ho, hc = _make(psgd, tail, once=True)
    with pytest.raises(RuntimeError):
        ho.step(hc)                                                        # the Hessian fit cannot differentiate it twice


# ------------------------------------------------------------------------------------------------------------------ resume
RESUME = dict(momentum=0.9, nonfinite="skip", loss_scale=2 ** 4, preconditioner_fit="whitening", probe_seed=5, clip=True,
              weight_decay=0.01)


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_resume_is_bit_identical(psgd, tail):
    """h. N117; save after 3 steps, load into a new optimizer, 3 more: the bits of 6 uninterrupted steps (momentum, guard and
    whitening on).  The object that loads has its other buffer current: the load goes into whichever is."""
    params, opt, closure = _make(psgd, tail, **RESUME)
    for _ in range(6):
        opt.step(closure)
    want = _state(params, opt)
    p1, o1, c1 = _make(psgd, tail, **RESUME)
    for _ in range(3):
        o1.step(c1)
    sd = o1.state_dict()
    assert sd["preconditioner"] == "dense" and sd["Q"].device.type == "cpu" and torch.equal(sd["Q"], o1.Q.cpu())
    assert sd["probe_step"] == 3 and sd["momentum_step"] == 3
    saved = [p.detach().clone() for p in p1]
    p2, o2, c2 = _make(psgd, tail, seed=999, **dict(RESUME, probe_seed=123))
    o2.lr_params.assign(9.0)
    ptr = o2.Q.data_ptr()
    o2.load_state_dict(sd)
    assert o2.Q.data_ptr() == ptr and _bits(o2.Q).tobytes() == _bits(sd["Q"]).tobytes()
    with torch.no_grad():
        for p, s in zip(p2, saved):
            p.copy_(s)
    for _ in range(3):
        o2.step(c2)
    _assert_same(_state(p2, o2), want, "resumed run")
    assert float(o2.lr_params) == LR and o2.probe_seed0 == 5


# ------------------------------------------------------------------------------------------------------------------- hello
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_hello_psgd_converges_through_the_class(psgd, monkeypatch, tail):
    """i. hello_psgd.py:7-27 through psgd.Dense on the device: xs = (-1, 1), Q = 0.1 I, 500 iterations, preconditioner step 0.2,
    learning rate 0.5, with the probe draws of examples/hello_psgd.py's run(seed=0).  The bar is test_hello_psgd_converges of
    tests/test_host_logic_cpu.py, unchanged: f starts at 4 and ends below 1e-8, both coordinates within 1e-3 of 1."""
    from examples.hello_psgd import rosenbrock
    gen = torch.Generator().manual_seed(0)
    monkeypatch.setattr(impl, "_randn_like", lambda p: torch.randn(p.shape, generator=gen, dtype=p.dtype).to(p.device))
    xs = [torch.tensor(-1.0, device=_dev(), requires_grad=True), torch.tensor(1.0, device=_dev(), requires_grad=True)]
    opt = psgd.Dense(xs, 0.1, lr_params=0.5, lr_preconditioner=0.2, step_tail=tail)
    assert opt.Q.shape == (2, 2)
    f = torch.stack([opt.step(lambda: rosenbrock(xs)).detach() for _ in range(500)]).cpu().tolist()
    xs = [float(x.detach()) for x in xs]
    print("hello through class Dense, %s tail: f %.3e -> %.3e, x = (%.6f, %.6f)" % (tail, f[0], f[-1], xs[0], xs[1]))
    assert f[0] == pytest.approx(4.0) and f[-1] < 1e-8 and abs(xs[0] - 1) < 1e-3 and abs(xs[1] - 1) < 1e-3
