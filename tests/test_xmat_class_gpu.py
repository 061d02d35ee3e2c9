"""class XMat: the hand-written loop, fused against torch tail, a checkpoint round trip, the whitening fit against float64."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from examples.xmat_class import whiten
from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl
from tests.xmat_cases import STATE_BAR, TINY32, err, xmat_update_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(7, 9), (33,), (2, 2, 2, 2), (5,)]                            # N = 117: odd, the dword route, a middle element
LR, LR_Q = 0.05, 0.1
ON = dict(momentum=0.9, weight_decay=0.01, grad_clip_max_norm=2.0, nonfinite="skip")


def _setup(monkeypatch, dtype=torch.float32, **kw):
    """parameters, optimizer, closure (its Hessian changes with the parameters); the draws of psgd.py:713 from one seeded list"""
    gen = torch.Generator().manual_seed(5)
    params = [(0.5 * torch.randn(s, generator=gen)).to(DEV, dtype).requires_grad_() for s in SHAPES]
    weights = [torch.exp(torch.rand(s, generator=gen) * 2 - 1).to(DEV) for s in SHAPES]
    draws = iter([torch.randn(s, generator=gen).to(DEV, dtype) for _ in range(8) for s in SHAPES])
    monkeypatch.setattr(impl, "_randn_like", lambda p: next(draws))
    opt = psgd.XMat(params, 1.0, LR, LR_Q, generator=torch.Generator().manual_seed(11), **kw)
    return params, opt, lambda: sum(torch.sum(w * torch.cosh(p.float())) for w, p in zip(weights, params))


def _bits(params, opt):
    return [t.detach().clone() for t in list(params) + [opt.a] + ([] if opt.b is None else [opt.b])]


def _same(xs, ys):
    return len(xs) == len(ys) and all(torch.equal(x, y) for x, y in zip(xs, ys))


@pytest.mark.parametrize("diagonal", [False, True])
def test_five_steps_equal_the_hand_written_loop(monkeypatch, diagonal):
    params, opt, closure = _setup(monkeypatch, diagonal=diagonal)
    for _ in range(5):
        opt.step(closure)
    got = _bits(params, opt)
    params, _, closure = _setup(monkeypatch)
    a, b = psgd.xmat_initial_state(117, 1.0, DEV)
    b = None if diagonal else b
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    for _ in range(5):
        vs = [impl._randn_like(p) for p in params]
        grads = torch.autograd.grad(closure(), params, create_graph=True)
        Hvs = torch.autograd.grad(grads, params, vs)
        pre = psgd.update_precond_grad_Xmat_math_(a, b, cat(vs), cat(Hvs), cat(grads).detach(), LR_Q, TINY32)
        with torch.no_grad():
            for p, d in zip(params, torch.split(pre, [p.numel() for p in params])):
                p.sub_(LR * d.reshape(p.shape))
    assert _same(got, [p.detach() for p in params] + [a] + ([] if diagonal else [b]))
    assert not torch.equal(a, torch.ones_like(a))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_both_tails_bit_identical_with_the_switches_on(monkeypatch, dtype):
    runs = []
    for tail in ("torch", "fused"):
        params, opt, closure = _setup(monkeypatch, dtype, step_tail=tail, **ON)
        for _ in range(3):
            opt.step(closure)
        assert opt.skipped_steps == 0 and (opt._tail is not None) == (tail == "fused")
        runs.append(_bits(params, opt) + [opt._momentum_buffer().clone()])
    assert _same(*runs)


def test_checkpoint_round_trip_continues_bit_identically(monkeypatch):
    kw = dict(step_tail="fused", preconditioner_fit="whitening", probe_seed=5, **ON)
    params, opt, closure = _setup(monkeypatch, **kw)
    for _ in range(3):
        opt.step(closure)
    sd, saved = opt.state_dict(), [p.detach().clone() for p in params]
    assert sd["preconditioner"] == "xmat" and torch.equal(sd["a"], opt.a.cpu()) and torch.equal(sd["b"], opt.b.cpu())
    for _ in range(3):
        opt.step(closure)
    want = _bits(params, opt)
    p2, o2, c2 = _setup(monkeypatch, **dict(kw, probe_seed=99))
    o2.load_state_dict(sd)
    with torch.no_grad():
        for p, s in zip(p2, saved):
            p.copy_(s)
    for _ in range(3):
        o2.step(c2)
    assert _same(_bits(p2, o2), want)
    assert "b" not in _setup(monkeypatch, diagonal=True)[1].state_dict()


def test_whitening_fit_tracks_the_float64_restatement():
    """500 steps on the 256-element quadratic of examples/xmat_class.py; the restatement runs in float64 on the class's own v and
    h, read after every step, never resynchronised.  The spread itself is printed, not judged."""
    state = {"a": torch.ones(256, dtype=torch.float64), "b": torch.zeros(256, dtype=torch.float64)}

    def follow(opt):
        v, h = (opt._flat_bufs[k].double().cpu() for k in ("v", "g"))     # (no momentum: h and g are one buffer)
        state["a"], state["b"] = xmat_update_ref(state["a"], state["b"], v, h, float(torch.tensor(0.1, dtype=torch.float32)), TINY32)
    got, opt = whiten(on_step=follow)
    want = (state["a"] ** 2 + torch.flip(state["b"], [0]) ** 2) * torch.logspace(-2, 2, 256, dtype=torch.float64)
    print("whitening: diag(Q'Q) sigma_g in [%.4f, %.4f]; against float64 %.2e" % (float(got.min()), float(got.max()), err(got, want)))
    assert opt.probe_step == 500 and err(got, want) < STATE_BAR
