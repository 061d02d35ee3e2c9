"""class Kron(preconditioner_update="quad") against a hand-written loop over the functional calls."""
import numpy as np
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(5, 7), (70, 3, 3), (6,), (4, 6)]             # two matrix layers (one a rank-3 view), a vector layer, a (dense, scale) layer
FORMATS = ["dense", "dense", "dense", ("dense", "scale")]
QUAD, OTHER = [0, 1], [2, 3]
LR, LR_Q = 0.01, 0.1


def _model():
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(DEV) for s in SHAPES]
    return params, lambda: sum(((p - t) ** 2).sum() for p, t in zip(params, targets))     # separable: no layer sees another


def _opt(params, update="quad", **kw):
    return psgd.Kron(params, FORMATS, 1.0, LR, LR_Q, any_rank=True, preconditioner_fit="whitening", probe_seed=3,
                     generator=torch.Generator().manual_seed(1), preconditioner_update=update, **kw)


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_three_steps_are_the_functional_calls(tail):
    params, closure = _model()
    opt = _opt(params, step_tail=tail)
    assert opt.quad_layers == QUAD
    tri_params, tri_closure = _model()
    tri = _opt(tri_params, "triangular", step_tail=tail)
    hand, hand_closure = _model()
    state = {i: psgd.kron_quad_initial_state(SHAPES[i][0], int(np.prod(SHAPES[i][1:])), device=DEV) for i in QUAD}
    for _ in range(3):
        opt.step(closure)
        tri.step(tri_closure)
        grads = torch.autograd.grad(hand_closure(), hand)
        with torch.no_grad():
            for i in QUAD:
                Ql, Qr, L = state[i]
                g = grads[i].reshape(Ql.shape[0], Qr.shape[0])
                psgd.update_precond_kron_quad_(Ql, Qr, L, g, LR_Q)
                hand[i].sub_((float(np.float32(LR)) * psgd.precond_grad_kron_quad(Ql, Qr, g)).reshape(SHAPES[i]))
    for i in QUAD:
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [opt.quad_L[i]], state[i]))
        assert torch.equal(params[i], hand[i])
    for i in OTHER:                                     # the same probe stream, the triangular update
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i], tri.factors[i])) and torch.equal(params[i], tri_params[i])


def test_state_dict_round_trip_resumes_bit_for_bit():
    params, closure = _model()
    opt = _opt(params)
    for _ in range(2):
        opt.step(closure)
    sd = opt.state_dict()
    assert sd["preconditioner_update"] == "quad" and len(sd["quad_L"]) == len(QUAD)
    assert "quad_L" not in _opt(_model()[0], "triangular").state_dict()
    saved = [p.detach().clone() for p in params]
    opt.step(closure)
    again_params, again_closure = _model()
    with torch.no_grad():
        for p, s in zip(again_params, saved):
            p.copy_(s)
    again = _opt(again_params)
    again.load_state_dict(sd)
    again.step(again_closure)
    assert all(torch.equal(a, b) for a, b in zip(params, again_params))
    for i in QUAD:
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [opt.quad_L[i]], again.factors[i] + [again.quad_L[i]]))


def test_a_guarded_step_with_an_inf_gradient_leaves_the_state():
    params, closure = _model()
    opt = _opt(params, nonfinite="skip")
    opt.step(closure)
    before = [[t.clone() for t in opt.factors[i] + [opt.quad_L[i]]] for i in QUAD]
    opt.step(lambda: closure() + params[0].sum() * float("inf"))
    assert opt.last_step_skipped
    for i, old in zip(QUAD, before):
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [opt.quad_L[i]], old))
