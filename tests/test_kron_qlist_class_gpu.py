"""class Kron(preconditioner_update="quad", quad_route="list") against quad_route="layer": five steps on five small matrix
parameters, one of them a (dense, scale) layer that quad_diagonal=True brings in and that stays on the per-layer calls.  Parameters,
factors and quad_L bit for bit, uninterrupted and across a state_dict saved under "layer" and loaded under "list"."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(5, 7), (70, 6), (65, 131), (6, 70), (64, 64)]
FORMATS = ["dense", "dense", "dense", ("dense", "scale"), "dense"]
STEPS, SAVE_AT = 5, 2


def _model():
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(DEV) for s in SHAPES]
    return params, lambda: sum(((x - t) ** 2).sum() for x, t in zip(params, targets))


def _opt(params, route):
    return psgd.Kron(params, FORMATS, 1.0, 0.01, 0.1, preconditioner_fit="whitening", probe_seed=3, preconditioner_update="quad",
                     generator=torch.Generator().manual_seed(1), quad_diagonal=True, quad_route=route)


def _everything(opt, params):
    return [t for i in range(len(SHAPES)) for t in opt.factors[i] + [opt.quad_L[i], params[i]]]


def test_list_route_has_the_bits_of_the_layer_route_and_resumes_its_checkpoint():
    runs = {}
    for route in ("layer", "list"):
        params, closure = _model()
        opt = _opt(params, route)
        assert opt.quad_layers == [0, 1, 2, 3, 4]
        for step in range(STEPS):
            if step == SAVE_AT and route == "layer":
                sd, saved = opt.state_dict(), [x.detach().clone() for x in params]
            opt.step(closure)
        runs[route] = _everything(opt, params)
    assert "quad_route" not in sd
    assert opt._quad_listed == [0, 1, 2, 4] and opt._quad_layer == [3] and len(opt._quad_plan.groups) == 1
    assert all(torch.equal(a, b) for a, b in zip(runs["layer"], runs["list"]))
    assert not torch.equal(runs["list"][0], torch.eye(5, device=DEV))                       # the state did move
    params, closure = _model()
    with torch.no_grad():
        for x, s in zip(params, saved):
            x.copy_(s)
    resumed = _opt(params, "list")
    resumed.load_state_dict(sd)
    for _ in range(SAVE_AT, STEPS):
        resumed.step(closure)
    assert all(torch.equal(a, b) for a, b in zip(runs["layer"], _everything(resumed, params)))
