"""class Kron(quad_tensor=True, quad_tensor_route="list") against quad_tensor_route="layer": three conv-shaped parameters and one
matrix, five steps, bit for bit -- uninterrupted, and across a checkpoint saved under one route and loaded under the other.  At
these shapes no side is split (asserted on the plan), so the grouped update owes the per-layer bits."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = ((6, 5, 3, 3), (8, 6, 3, 3), (5, 7), (4, 8, 1, 1))


def _model():
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(DEV) for s in SHAPES]
    return params, lambda: sum(((x - t) ** 2).sum() for x, t in zip(params, targets))


def _opt(params, route):
    return psgd.Kron(params, "dense", 1.0, 0.01, 0.1, preconditioner_fit="whitening", probe_seed=3, preconditioner_update="quad",
                     generator=torch.Generator().manual_seed(1), any_rank=True, quad_tensor=True, quad_tensor_route=route)


def _state(opt, params):
    return [x for i in range(len(SHAPES)) for x in opt.factors[i] + [opt.quad_L[i], params[i]]]


@pytest.mark.parametrize("saved_under, resumed_under", [("list", "layer"), ("layer", "list")])
def test_list_route_is_the_layer_route_bit_for_bit(saved_under, resumed_under):
    runs = {route: _model() for route in ("list", "layer")}
    opts = {route: _opt(runs[route][0], route) for route in runs}
    assert opts["list"].quad_tensor_layers == opts["layer"].quad_tensor_layers == [0, 1, 3] and opts["layer"].quad_tensor_plan is None
    assert opts["list"].quad_tensor_plan.slices == [(1, 1, 1)] * 3
    for step in range(5):
        if step == 2:
            sd, at = opts[saved_under].state_dict(), [x.detach().clone() for x in runs[saved_under][0]]
        for route in runs:
            opts[route].step(runs[route][1])
    assert opts["list"].state_dict().keys() == opts["layer"].state_dict().keys()
    have, want = _state(opts["list"], runs["list"][0]), _state(opts["layer"], runs["layer"][0])
    assert all(torch.equal(a, b) for a, b in zip(have, want))
    params, closure = _model()
    with torch.no_grad():
        for x, s in zip(params, at):
            x.copy_(s)
    again = _opt(params, resumed_under)
    again.load_state_dict(sd)
    for _ in range(3):
        again.step(closure)
    assert all(torch.equal(a, b) for a, b in zip(_state(again, params), want))
