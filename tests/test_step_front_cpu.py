"""The two members of _StepFeatures under every optimizer class's step(), on CPU tensors: the closure front
(_closure_gradients: the order of closure calls, backward passes and draws) and the coefficient rule of the torch tail
(_tail_coefficients, against a numpy restatement of the rule)."""
import numpy as np
import pytest
import torch

from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl

_StepFeatures = impl._StepFeatures


# ------------------------------------------------------------------------------------------------------- _closure_gradients
class _Front:
    """the least a class must have for _closure_gradients: _params and _loss_of"""
    _loss_of = staticmethod(_StepFeatures._loss_of)
    _closure_gradients = _StepFeatures._closure_gradients

    def __init__(self, params):
        self._params = params


def _problem(returns_tuple=False):
    """loss = 0.5 x'Hx over x = (p0, p1) flattened, H symmetric with small integer entries: every product below is exact"""
    g = torch.Generator().manual_seed(0)
    p0 = torch.randint(-3, 4, (3, 2), generator=g).float().requires_grad_(True)
    p1 = torch.randint(-3, 4, (2,), generator=g).float().requires_grad_(True)
    A = torch.randint(-2, 3, (8, 8), generator=g).float()
    H = A + A.t()
    events = []

    def closure():
        events.append("closure")
        x = torch.cat([p0.reshape(-1), p1])
        loss = 0.5 * x @ (H @ x)
        return (loss, "aux") if returns_tuple else loss

    def randn(p):
        events.append(("randn", [id(q) for q in (p0, p1)].index(id(p))))
        return torch.randint(-2, 3, p.shape, generator=g).to(p.dtype)

    def perturb(vs):
        assert not torch.is_grad_enabled()
        events.append("perturb")
        for p, v in zip((p0, p1), vs):
            p.add_(v)
    return _Front([p0, p1]), H, closure, randn, perturb, events


def _cat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


IDENTITY = lambda loss: loss
DRAWS = [("randn", 0), ("randn", 1)]


def test_closure_front_finite_differences():
    front, H, closure, randn, perturb, events = _problem()
    x0 = _cat(front._params).detach().clone()
    ret, grads, second, vs = front._closure_gradients(closure, "fd", IDENTITY, randn, 0.5, perturb)
    assert events == ["closure"] + DRAWS + ["perturb", "closure"]
    assert isinstance(ret, torch.Tensor) and ret.item() == (0.5 * x0 @ (H @ x0)).item()     # the loss before the perturbation
    assert [v.shape for v in vs] == [(3, 2), (2,)] and all(v.dtype == torch.float32 for v in vs)
    assert torch.equal(_cat(front._params).detach(), x0 + _cat(vs))                         # the caller undoes it, not the front
    assert torch.equal(_cat(grads), H @ x0) and torch.equal(_cat(second), H @ (x0 + _cat(vs)))
    assert not any(t.requires_grad for t in list(grads) + list(second) + list(vs))


def test_closure_front_finite_differences_without_a_hook_adds_per_tensor():
    front, H, closure, randn, _, events = _problem()
    x0 = _cat(front._params).detach().clone()
    _, _, second, vs = front._closure_gradients(closure, "fd", IDENTITY, randn, 0.5)
    assert events == ["closure"] + DRAWS + ["closure"]
    assert torch.equal(_cat(second), H @ (x0 + _cat(vs)))


def test_closure_front_exact_products():
    front, H, closure, randn, perturb, events = _problem()
    x0 = _cat(front._params).detach().clone()
    ret, grads, second, vs = front._closure_gradients(closure, "exact", IDENTITY, randn, 0.5, perturb)
    assert events == ["closure"] + DRAWS                                                     # delta is not applied on this route
    assert torch.equal(_cat(second), H @ _cat(vs)) and torch.equal(_cat(grads), H @ x0)
    assert torch.equal(_cat(front._params).detach(), x0)
    assert not any(t.requires_grad or t.grad_fn is not None for t in list(grads) + list(second))


@pytest.mark.parametrize("route", ["whitening", None])
def test_closure_front_without_a_draw(route):
    front, H, closure, randn, perturb, events = _problem()
    x0 = _cat(front._params).detach().clone()
    ret, grads, second, vs = front._closure_gradients(closure, route, IDENTITY, randn, 0.5, perturb)
    assert events == ["closure"] and second is None and vs is None
    assert torch.equal(_cat(grads), H @ x0) and not any(g.requires_grad for g in grads)


@pytest.mark.parametrize("route", ["fd", "exact", "whitening", None])
def test_closure_front_loss_scale_and_tuple_returns(route):
    """a loss scale of 8 makes every gradient exactly 8 times the unscaled one; what the closure returns is passed through"""
    plain = _problem()
    scaled = _problem(returns_tuple=True)
    _, grads, second, vs = plain[0]._closure_gradients(plain[2], route, IDENTITY, plain[3], 0.5, plain[4])
    ret, grads8, second8, vs8 = scaled[0]._closure_gradients(scaled[2], route, lambda loss: loss * 8.0, scaled[3], 0.5, scaled[4])
    assert type(ret) is tuple and len(ret) == 2 and ret[1] == "aux" and ret[0].requires_grad    # untouched: still the closure's
    assert all(torch.equal(a * 8.0, b) for a, b in zip(grads, grads8)) and not any(g.requires_grad for g in grads8)
    if second is not None:
        assert all(torch.equal(a * 8.0, b) for a, b in zip(second, second8))
        assert all(torch.equal(a, b) for a, b in zip(vs, vs8))                                  # the draws are never scaled
    else:
        assert second8 is None and vs8 is None


def test_step_route():
    class Opt:
        _step_route = _StepFeatures._step_route

        def __init__(self, whiten, exact):
            self._whiten, self.exact_hessian_vector_product = whiten, impl._Hyper(exact)
    for whiten in (False, True):
        for exact in (False, True):
            assert Opt(whiten, exact)._step_route(False) is None
            assert Opt(whiten, exact)._step_route(True) == ("whitening" if whiten else "exact" if exact else "fd")


# ------------------------------------------------------------------------------------------------------- _tail_coefficients
def _rule(lr, wd, groups, max_norm, sumsq, tiny, k):
    """the rule in numpy scalars: [(lr_eff, c or None)] * k as float32"""
    f32, f64 = np.float32, np.float64
    out = [None] * k
    for indices, scale, wd_j in (groups if groups is not None else [(range(k), 1.0, wd)]):
        lr_j = f32(f64(lr) * f64(scale))
        if sumsq is not None:
            with np.errstate(all="ignore"):
                ratio = f64(f32(max_norm)) / (np.sqrt(f64(sumsq)) + f64(f32(tiny)))
                ratio = ratio if np.isnan(ratio) else min(ratio, f64(1.0))
            lr_j = f32(f64(lr_j) * ratio)
        c = None if f32(wd_j) == 0 else f32(lr_j * f32(wd_j))
        for i in indices:
            out[i] = (lr_j, c)
    return out


def _bits(x):
    if isinstance(x, torch.Tensor):
        assert x.dtype == torch.float32 and x.dim() == 0
        return x.view(torch.int32).item()
    assert isinstance(x, float) and float(np.float32(x)) == x                              # a Python float that holds a float32
    return int(np.float32(x).view(np.int32))


TINY = float(np.finfo(np.float32).tiny)
GROUPS = [((0, 2), 0.5, 0.0), ((1, 3, 4), 3.0, 0.3)]
CLIPS = {"none": (1.7, None), "inactive": (1.7, 1.3), "active": (1.7, 123.456), "active-small-norm": (1e-3, 7.0 / 3.0),
         "nan": (1.7, float("nan")), "zero": (1.7, 0.0)}


@pytest.mark.parametrize("clip", sorted(CLIPS))
@pytest.mark.parametrize("groups", [None, GROUPS], ids=["plain", "groups"])
@pytest.mark.parametrize("wd", [0.0, 0.01, 1e-46], ids=["wd0", "wd", "wd-below-subnormal"])
def test_tail_coefficients_are_the_rule_bit_for_bit(clip, groups, wd):
    max_norm, s = CLIPS[clip]
    sumsq = None if s is None else torch.tensor(s, dtype=torch.float64)
    lr, k = 0.037, 5
    if groups is not None and wd == 1e-46:
        groups = [(g[0], g[1], 1e-46) for g in groups]
    got = _StepFeatures._tail_coefficients(lr, wd, groups, max_norm, sumsq, TINY, k)
    want = _rule(lr, wd, groups, max_norm, s, TINY, k)
    assert len(got) == k
    for j, ((lr_eff, c), (lr_want, c_want)) in enumerate(zip(got, want)):
        assert isinstance(lr_eff, torch.Tensor) == (sumsq is not None), j                       # device scalars only with a clip
        if np.isnan(lr_want):
            assert clip == "nan" and torch.isnan(lr_eff).item(), j
        else:
            assert _bits(lr_eff) == int(lr_want.view(np.int32)), (j, lr_eff, lr_want)
        if c_want is None:
            assert c is None, j
        elif np.isnan(c_want):
            assert torch.isnan(c).item(), j
        else:
            assert _bits(c) == int(c_want.view(np.int32)), (j, c, c_want)
    # what the cases are there for
    if clip == "inactive" or clip == "zero":
        assert all(_bits(a) == int(np.float32(np.float64(lr) * (1.0 if groups is None else g)).view(np.int32))
                   for (a, _), g in zip(got, (0.5, 3.0, 0.5, 3.0, 3.0)))
    if clip.startswith("active"):
        assert all(float(a) < lr * (1.0 if groups is None else 3.0) * 0.5 for a, _ in got)
    if groups is GROUPS:                                                                        # the group with weight decay 0
        assert got[0][1] is None and got[2][1] is None and None not in (got[1][1], got[3][1], got[4][1])
    else:                                                       # fl32(1e-46) == 0: no decay term, as for a weight decay of 0
        assert all((c is None) == (wd != 0.01) for _, c in got)
