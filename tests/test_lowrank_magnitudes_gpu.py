"""GPU: UVd and sparse LU on data far from O(1) (Kron and dense have such tests; these two families had none).

Both updates are scale-free in their data up to `tiny`: the gradient of the preconditioner is normalised by its own maximum / norm, so
scaling (v, h) -- or (dx, dg) -- by 2^k must leave the new state where it was, while the intermediates move by 2^2k (and the norm of
the UVd factor update by 2^4k).  The applies are linear in g.  Powers of two: the scaled inputs are exact, the fp64 oracle sees the same
numbers.  Bars: those of tests/test_uvd_gpu.py and tests/test_splu_gpu.py, hard (state 1e-5, ranks above 32 of UVd 2e-5; increment
2e-3; apply 1e-5, relative to the scaled result); the bf16-state sparse-LU update by the off-by-one-code rule of
tests/test_splu_bf16_gpu.py.

Which k: the fp32 NumPy oracle (the same functions on float32 arrays) was run on the CPU at every k asked for, and a k is kept where
it stays inside these bars.
  UVd (v, h) * 2^k, asked -40, -20, 20, 40: kept -40, -20, 20 (fp32 oracle: state <= 3.0e-8, increment <= 4.2e-5, the figures of k = 0).
      Dropped 40: the norm of the factor update, sqrt|a'a (atV V')(atV V')' + ...| (psgd.py:594-596), is a product of four factors
      2^40: 2^160 is past the largest fp32 number, the fp32 oracle returns NaN.  A reference in fp32 overflows there as well, so
      there is nothing to hold the kernels to (they form that norm in fp64 and would pass).
  UVd g * 2^k, -100, -60, 60, 100: all kept (linear; 2^100 * O(10) < 2^128, 2^-100 is a normal number).
  sparse LU (dx, dg) * 2^k, -40, -20, 20, 40: all kept (fp32 oracle: state <= 8.6e-8, increment <= 3.1e-4 at every k, the figures
      of k = 0: its gradient is a sum of products of two factors only).
  sparse LU g * 2^k, -100, -60, 60, 100: all kept (fp32 oracle <= 1.7e-7)."""
import functools

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from tests import uvd_cases as uc
from tests.splu_cases import make_splu_problem
from tests.uvd_cases import TINY32, rel_err

pytestmark = pytest.mark.gpu

APPLY_TOL = 1e-5
STATE_TOL = 1e-5
INCR_TOL = 2e-3
STEP = 0.01
UVD_K = (-40, -20, 20)
G_K = (-100, -60, 60, 100)
SPLU_K = (-40, -20, 20, 40)
UVD_SHAPES = [(1021, 10), (1021, 32), (2049, 40), (2049, 64)]
SPLU_RANKS = (7, 32, 47, 64)
SPLU_N = 1021
KEYS = ("L12", "l3", "U12", "u3")


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import preconditioned_stochastic_gradient_descent as m
    assert torch.cuda.is_available()
    return m


def _t(a):
    return torch.tensor(np.asarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _uvd_problem(N, r, kind):
    p = uc.make_uvd_problem(N, r, seed=N + r, d_spread=0.3) if kind == "default" else uc.gram_case(N, r, kind)
    for a in p.values():
        a.setflags(write=False)
    return p


def _scaled(p, **k):
    """a copy of the problem with the named columns multiplied by 2^k"""
    return {name: (np.ldexp(a, k[name]) if name in k else a.copy()) for name, a in p.items()}


# ------------------------------------------------------------------------------------------------ UVd
@pytest.mark.parametrize("kind", ("default", "cyclic"))
@pytest.mark.parametrize("N,r", UVD_SHAPES)
@pytest.mark.parametrize("k,kg", list(zip(UVD_K, (100, -60, 60))))
def test_uvd_update_and_fused_step_are_scale_free(psgd, N, r, kind, k, kg):
    p = _scaled(_uvd_problem(N, r, kind), v=k, h=k, g=kg)
    for upd in (True, False):
        q = {a: x.astype(np.float64) for a, x in p.items()}
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=False, update_U=upd)
        ref_out = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])
        for fused in (0, 1):
            t = {a: _t(x) for a, x in p.items()}
            if fused:
                out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32,
                                                                    balance=False, update_U=upd)
                e = rel_err(out.cpu().numpy(), ref_out)
                assert e < APPLY_TOL, (upd, e)
            else:
                psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=False, update_U=upd)
            for a in ("U", "V", "d"):
                e = rel_err(t[a].cpu().numpy(), q[a])
                assert e < (2 * STATE_TOL if r > 32 else STATE_TOL), (fused, upd, a, e)
            for a in (("U" if upd else "V"), "d"):
                e = rel_err(t[a].cpu().numpy().astype(np.float64) - p[a], q[a] - p[a].astype(np.float64))
                print("uvd N=%d r=%d %s k=%d fused=%d update_%s: increment of %s %.2e" % (N, r, kind, k, fused, "U" if upd else "V", a, e))
                assert e < INCR_TOL, (fused, upd, a, e)
            frozen = "V" if upd else "U"
            assert np.array_equal(t[frozen].cpu().numpy(), p[frozen])


@pytest.mark.parametrize("kind", ("default", "cyclic"))
@pytest.mark.parametrize("N,r", UVD_SHAPES)
def test_uvd_apply_is_linear_in_g(psgd, N, r, kind):
    p0 = _uvd_problem(N, r, kind)
    for kg in G_K:
        p = _scaled(p0, g=kg)
        out = psgd.precond_grad_UVd_math(_t(p["U"]), _t(p["V"]), _t(p["d"]), _t(p["g"]))
        ref = orc.precond_grad_UVd_math(*(p[a].astype(np.float64) for a in ("U", "V", "d", "g")))
        assert np.isfinite(ref).all() and np.linalg.norm(ref) > 0
        e = rel_err(out.cpu().numpy(), ref)
        assert e < APPLY_TOL, (kg, e)


# ------------------------------------------------------------------------------------------------ sparse LU
@functools.lru_cache(maxsize=None)
def _splu_problem(r):
    p = make_splu_problem(SPLU_N, r, seed=3 * SPLU_N + r)
    for a in p.values():
        a.setflags(write=False)
    return p


def _splu_base(q, r):
    rho = np.sqrt(max(np.max(np.diag(q["L12"][:r])), np.max(q["l3"], initial=-np.inf)) /
                  max(np.max(np.diag(q["U12"][:, :r])), np.max(q["u3"], initial=-np.inf)))
    return {"L12": q["L12"] / rho, "l3": q["l3"] / rho, "U12": q["U12"] * rho, "u3": q["u3"] * rho}


@pytest.mark.parametrize("r", SPLU_RANKS)
@pytest.mark.parametrize("k", SPLU_K)
def test_splu_update_is_scale_free(psgd, r, k):
    p = _scaled(_splu_problem(r), dx=k, dg=k)
    t, q = {a: _t(x) for a, x in p.items()}, {a: x.astype(np.float64) for a, x in p.items()}
    new = psgd.update_precond_splu(t["L12"], t["l3"], t["U12"], t["u3"], [t["dx"]], [t["dg"]], STEP)
    ref = orc.update_precond_splu(q["L12"], q["l3"], q["U12"], q["u3"], [q["dx"]], [q["dg"]], STEP)
    base = _splu_base(q, r)
    for name, a, b in zip(KEYS, new, ref):
        got = a.cpu().numpy()
        e, ei = rel_err(got, b), rel_err(got - base[name], b - base[name])
        print("splu r=%d k=%d %s: state %.2e increment %.2e" % (r, k, name, e, ei))
        assert e < STATE_TOL, (name, e)
        assert ei < INCR_TOL, (name, ei)
    L1, U1 = new[0][:r].cpu().numpy(), new[2][:, :r].cpu().numpy()
    assert np.array_equal(np.triu(L1, 1), np.zeros((r, r))) and np.array_equal(np.tril(U1, -1), np.zeros((r, r)))


@pytest.mark.parametrize("r", SPLU_RANKS)
def test_splu_apply_is_linear_in_g(psgd, r):
    p0 = _splu_problem(r)
    for kg in G_K:
        p = _scaled(p0, g=kg)
        out = psgd.precond_grad_splu(_t(p["L12"]), _t(p["l3"]), _t(p["U12"]), _t(p["u3"]), [_t(p["g"])])[0]
        ref = orc.precond_grad_splu(*(p[a].astype(np.float64) for a in KEYS), [p["g"].astype(np.float64)])[0]
        assert np.isfinite(ref).all() and np.linalg.norm(ref) > 0
        e = rel_err(out.cpu().numpy(), ref)
        assert e < APPLY_TOL, (kg, e)


@pytest.mark.parametrize("r", (7, 32))
@pytest.mark.parametrize("k", SPLU_K)
def test_splu_bf16_state_update_is_scale_free(psgd, r, k):
    """the bf16-stored state, rounding="nearest": every stored code is the nearest code of the fp64 oracle's value (on the widened
    codes) or one of its two neighbours"""
    from tests.test_splu_bf16_gpu import off_by, widen64
    p = _scaled(_splu_problem(r), dx=k, dg=k)
    st = [_t(p[a]).bfloat16() for a in KEYS]
    new = orc.update_precond_splu(*[widen64(s) for s in st], [p["dx"].astype(np.float64)], [p["dg"].astype(np.float64)], STEP)
    out = psgd.update_precond_splu(*st, [_t(p["dx"])], [_t(p["dg"])], STEP)
    assert all(o.dtype == torch.bfloat16 and o.shape == s.shape for o, s in zip(out, st))
    d = off_by(out, new)
    print("splu-bf16 r=%d k=%d: share of neighbour codes %.3e" % (r, k, float((d != 0).mean())))
    assert d.max() <= 1, (r, k, int(d.max()))
