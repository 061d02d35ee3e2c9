"""psgd_xmat.hip against the float64 restatement: the middle element, all residues mod 4, quads where the runs meet (4, 20), one
workgroup's trip T - 1 .. 2T + 1, the second trip of the grid-stride loop (GRID * T + 3); fused == update-then-apply, bit for bit."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib
from tests.xmat_cases import (APPLY_BAR, GRID, INCREMENT_BAR, STATE_BAR, STEP, T, TINY32, err, problem, xmat_apply_ref,
                              xmat_update_ref)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 20, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, GRID * T + 3]
CASES = [(n, False) for n in NS] + [(n, True) for n in (1, 5, 8, 2 * T + 1)]


def _dev(p, diagonal, *keys):
    return [None if (k == "b" and diagonal) else p[k].to(DEV) for k in keys]


@pytest.mark.parametrize("N, diagonal", CASES)
def test_update_apply_and_fused_match_fp64(N, diagonal):
    p = problem(N, diagonal)
    a, b, v, h, g = _dev(p, diagonal, *"abvhg")
    assert err(psgd.precond_grad_Xmat_math(a, b, g), p["out"]) < APPLY_BAR
    psgd.update_precond_Xmat_math_(a, b, v, h, STEP, TINY32)
    out = psgd.precond_grad_Xmat_math(a, b, g)
    for new, old, ref in [(a, p["a"], p["new_a"])] + ([] if diagonal else [(b, p["b"], p["new_b"])]):
        e_state, e_inc = err(new, ref), err(new.cpu() - old, ref - old.double())
        print("N=%d diagonal=%s: state %.2e increment %.2e" % (N, diagonal, e_state, e_inc))
        assert e_state < STATE_BAR and e_inc < INCREMENT_BAR
    assert err(out, p["out_new"]) < APPLY_BAR
    a2, b2 = _dev(p, diagonal, *"ab")
    out2 = psgd.update_precond_grad_Xmat_math_(a2, b2, v, h, g, STEP, TINY32)
    assert torch.equal(a2, a) and torch.equal(out2, out) and (diagonal or torch.equal(b2, b))


@pytest.mark.parametrize("N", [17, 2 * T])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_nan_in_h_reaches_what_the_restatement_gives(N, where):
    p = problem(N)
    h = p["h"].clone()
    h[{"first": 0, "middle": (N - 1) // 2, "last": N - 1}[where]] = float("nan")
    a, b, v, g = _dev(p, False, *"abvg")
    out = psgd.update_precond_grad_Xmat_math_(a, b, v, h.to(DEV), g, STEP, TINY32)
    ra, rb = xmat_update_ref(p["a"].double(), p["b"].double(), p["v"].double(), h.double())
    for got, ref in ((a, ra), (b, rb), (out, xmat_apply_ref(ra, rb, p["g"].double()))):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(ref)) and bool(torch.isnan(ref).any())


@pytest.mark.parametrize("N", [17, 2 * T])
def test_zero_v_and_h_leave_the_state_bit_for_bit(N):
    p = problem(N)
    a, b = _dev(p, False, *"ab")
    zero = torch.zeros(N, device=DEV)
    psgd.update_precond_Xmat_math_(a, b, zero, zero, STEP, TINY32)
    assert torch.equal(a.cpu(), p["a"]) and torch.equal(b.cpu(), p["b"])


def test_out_aliasing_g_and_a_matrix_g_are_refused():
    a, b, v, h, g = _dev(problem(17), False, *"abvhg")
    with pytest.raises(_lib.PsgdHipError):
        psgd.precond_grad_Xmat_math(a, b, g, out=g)
    with pytest.raises(_lib.PsgdHipError):
        psgd.update_precond_grad_Xmat_math_(a, b, v, h, g, STEP, TINY32, out=g)
    with pytest.raises(ValueError, match="not a matrix"):
        psgd.precond_grad_Xmat_math(a, b, torch.ones(17, 2, device=DEV))
    assert torch.equal(g.cpu(), problem(17)["g"])
