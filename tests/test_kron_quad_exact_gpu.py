"""psgd_kron_quad.hip on inputs where fp32 arithmetic is exact (tests/kron_quad_cases.py, exact_problem and shift_problem; the
conditions are checked in tests/test_kron_quad_cpu.py): the product core is an fp32 fma chain, so the kernels must give the float64
reference bit for bit, and one wrong element of one edge tile fails.  No tolerance anywhere in this file."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from tests import kron_quad_cases as qc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _wrong(got, ref):
    """'' when equal, else where and by how much the first few elements differ"""
    got = got.double().cpu()
    if torch.equal(got, ref):
        return ""
    at = torch.nonzero(got != ref)
    return "%d wrong element(s), first at %s: %s" % (len(at), at[:4].tolist(), [(float(got[tuple(i)]), float(ref[tuple(i)])) for i in at[:4]])


@pytest.mark.parametrize("M, N, seed", qc.EXACT_CASES)
def test_apply_is_the_float64_reference_bit_for_bit(M, N, seed):
    p = qc.exact_problem(M, N, seed)
    out = psgd.precond_grad_kron_quad(p["Ql"].to(DEV), p["Qr"].to(DEV), p["G"].to(DEV))
    assert torch.equal(out.double().cpu(), p["out"]), _wrong(out, p["out"])


@pytest.mark.parametrize("M, N, seed", qc.EXACT_CASES)
def test_update_is_the_float64_reference_bit_for_bit(M, N, seed):
    p = qc.exact_problem(M, N, seed)
    Ql, Qr, L = (p[k].to(DEV).clone() for k in ("Ql", "Qr", "L"))
    psgd.update_precond_kron_quad_(Ql, Qr, L, p["G"].to(DEV), p["step"], p["decay"])
    assert L.tolist() == [qc.EXACT_L0, qc.EXACT_L0] == p["new_L"].tolist()
    for k, Q in (("Ql", Ql), ("Qr", Qr)):
        assert torch.equal(Q.double().cpu(), p["new_" + k]), k + ": " + _wrong(Q, p["new_" + k])
        assert torch.equal(Q, Q.T)


@pytest.mark.parametrize("M, N, seed, shift", qc.SHIFT_CASES)
def test_apply_with_shift_factors_rotates_rows_and_columns_by_two(M, N, seed, shift):
    """factors that are not symmetric: a transposed operand anywhere in the four products rotates the wrong way"""
    p = qc.shift_problem(M, N, seed, shift)
    out = psgd.precond_grad_kron_quad(p["Ql"].to(DEV), p["Qr"].to(DEV), p["G"].to(DEV))
    assert torch.equal(out.double().cpu(), p["out"]), _wrong(out, p["out"])
