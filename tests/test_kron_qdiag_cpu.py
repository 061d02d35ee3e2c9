"""include/psgd_kron_quad_diag_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, the Python
refusals, and the float32 restatement on the inputs of tests/test_kron_qdiag_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, kron_quad, kron_quad_diag as qd
from tests import test_kron_qdiag_gpu as cases

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_kron_quad_diag_hip.h")


def test_header_symbols_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psgd_kron_qdiag_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(qd.SIGNATURES) and len(declared) == 4
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), qd.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == qd.SIGNATURES[n][1] for n in declared)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(kron_quad.SIGNATURES))


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS = qd.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    Ql, Qr, L, G, out, ws = (0x10000 * k for k in range(1, 7))          # never dereferenced: the checks fail first
    need = lib.psgd_kron_qdiag_workspace_bytes(1000, 5, 0)
    assert need > 4 * (1000 * 5 + 2 * 5 * 5 + 1000) + 8 * 1000
    for bad in ((0, 5, 0), (5, -1, 1), (5, 5, 2), (5, 5, -1)):
        assert lib.psgd_kron_qdiag_workspace_bytes(*bad) == BAD and lib.psgd_kron_qdiag_slices(*bad) == BAD
    # S is a function of the shape alone: the header's rule, evaluated here
    for D, n in cases.CASES + [(32768, 1024), (131072, 1024), (131072, 8192), (4096, 64)]:
        upper = -(-n // 64) * (-(-n // 64) + 1) // 2
        steps = -(-D // 16)
        per = -(-steps // max(1, min(-(-1024 // upper), -(-D // 256))))
        assert lib.psgd_kron_qdiag_slices(D, n, 0) == lib.psgd_kron_qdiag_slices(n, D, 1) == -(-steps // per), (D, n)
    for args in ((None, Qr, G, out, 1000, 5, 0), (Ql, None, G, out, 1000, 5, 0), (Ql, Qr, None, out, 1000, 5, 0),
                 (Ql, Qr, G, None, 1000, 5, 0), (Ql, Qr, G, out, 0, 5, 0), (Ql, Qr, G, out, 1000, 0, 0), (Ql, Qr, G, out, 1000, 5, 2),
                 (Ql, Qr, G, G, 1000, 5, 0), (Ql, Qr, G, Ql, 1000, 5, 0), (Ql, Qr, G, Qr, 1000, 5, 0)):
        assert lib.psgd_kron_qdiag_apply_f32(*args, ws, need, None) == BAD
    for args in ((None, Qr, L, G, 1000, 5, 0), (Ql, None, L, G, 1000, 5, 0), (Ql, Qr, None, G, 1000, 5, 0), (Ql, Qr, L, None, 1000, 5, 0),
                 (Ql, Qr, L, G, 1000, -1, 0), (Ql, Qr, L, G, 1000, 5, -1), (Ql, Ql, L, G, 1000, 5, 0), (Ql, Qr, L, Ql, 1000, 5, 0),
                 (Ql, Qr, Qr, G, 1000, 5, 0)):
        assert lib.psgd_kron_qdiag_update_f32(*args, 0.1, 0.95, ws, need, None) == BAD
    for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
        assert lib.psgd_kron_qdiag_apply_f32(Ql, Qr, G, out, 1000, 5, 0, *bad_ws, None) == WS
        assert lib.psgd_kron_qdiag_update_f32(Ql, Qr, L, G, 1000, 5, 0, 0.1, 0.95, *bad_ws, None) == WS


def test_python_refusals():
    ql, Qr, L = psgd.kron_quad_initial_state(3, 5, formats=("scale", "dense"))
    assert tuple(ql.shape) == (1, 3) and tuple(Qr.shape) == (5, 5)
    G = torch.zeros(3, 5)
    with pytest.raises(ValueError, match="both scale factors"):
        psgd.precond_grad_kron_quad(ql, torch.ones(1, 5), G)
    with pytest.raises(ValueError, match="both scale factors"):
        psgd.update_precond_kron_quad_(ql, torch.ones(1, 5), L, G, 0.1)
    with pytest.raises(TypeError, match="Ql"):
        psgd.precond_grad_kron_quad(ql.double(), Qr, G)
    with pytest.raises(ValueError, match="Qr"):
        psgd.update_precond_kron_quad_(ql, torch.eye(4), L, G, 0.1)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        psgd.update_precond_kron_quad_(ql, Qr, L, G, 0.1)
    with pytest.raises(ValueError, match="formats"):
        psgd.kron_quad_initial_state(3, 5, formats=("scale", "scale"))
    for kw in (dict(), dict(preconditioner_fit="whitening")):
        with pytest.raises(ValueError, match="quad_diagonal"):
            psgd.Kron([torch.zeros(3, 5, requires_grad=True)], quad_diagonal=True, **kw)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("D, n", cases.CASES)
def test_float32_restatement_holds_the_bars(D, n, side):
    """A case on which fp32 arithmetic itself misses a bar is a wrong case, not a kernel bug (problem() asserts the tie rule)."""
    p = cases.problem(D, n, side)
    q, Q, G = p["q"][0], p["Q"], p["G"]
    new_q, new_Q, new_L = cases.ref_update(side, q, Q, p["L"], G)
    assert new_q.dtype == torch.float32
    cases.assert_bars(cases.errors(p, cases.ref_apply(side, q, Q, G), new_q[None, :], new_Q, new_L,
                                   cases.ref_apply(side, new_q, new_Q, G)), (D, n, side))
