"""include/psgd_kron_quad_x3_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, the refusals
of products= and quad_products=, and the tie condition of the shapes tests/test_kron_quad_x3_gpu.py adds."""
import ctypes
import os
import re

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, kron_quad, kron_quad_diag, kron_quad_list, kron_quad_x3
from tests import kron_quad_cases as qc
from tests import test_kron_quad_x3_gpu as gpu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_kron_quad_x3_hip.h")


def test_header_symbols_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psgd_kron_quad_x3_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(kron_quad_x3.SIGNATURES) and len(declared) == 3
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), kron_quad_x3.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == kron_quad_x3.SIGNATURES[n][1] for n in declared)
    others = (_lib.SIGNATURES, kron_quad.SIGNATURES, kron_quad_diag.SIGNATURES, kron_quad_list.SIGNATURES)
    assert not any(set(declared) & set(t) for t in others)
    assert lib.psgd_abi_version() == _lib.PSGD_ABI_VERSION == 7


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS = kron_quad_x3.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    Ql, Qr, L, G, out, ws = (0x10000 * k for k in range(1, 7))          # never dereferenced: the checks fail first
    need = lib.psgd_kron_quad_x3_workspace_bytes(70, 5)
    assert need == kron_quad.load().psgd_kron_quad_workspace_bytes(70, 5)    # state AND workspace are the fp32 route's
    assert lib.psgd_kron_quad_x3_workspace_bytes(0, 5) == BAD and lib.psgd_kron_quad_x3_workspace_bytes(5, -1) == BAD
    for args in ((None, Qr, G, out, 70, 5), (Ql, None, G, out, 70, 5), (Ql, Qr, None, out, 70, 5), (Ql, Qr, G, None, 70, 5),
                 (Ql, Qr, G, out, 0, 5), (Ql, Qr, G, out, 70, 0), (Ql, Qr, G, G, 70, 5), (Ql, Qr, G, Ql, 70, 5), (Ql, Qr, G, Qr, 70, 5)):
        assert lib.psgd_kron_quad_x3_apply_f32(*args, ws, need, None) == BAD
    for args in ((None, Qr, L, G, 70, 5), (Ql, None, L, G, 70, 5), (Ql, Qr, None, G, 70, 5), (Ql, Qr, L, None, 70, 5),
                 (Ql, Qr, L, G, 70, -1), (Ql, Ql, L, G, 70, 5), (Ql, Qr, L, Ql, 70, 5), (Ql, Qr, Qr, G, 70, 5)):
        assert lib.psgd_kron_quad_x3_update_f32(*args, 0.1, 0.95, ws, need, None) == BAD
    for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
        assert lib.psgd_kron_quad_x3_apply_f32(Ql, Qr, G, out, 70, 5, *bad_ws, None) == WS
        assert lib.psgd_kron_quad_x3_update_f32(Ql, Qr, L, G, 70, 5, 0.1, 0.95, *bad_ws, None) == WS


def test_functions_refuse_products_by_name():
    Ql, Qr, L = psgd.kron_quad_initial_state(3, 5)
    G = torch.zeros(3, 5)
    for products in ("bf16", None):
        with pytest.raises(ValueError, match="products"):
            psgd.precond_grad_kron_quad(Ql, Qr, G, products=products)
        with pytest.raises(ValueError, match="products"):
            psgd.update_precond_kron_quad_(Ql, Qr, L, G, 0.1, products=products)
    ql, _, _ = psgd.kron_quad_initial_state(3, 5, formats=("scale", "dense"))
    _, qr, _ = psgd.kron_quad_initial_state(3, 5, formats=("dense", "scale"))
    with pytest.raises(ValueError, match="Ql is a scale factor"):
        psgd.precond_grad_kron_quad(ql, Qr, G, products="bf16x3")
    with pytest.raises(ValueError, match="Qr is a scale factor"):
        psgd.update_precond_kron_quad_(Ql, qr, L, G, 0.1, products="bf16x3")
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):     # judged like the fp32 route's operands
        psgd.update_precond_kron_quad_(Ql, Qr, L, G, 0.1, products="bf16x3")


@pytest.mark.parametrize("kw, match", [
    (dict(preconditioner_update="quad", quad_products="bf16"), "quad_products must be"),
    (dict(quad_products="bf16x3"), "needs preconditioner_update='quad'"),
    (dict(preconditioner_update="quad", quad_products="bf16x3", quad_route="list"), "quad_route='list'")])
def test_class_refusals_before_a_device_is_touched(kw, match):
    with pytest.raises(ValueError, match=match):
        psgd.Kron([torch.zeros(3, 5, requires_grad=True)], preconditioner_fit="whitening", **kw)


def test_added_shapes_hold_the_tie_condition_and_reach_every_k_residue():
    for M, N, seed in gpu.EDGE_CASES:
        qc.problem(M, N, seed)                                              # asserts the condition on both sides
    assert {k % 32 for case in gpu.EDGE_CASES for k in case[:2]} >= {0, 1, 4, 31}
