"""include/psgd_kron_quad_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, class refusals."""
import ctypes
import os
import re

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, kron_quad
from tests import kron_quad_cases as qc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_kron_quad_hip.h")


def test_header_symbols_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psgd_kron_quad_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(kron_quad.SIGNATURES) and len(declared) == 3
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), kron_quad.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == kron_quad.SIGNATURES[n][1] for n in declared)
    assert not set(declared) & set(_lib.SIGNATURES)
    assert int(re.search(r"#define\s+PSGD_KRON_QUAD_TILE\s+(\d+)", text).group(1)) == kron_quad.KRON_QUAD_TILE == qc.T


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS = kron_quad.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    Ql, Qr, L, G, out, ws = (0x10000 * k for k in range(1, 7))          # never dereferenced: the checks fail first
    need = lib.psgd_kron_quad_workspace_bytes(70, 5)
    assert need > 4 * (2 * 70 * 5 + 2 * 70 * 70 + 2 * 5 * 5)
    assert lib.psgd_kron_quad_workspace_bytes(0, 5) == BAD and lib.psgd_kron_quad_workspace_bytes(5, -1) == BAD
    for args in ((None, Qr, G, out, 70, 5), (Ql, None, G, out, 70, 5), (Ql, Qr, None, out, 70, 5), (Ql, Qr, G, None, 70, 5),
                 (Ql, Qr, G, out, 0, 5), (Ql, Qr, G, out, 70, 0), (Ql, Qr, G, G, 70, 5), (Ql, Qr, G, Ql, 70, 5), (Ql, Qr, G, Qr, 70, 5)):
        assert lib.psgd_kron_quad_apply_f32(*args, ws, need, None) == BAD
    for args in ((None, Qr, L, G, 70, 5), (Ql, None, L, G, 70, 5), (Ql, Qr, None, G, 70, 5), (Ql, Qr, L, None, 70, 5),
                 (Ql, Qr, L, G, 70, -1), (Ql, Ql, L, G, 70, 5), (Ql, Qr, L, Ql, 70, 5), (Ql, Qr, Qr, G, 70, 5)):
        assert lib.psgd_kron_quad_update_f32(*args, 0.1, 0.95, ws, need, None) == BAD
    for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
        assert lib.psgd_kron_quad_apply_f32(Ql, Qr, G, out, 70, 5, *bad_ws, None) == WS
        assert lib.psgd_kron_quad_update_f32(Ql, Qr, L, G, 70, 5, 0.1, 0.95, *bad_ws, None) == WS


def test_functions_refuse_bad_operands_by_name():
    Ql, Qr, L = psgd.kron_quad_initial_state(3, 5)
    G = torch.zeros(3, 5)
    with pytest.raises(ValueError, match="Qr"):
        psgd.precond_grad_kron_quad(Ql, Ql, G)
    with pytest.raises(TypeError, match="Ql"):
        psgd.precond_grad_kron_quad(Ql.double(), Qr, G)
    with pytest.raises(ValueError, match="L "):
        psgd.update_precond_kron_quad_(Ql, Qr, torch.zeros(3), G, 0.1)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        psgd.update_precond_kron_quad_(Ql, Qr, L, G, 0.1)


@pytest.mark.parametrize("kw", [dict(preconditioner_update="quad"), dict(preconditioner_update="qr", preconditioner_fit="whitening"),
                                dict(preconditioner_update="quad", preconditioner_fit="whitening", operands="bfloat16")])
def test_class_refusals_before_a_device_is_touched(kw):
    with pytest.raises(ValueError, match="preconditioner_update"):
        psgd.Kron([torch.zeros(3, 5, requires_grad=True)], **kw)
