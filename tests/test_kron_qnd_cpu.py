"""include/psgd_kron_quad_nd_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, the class
switch's refusals, kron_layers with and without it."""
import ctypes
import os
import re

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, kron_quad_nd

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_kron_quad_nd_hip.h")


def test_header_symbols_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psgd_kron_qnd_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(kron_quad_nd.SIGNATURES) and len(declared) == 3
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), kron_quad_nd.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == kron_quad_nd.SIGNATURES[n][1] for n in declared)
    assert not set(declared) & set(_lib.SIGNATURES)
    assert _lib.PSGD_ABI_VERSION == 7 == lib.psgd_abi_version()
    for name in ("kron_quad_nd_initial_state", "update_precond_kron_quad_nd_", "precond_grad_kron_quad_nd"):
        assert getattr(psgd, name) is getattr(kron_quad_nd, name)


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS = kron_quad_nd.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    Qa, Qb, Qc, L, G, out, ws = (0x10000 * k for k in range(1, 8))       # never dereferenced: the checks fail first
    A, B, C = 70, 5, 9
    need = lib.psgd_kron_qnd_workspace_bytes(A, B, C)
    for shape in ((0, 5, 9), (70, -1, 9), (70, 5, 0), (2048, 2048, 512)):  # (the last: A B C = 2^31)
        assert lib.psgd_kron_qnd_workspace_bytes(*shape) == BAD
        assert lib.psgd_kron_qnd_apply_f32(Qa, Qb, Qc, G, out, *shape, ws, need, None) == BAD
        assert lib.psgd_kron_qnd_update_f32(Qa, Qb, Qc, L, G, *shape, 0.1, 0.95, ws, need, None) == BAD
    for args in ((None, Qb, Qc, G, out), (Qa, None, Qc, G, out), (Qa, Qb, None, G, out), (Qa, Qb, Qc, None, out), (Qa, Qb, Qc, G, None),
                 (Qa, Qb, Qc, G, G), (Qa, Qb, Qc, G, Qa), (Qa, Qb, Qc, G, Qb), (Qa, Qb, Qc, G, Qc)):
        assert lib.psgd_kron_qnd_apply_f32(*args, A, B, C, ws, need, None) == BAD
    for args in ((None, Qb, Qc, L, G), (Qa, None, Qc, L, G), (Qa, Qb, None, L, G), (Qa, Qb, Qc, None, G), (Qa, Qb, Qc, L, None),
                 (Qa, Qa, Qc, L, G), (Qa, Qb, Qa, L, G), (Qa, Qb, Qb, L, G), (Qa, Qb, Qc, L, Qb), (Qa, Qb, Qc, Qc, G), (Qa, Qb, Qc, G, G)):
        assert lib.psgd_kron_qnd_update_f32(*args, A, B, C, 0.1, 0.95, ws, need, None) == BAD
    for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
        assert lib.psgd_kron_qnd_apply_f32(Qa, Qb, Qc, G, out, A, B, C, *bad_ws, None) == WS
        assert lib.psgd_kron_qnd_update_f32(Qa, Qb, Qc, L, G, A, B, C, 0.1, 0.95, *bad_ws, None) == WS


@pytest.mark.parametrize("kw", [dict(any_rank=True), dict(preconditioner_update="quad", preconditioner_fit="whitening"),
                                dict(any_rank=True, preconditioner_fit="whitening")])
def test_class_switch_refusals_before_a_device_is_touched(kw):
    with pytest.raises(ValueError, match="quad_tensor"):
        psgd.Kron([torch.zeros(6, 5, 3, 3, requires_grad=True)], quad_tensor=True, **kw)


def test_kron_layers_with_and_without_the_switch():
    shapes = [(6, 5, 3, 3), (5, 7), (7,), (4, 3, 2), ()]
    folded = [("matrix", (6, 45), ("dense", "dense")), ("matrix", (5, 7), ("dense", "dense")), ("vector", (1, 7), ("dense", "scale")),
              ("matrix", (4, 6), ("dense", "dense")), ("scalar", (1, 1), ("dense", "dense"))]
    assert psgd.kron_layers(shapes, "dense", True) == psgd.kron_layers(shapes, "dense", True, False) == folded
    on = psgd.kron_layers(shapes, "dense", True, True)
    assert on[0] == ("tensor", (6, 5, 9), ("dense", "dense")) and on[3] == ("tensor", (4, 3, 2), ("dense", "dense"))
    assert [on[i] for i in (1, 2, 4)] == [folded[i] for i in (1, 2, 4)]
    assert psgd.kron_layers(shapes[:2], [("dense", "scale"), "dense"], True, True)[0] == ("matrix", (6, 45), ("dense", "scale"))
