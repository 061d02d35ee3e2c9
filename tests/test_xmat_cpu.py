"""include/psgd_xmat_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, class refusals."""
import ctypes
import os
import re

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, xmat

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_xmat_hip.h")


def test_header_symbols_are_exported_and_bound():
    declared = sorted(set(re.findall(r"\b(psgd_xmat_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))))
    assert declared == sorted(xmat.SIGNATURES) and len(declared) == 4
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), xmat.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == xmat.SIGNATURES[n][1] for n in declared)
    assert not set(declared) & set(_lib.SIGNATURES) and lib.psgd_abi_version() == 7


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS = xmat.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    a, b, v, h, g, out, ws = (0x10000 * k for k in range(1, 8))          # never dereferenced: the checks fail first
    need = lib.psgd_xmat_workspace_bytes(100)
    assert need == 4 * xmat.XMAT_MAX_GRID and lib.psgd_xmat_workspace_bytes(0) == BAD
    for args in ((None, b, g, out, 100), (a, b, None, out, 100), (a, b, g, None, 100), (a, b, g, out, 0), (a, b, g, g, 100),
                 (a, b, g, a, 100)):
        assert lib.psgd_xmat_apply_f32(*args, None) == BAD
    for args in ((None, b, v, h, 100), (a, b, None, h, 100), (a, b, v, None, 100), (a, b, v, h, -1)):
        assert lib.psgd_xmat_update_f32(*args, 0.1, 1e-38, ws, need, None) == BAD
    for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
        assert lib.psgd_xmat_update_f32(a, b, v, h, 100, 0.1, 1e-38, *bad_ws, None) == WS
    for o in (a, b, v, h, g, None):
        assert lib.psgd_xmat_update_apply_f32(a, b, v, h, g, o, 100, 0.1, 1e-38, ws, need, None) == BAD


@pytest.mark.parametrize("kw, exc", [(dict(state_dtype=torch.bfloat16), TypeError), (dict(group=object()), ValueError),
                                     (dict(placement="probe"), ValueError), (dict(diagonal=1), ValueError)])
def test_constructor_refusals(kw, exc):
    with pytest.raises(exc, match="XMat"):
        psgd.XMat([torch.zeros(5, requires_grad=True)], **kw)
