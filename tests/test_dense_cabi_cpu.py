"""The dense preconditioner's C ABI (psgd_dense.hip): exported, bound, and its argument checks return before any HIP call.
No compute calls here; the arithmetic is checked on the GPU in test_dense_gpu.py."""
import ctypes

import pytest

from psgd_tf_amd import _lib

NAMES = ("psgd_dense_workspace_bytes", "psgd_dense_update_f32", "psgd_dense_apply_f32")


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def test_exports_are_bound(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).restype is not None


def test_workspace_grows_with_n(lib):
    ws = lib.psgd_dense_workspace_bytes
    sizes = [ws(n) for n in (1, 65, 400, 4096, 46400)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert all(ws(n + 1) >= ws(n) for n in range(1, 300))
    assert sizes[-1] >= 2 * 4 * 725 * 46400        # two [ceil(N / 64)][N] fp32 planes of column partials
    assert ws(0) == _lib.PSGD_ERR_BAD_ARG and ws(-5) == _lib.PSGD_ERR_BAD_ARG


def test_argument_checks(lib):
    BAD, WS = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    upd, app = lib.psgd_dense_update_f32, lib.psgd_dense_apply_f32
    Q, dx, dg, out, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # never dereferenced: the checks fail first
    need = lib.psgd_dense_workspace_bytes(100)
    for args in ((None, dx, dg, out), (Q, None, dg, out), (Q, dx, None, out), (Q, dx, dg, None)):
        assert upd(*args, 100, 0.01, 1e-38, ws, need, None) == BAD
    assert upd(Q, dx, dg, out, 0, 0.01, 1e-38, ws, need, None) == BAD
    assert upd(Q, dx, dg, out, -3, 0.01, 1e-38, ws, need, None) == BAD
    assert upd(Q, dx, dg, Q, 100, 0.01, 1e-38, ws, need, None) == BAD        # the update is pure: no in-place form
    assert upd(Q, dx, dg, out, 100, 0.01, 1e-38, None, need, None) == WS
    assert upd(Q, dx, dg, out, 100, 0.01, 1e-38, ws, need - 1, None) == WS
    assert upd(Q, dx, dg, out, 100, 0.01, 1e-38, ws + 4, need, None) == WS    # not 256-byte aligned
    for args in ((None, dx, out), (Q, None, out), (Q, dx, None)):
        assert app(*args, 100, ws, need, None) == BAD
    assert app(Q, dx, out, 0, ws, need, None) == BAD
    assert app(Q, dx, out, 100, None, need, None) == WS
    assert app(Q, dx, out, 100, ws, need - 256, None) == WS
