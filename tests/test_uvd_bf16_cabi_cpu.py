"""The C ABI of the bf16-stored UVd state (psgd_uvd_bf16.hip): exported with the header's signatures, bound, and its
argument checks return before any HIP call.  The arithmetic is checked on the GPU in test_uvd_bf16_gpu.py."""
import ctypes
import os
import re

import pytest

from psgd_tf_amd import _lib

NAMES = ("psgd_uvd_bf16_workspace_bytes", "psgd_uvd_bf16_rounding_key", "psgd_uvd_apply_bf16", "psgd_uvd_update_bf16", "psgd_uvd_update_apply_bf16")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def test_exports_are_bound(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.psgd_abi_version() == 7


def test_signatures_match_the_header():
    """argument count and the scalar types of every new declaration against the ctypes table"""
    text = open(HEADER).read()
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    for name in NAMES:
        m = re.search(r"(uint64_t|int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is kinds[m.group(1)], name
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is ctypes.c_void_p, (name, p)
            else:
                assert t is kinds[p.split()[0]], (name, p)


def test_workspace_bytes(lib):
    ws = lib.psgd_uvd_bf16_workspace_bytes
    for r in (1, 7, 20, 32):
        sizes = [ws(n, r) for n in (1, 5, 777, 65536, 1 << 20, 100_000_000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        assert sizes[-1] >= 4 * 100_000_000          # the N-float nablaD temporary
    assert ws(0, 10) == _lib.PSGD_ERR_BAD_ARG and ws(-1, 10) == _lib.PSGD_ERR_BAD_ARG
    assert ws(100, 0) == _lib.PSGD_ERR_BAD_ARG and ws(100, -2) == _lib.PSGD_ERR_BAD_ARG
    assert ws(100, 33) == _lib.PSGD_ERR_RANK and ws(100, 64) == _lib.PSGD_ERR_RANK


def test_argument_checks(lib):
    BAD, RANK, WS, ALIGN = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_RANK, _lib.PSGD_ERR_WORKSPACE, _lib.PSGD_ERR_ALIGN
    U, V, d, v, h, g, out, ws = (0x10000 * k for k in range(1, 9))      # never dereferenced: the checks fail first
    need = lib.psgd_uvd_bf16_workspace_bytes(1000, 10)
    app, upd, fus = lib.psgd_uvd_apply_bf16, lib.psgd_uvd_update_bf16, lib.psgd_uvd_update_apply_bf16
    assert app(None, V, d, g, out, 1000, 10, ws, need, None) == BAD
    assert app(U, V, d, g, out, 0, 10, ws, need, None) == BAD
    assert app(U, V, d, g, out, 1000, 33, ws, need, None) == RANK
    assert app(U, V, d, g, g, 1000, 10, ws, need, None) == BAD
    assert app(U + 2, V, d, g, out, 1000, 10, ws, need, None) == ALIGN      # a bf16 row is 2r bytes: the BASE must be 16-byte aligned
    assert app(U, V, d + 8, g, out, 1000, 10, ws, need, None) == ALIGN
    assert app(U, V, d, g, out, 1000, 10, None, need, None) == WS
    assert app(U, V, d, g, out, 1000, 10, ws, need - 1, None) == WS
    assert app(U, V, d, g, out, 1000, 10, ws + 16, need, None) == WS
    tail = (ws, need, None)
    assert upd(U, V, d, v, h, 1000, 10, 0.01, 1e-38, 0, 1, 2, 0, *tail) == BAD          # rounding outside {0, 1}
    assert upd(U, V, d, v, h, 1000, 10, 0.01, 1e-38, 0, 1, -1, 0, *tail) == BAD
    assert upd(U, V, d, v, h, 1000, 40, 0.01, 1e-38, 0, 1, 0, 0, *tail) == RANK
    assert upd(U, V, d, None, h, 1000, 10, 0.01, 1e-38, 0, 1, 0, 0, *tail) == BAD
    assert upd(U, V + 4, d, v, h, 1000, 10, 0.01, 1e-38, 0, 1, 0, 0, *tail) == ALIGN
    assert upd(U, V, d, v, h, 1000, 10, 0.01, 1e-38, 0, 1, 1, 7, ws, need - 256, None) == WS
    assert fus(U, V, d, v, h, g, out, 1000, 10, 0.01, 1e-38, 0, 1, 3, 0, *tail) == BAD
    assert fus(U, V, d, v, h, g, None, 1000, 10, 0.01, 1e-38, 0, 1, 0, 0, *tail) == BAD
    assert fus(U, V, d, v, h, g, g, 1000, 10, 0.01, 1e-38, 0, 1, 0, 0, *tail) == BAD
    assert fus(U, V, d, v, h, g, out, 1000, 33, 0.01, 1e-38, 0, 1, 0, 0, *tail) == RANK
    assert fus(U, V, d, v, h, g, out, 1000, 10, 0.01, 1e-38, 0, 1, 0, 0, None, need, None) == WS


def test_rounding_streams_do_not_alias(lib):
    """The key of a tensor's stochastic-rounding stream (0 = U, 1 = V, 2 = d): distinct over the steps of a class UVd run and the three
    tensors -- in particular key(step k, d) != key(step k + 1, V) != key(step k + 2, U), which an additive derivation of both the step
    seed and the tensor key would make equal -- and over seeds in arithmetic progression with the golden-ratio increment."""
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import uvd_step_rounding_seed
    key = lib.psgd_uvd_bf16_rounding_key
    G = 0x9E3779B97F4A7C15
    for seed0 in (0, 1, 0x50534744, 2 ** 62 - 1):
        seeds = [uvd_step_rounding_seed(seed0, k) for k in range(200)]
        assert len(set(seeds)) == len(seeds) and all(0 <= s < 2 ** 64 for s in seeds)
        keys = {(k, t): key(seeds[k], t) for k in range(200) for t in range(3)}
        assert len(set(keys.values())) == len(keys)
        for k in range(198):
            assert len({keys[(k, 2)], keys[(k + 1, 1)], keys[(k + 2, 0)]}) == 3
        plain = {(j, t): key((seed0 + G * j) % 2 ** 64, t) for j in range(200) for t in range(3)}      # a caller's own additive seeds
        assert len(set(plain.values())) == len(plain)
        # both 32-bit halves feed the element hash: neither may collide between neighbouring streams
        for k in range(198):
            trio = (keys[(k, 2)], keys[(k + 1, 1)], keys[(k + 2, 0)])
            assert len({x & 0xFFFFFFFF for x in trio}) == 3 and len({x >> 32 for x in trio}) == 3
