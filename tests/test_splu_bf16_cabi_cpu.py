"""The C ABI and the host refusals of the bf16-stored sparse-LU state (psgd_splu_bf16.hip): exported with the header's
signatures, bound, argument checks that return before any HIP call, and a host layer that refuses what the kernels do not
take before anything is written.  The arithmetic is checked on the GPU in test_splu_bf16_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

from psgd_tf_amd import _lib

NAMES = ("psgd_splu_bf16_workspace_bytes", "psgd_splu_apply_bf16", "psgd_splu_update_bf16")
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
    assert lib.psgd_abi_version() == 7             # new symbols only: the version other tests pin stays


def test_signatures_match_the_header():
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
    assert "no existing layout changes" in text


def test_workspace_bytes(lib):
    ws = lib.psgd_splu_bf16_workspace_bytes
    for r in (1, 7, 10, 20, 32):
        sizes = [ws(n, r) for n in (r, r + 1, 777, 65536, 50_000_000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert max(sizes) < 4 << 20                # block partials only: no N-sized temporary
    assert ws(100, 33) == _lib.PSGD_ERR_RANK and ws(100, 64) == _lib.PSGD_ERR_RANK
    assert ws(100, 0) == _lib.PSGD_ERR_BAD_ARG and ws(100, -1) == _lib.PSGD_ERR_BAD_ARG
    assert ws(9, 10) == _lib.PSGD_ERR_BAD_ARG


def test_argument_checks(lib):
    BAD, RANK, WS, ALIGN = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_RANK, _lib.PSGD_ERR_WORKSPACE, _lib.PSGD_ERR_ALIGN
    # never dereferenced: the checks fail first.  1 MiB apart: no two buffers of the shapes below overlap
    L, l3, U, u3, dx, dg, Lo, l3o, Uo, u3o, g, out, ws = (0x100000 * k for k in range(1, 14))
    N, r = 1000, 10
    need = lib.psgd_splu_bf16_workspace_bytes(N, r)
    app, upd = lib.psgd_splu_apply_bf16, lib.psgd_splu_update_bf16
    tail = (ws, need, None)
    assert app(L, l3, U, u3, g, out, N, 0, *tail) == BAD
    assert app(L, l3, U, u3, g, out, N, 33, *tail) == RANK
    assert app(L, l3, U, u3, g, out, 9, 10, *tail) == BAD                      # N < r
    assert app(None, l3, U, u3, g, out, N, r, *tail) == BAD
    assert app(L, None, U, u3, g, out, N, r, *tail) == BAD                     # a tail needs l3
    assert app(L, l3, U, u3, g, None, N, r, *tail) == BAD
    assert app(L, l3, U, u3, g, g, N, r, *tail) == BAD
    assert app(L + 2, l3, U, u3, g, out, N, r, *tail) == ALIGN
    assert app(L, l3, U + 8, u3, g, out, N, r, *tail) == ALIGN
    assert app(L, l3 + 4, U, u3, g, out, N, r, *tail) == ALIGN
    assert app(L, l3, U, u3, g, out, N, r, None, need, None) == WS
    assert app(L, l3, U, u3, g, out, N, r, ws, need - 1, None) == WS
    assert app(L, l3, U, u3, g, out, N, r, ws + 16, need, None) == WS
    u = lambda *a, N=N, r=r, rounding=0, tail=tail: upd(*a, N, r, 0.01, 1e-38, rounding, 0, *tail)
    ok = (L, l3, U, u3, dx, dg, Lo, l3o, Uo, u3o)
    assert u(*ok, r=0) == BAD
    assert u(*ok, r=33) == RANK
    assert u(*ok, N=9) == BAD
    assert u(*ok, rounding=2) == BAD and u(*ok, rounding=-1) == BAD
    assert u(L, l3, U, u3, None, dg, Lo, l3o, Uo, u3o) == BAD
    assert u(L, l3, U, u3, dx, dg, None, l3o, Uo, u3o) == BAD
    assert u(L, l3, U + 2, u3, dx, dg, Lo, l3o, Uo, u3o) == ALIGN
    assert u(L, l3, U, u3, dx, dg, Lo, l3o, Uo, u3o + 6) == ALIGN
    assert u(L, l3, U, u3, dx, dg, L, l3o, Uo, u3o) == BAD                     # the update is pure: no aliasing
    assert u(L, l3, U, u3, dx, dg, Lo, l3, Uo, u3o) == BAD
    assert u(L, l3, U, u3, dx, dg, Lo, l3o, U + 16, u3o) == BAD                # overlapping, not only equal
    assert u(*ok, tail=(ws, need - 256, None)) == WS
    assert u(*ok, tail=(None, need, None)) == WS


def _cpu_state(N=40, r=5, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.randn(*s, generator=g).to(dtype)
    return [mk(N, r), mk(N - r, 1), mk(r, N), mk(N - r, 1)], torch.randn(N, 1, generator=g), torch.randn(N, 1, generator=g)


def _refusals(update, apply):
    """every refusal names its error type and leaves every tensor as it was (CPU tensors: nothing can have been launched)"""
    cases = []
    st, dx, dg = _cpu_state()
    st[1] = st[1].float()
    cases.append((st, dx, dg, TypeError, "mixed"))
    st, dx, dg = _cpu_state()
    st[2] = st[2].half()
    cases.append((st, dx, dg, TypeError, "float16"))
    st, dx, dg = _cpu_state(dtype=torch.float16)
    cases.append((st, dx, dg, TypeError, "float16"))
    st, dx, dg = _cpu_state(N=80, r=33)
    cases.append((st, dx, dg, ValueError, "32"))
    for st, dx, dg, err, msg in cases:
        before = [t.clone() for t in st + [dx, dg]]
        with pytest.raises(err, match=msg):
            update(*st, [dx], [dg])
        with pytest.raises(err, match=msg):
            apply(*st, [dg])
        for a, b in zip(before, st + [dx, dg]):
            assert a.dtype == b.dtype and torch.equal(a, b)


def test_host_refusals_change_nothing():
    import preconditioned_stochastic_gradient_descent as psgd
    _refusals(lambda *a: psgd.update_precond_splu(*a, 0.01), psgd.precond_grad_splu)
    st, dx, dg = _cpu_state(dtype=torch.float32)
    before = [t.clone() for t in st]
    for kw in ({"rounding": "stochastic"}, {"rounding_seed": 5}, {"rounding": "nearest", "rounding_seed": 0}):
        with pytest.raises(ValueError, match="bfloat16 state only"):
            psgd.update_precond_splu(*st, [dx], [dg], 0.01, **kw)
    with pytest.raises(ValueError, match="rounding must be"):
        psgd.update_precond_splu(*_cpu_state()[0], [dx], [dg], 0.01, rounding="up")
    assert all(torch.equal(a, b) for a, b in zip(before, st))
    # an fp32 state on the CPU is still what it was: refused by the device check, not by a dtype rule
    with pytest.raises(_lib.PsgdHipError, match="HIP device only"):
        psgd.update_precond_splu(*st, [dx], [dg], 0.01)
    with pytest.raises(_lib.PsgdHipError, match="HIP device only"):
        psgd.update_precond_splu(*_cpu_state()[0], [dx], [dg], 0.01)


def test_sharded_refuses_a_bf16_state():
    from psgd_tf_amd import sharded
    _refusals(lambda L, l, U, u, dx, dg: sharded.update_precond_splu(L, l, U, u, dx[0], dg[0]),
              lambda L, l, U, u, g: sharded.precond_grad_splu(L, l, U, u, g[0]))
    st, dx, dg = _cpu_state()
    before = [t.clone() for t in st]
    with pytest.raises(ValueError, match="not row-sharded"):
        sharded.update_precond_splu(*st, dx, dg)
    with pytest.raises(ValueError, match="not row-sharded"):
        sharded.precond_grad_splu(*st, dg)
    assert all(torch.equal(a, b) for a, b in zip(before, st))
