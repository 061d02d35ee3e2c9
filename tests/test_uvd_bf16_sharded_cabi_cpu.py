"""The staged C ABI of the bf16-stored UVd state (row-sharded optimizer): every new symbol is exported with the header's signature
and bound, its argument checks return before any HIP call, and the send regions lie inside the workspace without overlapping.
The arithmetic is checked on the GPU in test_uvd_bf16_sharded_gpu.py."""
import ctypes
import os
import re

import pytest

from psgd_tf_amd import _lib

NAMES = ("psgd_uvd_bf16_ws_region", "psgd_uvd_bf16_fold_gathered_f64", "psgd_uvd_balance_max_bf16", "psgd_uvd_update_gram_bf16",
         "psgd_uvd_update_rewrite_bf16", "psgd_uvd_update_d_bf16", "psgd_uvd_apply_sweep1_bf16", "psgd_uvd_apply_sweep1_d_bf16",
         "psgd_uvd_apply_sweep2_bf16", "psgd_uvd_apply_sweep3_bf16")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")
STAGES = (10, 11, 12, 1, 2)


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
    assert lib.psgd_abi_version() == 7                      # additive exports: the version does not move


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
                assert t is ctypes.c_void_p or t == ctypes.POINTER(ctypes.c_int64), (name, p)
            else:
                assert t is kinds[p.split()[0]], (name, p)


@pytest.mark.parametrize("r", (1, 7, 20, 32))
def test_send_regions(lib, r):
    for N in (1, 777, 1 << 20):
        total = lib.psgd_uvd_bf16_workspace_bytes(N, r)
        spans = []
        for stage in STAGES:
            off, cnt = _lib.uvd_bf16_ws_region(_lib.PSGD_WS_SEND_F64, stage, N, r)
            assert off % 8 == 0 and cnt > 0 and off >= 0 and off + 8 * cnt <= total, (stage, off, cnt)
            spans.append((off, off + 8 * cnt, stage))
        spans.sort()
        for (_, hi, a), (lo, _, b) in zip(spans, spans[1:]):
            assert hi <= lo, (a, b)
        counts = {s: _lib.uvd_bf16_ws_region(_lib.PSGD_WS_SEND_F64, s, N, r)[1] for s in STAGES}
        assert counts[1] == r and counts[2] == r and counts[10] == 2 and counts[12] == 1
        nb = (2 * r + 6 + 15) // 16
        assert counts[11] == 16 * nb * 80 and counts[11] <= 80 * 80           # the folded Gram, never the block partials


def test_ws_region_argument_checks(lib):
    BAD, RANK = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_RANK
    off, cnt = ctypes.c_int64(0), ctypes.c_int64(0)
    reg = lib.psgd_uvd_bf16_ws_region
    o, c = ctypes.byref(off), ctypes.byref(cnt)
    assert reg(_lib.PSGD_WS_SEND_F64, 11, 1000, 10, o, c) == 0
    assert reg(_lib.PSGD_WS_SEND_F64, 13, 1000, 10, o, c) == BAD              # no algebraic short cut: there is no stage 13
    assert reg(_lib.PSGD_WS_SEND_F64, 3, 1000, 10, o, c) == BAD
    assert reg(_lib.PSGD_WS_SUMS_F64, 11, 1000, 10, o, c) == BAD              # all-gather + fold is the only protocol
    assert reg(_lib.PSGD_WS_MAX_F32, 12, 1000, 10, o, c) == BAD
    assert reg(_lib.PSGD_WS_SEND_F64, 11, 0, 10, o, c) == BAD
    assert reg(_lib.PSGD_WS_SEND_F64, 11, 1000, 33, o, c) == RANK
    assert reg(_lib.PSGD_WS_SEND_F64, 11, 1000, 10, None, c) == BAD


def test_argument_checks(lib):
    BAD, RANK, WS, ALIGN = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_RANK, _lib.PSGD_ERR_WORKSPACE, _lib.PSGD_ERR_ALIGN
    U, V, d, v, h, g, out, ws, gat = (0x10000 * k for k in range(1, 10))      # never dereferenced: the checks fail first
    N, r = 1000, 10
    need = lib.psgd_uvd_bf16_workspace_bytes(N, r)
    tail = (ws, need, None)
    calls = {
        "fold": lambda **k: lib.psgd_uvd_bf16_fold_gathered_f64(k.get("stage", 11), k.get("gat", gat), k.get("world", 2), k.get("N", N),
                                                               k.get("r", r), *k.get("tail", tail)),
        "bmax": lambda **k: lib.psgd_uvd_balance_max_bf16(k.get("U", U), V, k.get("N", N), k.get("r", r), *k.get("tail", tail)),
        "gram": lambda **k: lib.psgd_uvd_update_gram_bf16(k.get("U", U), V, d, v, h, k.get("N", N), k.get("r", r), *k.get("tail", tail)),
        "rewrite": lambda **k: lib.psgd_uvd_update_rewrite_bf16(k.get("U", U), V, d, v, h, k.get("N", N), k.get("r", r), 0.01, 1e-38, 0, 1,
                                                                k.get("rounding", 1), 5, k.get("row0", 448), *k.get("tail", tail)),
        "upd_d": lambda **k: lib.psgd_uvd_update_d_bf16(k.get("U", d), k.get("N", N), k.get("r", r), 0.01, 1e-38, k.get("rounding", 1), 5,
                                                        k.get("row0", 448), *k.get("tail", tail)),
        "s1": lambda **k: lib.psgd_uvd_apply_sweep1_bf16(k.get("U", V), d, g, k.get("N", N), k.get("r", r), *k.get("tail", tail)),
        "s1d": lambda **k: lib.psgd_uvd_apply_sweep1_d_bf16(k.get("U", V), d, g, k.get("N", N), k.get("r", r), 0.01, 1e-38,
                                                            k.get("rounding", 1), 5, k.get("row0", 448), *k.get("tail", tail)),
        "s2": lambda **k: lib.psgd_uvd_apply_sweep2_bf16(k.get("U", U), d, g, out, k.get("N", N), k.get("r", r), *k.get("tail", tail)),
        "s3": lambda **k: lib.psgd_uvd_apply_sweep3_bf16(k.get("U", V), d, out, k.get("N", N), k.get("r", r), *k.get("tail", tail)),
    }
    for name, f in calls.items():
        assert f(N=0) == BAD, name
        assert f(r=33) == RANK, name
        assert f(r=0) == BAD, name
        assert f(tail=(None, need, None)) == WS, name
        assert f(tail=(ws, need - 1, None)) == WS, name
        assert f(tail=(ws + 16, need, None)) == WS, name
        if name != "fold":
            assert f(U=None) == BAD, name
            assert f(U=0x10000 + 2) == ALIGN, name                            # the state's base must be 16-byte aligned
    for name in ("rewrite", "upd_d", "s1d"):                                  # the stages that narrow
        assert calls[name](rounding=2) == BAD, name
        assert calls[name](rounding=-1) == BAD, name
        assert calls[name](row0=-1) == BAD, name
    assert calls["fold"](gat=None) == BAD
    assert calls["fold"](world=0) == BAD
    assert calls["fold"](stage=13) == BAD
    assert calls["fold"](stage=0) == BAD
    assert lib.psgd_uvd_apply_sweep2_bf16(U, d, g, g, N, r, *tail) == BAD     # out must not alias g
