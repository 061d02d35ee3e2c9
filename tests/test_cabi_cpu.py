"""The C-ABI library: builds for gfx950 without a GPU, loads, and exports exactly the symbols
that include/psgd_hip.h declares (and _lib.py binds).  No compute calls here -- only entry points
whose argument checks return before any HIP call."""
import ctypes
import os
import re

import pytest

from psgd_tf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "psgd_hip.h")


def _declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(psgd_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def test_header_symbols_are_exported_and_bound(lib):
    declared = _declared_symbols()
    assert len(declared) >= 20
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), "declared in psgd_hip.h but not exported: " + name
        assert name in _lib.SIGNATURES, "declared in psgd_hip.h but not bound in _lib.py: " + name
    assert sorted(_lib.SIGNATURES) == declared


def test_abi_version_and_error_strings(lib):
    assert lib.psgd_abi_version() == _lib.PSGD_ABI_VERSION == 7
    assert lib.psgd_error_string(0) == b"ok"
    for code in (-1, -2, -3, -4, -5, -6):
        assert len(lib.psgd_error_string(code)) > 3


def test_workspace_queries_and_argument_checks(lib):
    # psgd.py:690 keeps an N-vector temporary per call (nablaD, :581): workspace grows by 4 N bytes
    a = lib.psgd_uvd_workspace_bytes(1_000_000, 10)
    b = lib.psgd_uvd_workspace_bytes(2_000_000, 10)
    assert a > 0 and b - a == 4_000_000 and a % 256 == 0
    assert lib.psgd_uvd_workspace_bytes(100, 0) == -2 and lib.psgd_uvd_workspace_bytes(100, 33) == -2   # PSGD_ERR_RANK
    assert lib.psgd_uvd_workspace_bytes(0, 4) == -1                                                       # PSGD_ERR_BAD_ARG
    off, cnt = _lib.ws_region(_lib.PSGD_WS_SUMS_F64, 1, 1000, 20)
    off2, cnt2 = _lib.ws_region(_lib.PSGD_WS_SUMS_F64, 2, 1000, 20)
    assert cnt == cnt2 == 20 and off2 - off == 160
    _, gram = _lib.ws_region(_lib.PSGD_WS_SUMS_F64, 11, 1000, 20)
    assert gram == 6 * 256                      # [U V t w] = 42 columns -> 3 MFMA blocks -> 6 block pairs
    _, gram10 = _lib.ws_region(_lib.PSGD_WS_SUMS_F64, 11, 1000, 10)
    assert gram10 == 3 * 256
    _, m = _lib.ws_region(_lib.PSGD_WS_MAX_F32, 10, 1000, 20)
    assert m == 2
    # null pointers are rejected before anything touches the device
    assert lib.psgd_uvd_apply_f32(None, None, None, None, None, 100, 4, None, 0, None) == -1
    assert lib.psgd_uvd_update_f32(None, None, None, None, None, 100, 4, 0.01, 1e-38, 0, 1, None, 0, None) == -1
    assert lib.psgd_kron_dd_apply_f32(None, None, None, None, 4, 4, None, 0, None) == -1
    assert lib.psgd_kron_dd_workspace_bytes(0, 4) == -1
    assert lib.psgd_kron_dd_workspace_bytes(257, 120) > 4 * (2 * 257 * 257 + 2 * 120 * 120 + 4 * 257 * 120)


def test_kron_workspace_layout_rules(lib):
    """Workspace sizes are pure functions of the shape (a workspace sized once stays valid whatever the tuning keys): the plane
    buffers appear from the planes threshold on, the buffers of the solves through explicit inverses from 2048 x 2048 on --
    in the fp32 workspace and in the bf16-operand update's alike -- and tuning keys do not move the sizes."""
    ws = lib.psgd_kron_dd_workspace_bytes
    fp32_only = lambda m, n: 4 * (4 * m * m + 2 * n * n + 4 * m * n)          # a lower bound of the fp32 buffers
    assert ws(300, 300) < 3 * fp32_only(300, 300)                             # no planes at 300^2
    assert ws(1024, 1024) > fp32_only(1024, 1024) + 16 * 1024 * 1024 * 6      # planes of the large paths (6 B per element)
    per = lambda n: ws(n, n) / float(n * n)
    assert per(2048) > per(1920) + 4 * 4                                     # inverse route: more bytes per element from 2048^2 on
    upd = lib.psgd_kron_dd_update_workspace_bytes_bf16
    assert upd(2048, 2048) / float(2048 * 2048) > upd(1920, 1920) / float(1920 * 1920) + 4 * 4
    before = (ws(2048, 2048), upd(2048, 2048), ws(1024, 1024))
    try:
        for key, val in ((11, 0), (12, 0), (4, 0)):
            assert lib.psgd_kron_set_tuning(key, val) == 0
        assert (ws(2048, 2048), upd(2048, 2048), ws(1024, 1024)) == before
    finally:
        for key, val in ((11, 1), (12, 2), (4, 1)):
            lib.psgd_kron_set_tuning(key, val)
    assert lib.psgd_kron_set_tuning(999, 0) == -1                             # unknown key: PSGD_ERR_BAD_ARG
    sp = lib.psgd_kron_sparse_workspace_bytes
    assert sp(1, 30000, 1000) > sp(1, 30000, 500) and sp(2, 30000, 1000) < sp(1, 30000, 1000)      # (norm, dense) vs (norm, scaling)


def test_kron_route_flags_anchor_the_route_table(lib):
    """psgd_kron_dd_route_flags reports the predicates the Kron launch code branches on (no GPU needed): a few anchors of the
    route table, and a tuning key that moves the route moves the flag."""
    R = lambda m, n: lib.psgd_kron_dd_route_flags(m, n)
    inv = _lib.KRON_ROUTE_INV_SOLVES
    assert R(0, 4) == R(4, -1) == _lib.PSGD_ERR_SHAPE
    assert R(1024, 4096) & inv and R(4096, 1024) & inv
    assert not R(1023, 2048) & inv and not R(256, 8193) & inv
    assert R(6144, 6144) & inv and not R(6144, 6144) & _lib.KRON_ROUTE_INV_FIRST
    assert R(4096, 4096) & _lib.KRON_ROUTE_BG_FRONT
    assert R(512, 512) & _lib.KRON_ROUTE_SMALL and not R(513, 512) & _lib.KRON_ROUTE_SMALL
    chunks = lambda f: (f & _lib.KRON_ROUTE_RECT_CHUNKS_MASK) >> _lib.KRON_ROUTE_RECT_CHUNKS_SHIFT
    assert R(1024, 1536) & _lib.KRON_ROUTE_GRAD_RECT and chunks(R(1024, 1536)) == 2
    assert not R(1024, 1535) & _lib.KRON_ROUTE_GRAD_RECT and chunks(R(1024, 1535)) == 0
    try:
        assert lib.psgd_kron_set_tuning(11, 0) == 0
        assert not R(1024, 4096) & inv and R(1024, 4096) & _lib.KRON_ROUTE_PLANES_UPDATE
    finally:
        lib.psgd_kron_set_tuning(11, 1)
    assert R(1024, 4096) & inv


# Exported symbols that compute nothing on caller memory: version / error text, size and layout queries, host-only route and key
# functions, tuning setters, the profiling hooks, and the read-back of the bf16 hand-off counter.  Everything else is a compute
# entry point and must have an extent test.
NOT_COMPUTE = {
    "psgd_abi_version", "psgd_error_string", "psgd_set_tuning", "psgd_kron_set_tuning", "psgd_kron_bf16_set_tuning",
    "psgd_prof_enable", "psgd_prof_collect",
    "psgd_uvd_workspace_bytes", "psgd_uvd_ws_region", "psgd_uvd_gram_wide_scratch_bytes", "psgd_uvd_wide_scratch_bytes",
    "psgd_uvd_wide_update_scratch_bytes", "psgd_uvd_wide_update_apply_scratch_bytes", "psgd_uvd_bf16_workspace_bytes",
    "psgd_uvd_bf16_ws_region", "psgd_uvd_bf16_rounding_key", "psgd_splu_workspace_bytes", "psgd_splu_ws_region",
    "psgd_splu_bf16_workspace_bytes", "psgd_kron_dd_workspace_bytes", "psgd_kron_dd_workspace_bytes_batched",
    "psgd_kron_sparse_workspace_bytes", "psgd_kron_dd_workspace_bytes_bf16", "psgd_kron_dd_update_workspace_bytes_bf16",
    "psgd_kron_dd_apply_direct_distinct", "psgd_kron_dd_route_flags", "psgd_kron_bf16_handoff_counter_offset",
    "psgd_kron_bf16_handoff_timeouts", "psgd_dense_workspace_bytes",
}


def test_every_compute_entry_point_has_an_extent_test():
    """A kernel cannot arrive without a guard-band test: every exported symbol is exempt by name (NOT_COMPUTE), in the case table of
    tests/test_extents_gpu.py (and really called there), or in its covered-elsewhere list (the list kernels) with a GPU test file that runs it by name."""
    from tests import test_extents_gpu as ext
    declared = set(_declared_symbols())
    table = {n for names in ext.ENTRY_POINTS.values() for n in names}
    elsewhere = set(ext.COVERED_ELSEWHERE)
    assert NOT_COMPUTE <= declared and table <= declared and elsewhere <= declared, "a list names a symbol the header does not declare"
    assert not (table & elsewhere) and not (NOT_COMPUTE & (table | elsewhere))
    # covered elsewhere = the list kernels, by name pattern, all of them and nothing else: no other entry point can hide there
    is_list = lambda n: n.startswith(ext.COVERED_ELSEWHERE_PATTERNS)
    assert elsewhere == {n for n in declared if is_list(n)}, sorted(elsewhere ^ {n for n in declared if is_list(n)})
    missing = declared - NOT_COMPUTE - table - elsewhere
    assert not missing, "compute entry points without an extent test: %s" % sorted(missing)
    src = open(ext.__file__).read()
    for name in sorted(table):
        fmt = name.replace("_ds_", "_%s_").replace("_nd_", "_%s_").replace("_ns_", "_%s_")
        called = any(form % n in src for form in ('call("%s"', 'exchange("%s"') for n in (name, fmt))
        assert called, name + " is in the case table but no case calls it"
    for name, path in ext.COVERED_ELSEWHERE.items():
        text = open(os.path.join(ROOT, path)).read()
        assert os.path.basename(path).endswith("_gpu.py") and (name in text or name[len("psgd_"):] in text), (name, path)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback|missing"):
        _lib.load()
