"""Kron(operands="bfloat16"), the part that needs no GPU: the rule that picks the operand layers, the constructor's checks, and the C
ABI of the three list kernels behind it (exports, ctypes table, header, argument checks that return before any HIP call)."""
import ctypes
import os
import re

import pytest
import torch

from psgd_tf_amd import _lib
from psgd_tf_amd import kron_optimizer as ko

NAMES = ("psgd_multi_narrow_bf16", "psgd_multi_sumsq_mixed", "psgd_multi_param_update_mixed")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")
DD, DS, SD, ND = ("dense", "dense"), ("dense", "scale"), ("scale", "dense"), ("norm", "dense")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def _param(*shape, **kw):
    return torch.zeros(*shape, requires_grad=True, **kw)


# --------------------------------------------------------------------------------------------------------------- the rule
def test_the_threshold_holds_on_both_sides():
    shapes = [(63, 200), (64, 200), (200, 63), (200, 64), (64, 64), (63, 63), (1000, 65)]
    assert ko.kron_operand_layers(shapes, [DD] * 7, "bfloat16", 64) == [1, 3, 4, 6]
    assert ko.kron_operand_layers(shapes, [DD] * 7, torch.bfloat16, 64) == [1, 3, 4, 6]
    assert ko.kron_operand_layers(shapes, [DD] * 7, "bfloat16", 65) == [6]
    assert ko.kron_operand_layers(shapes, [DD] * 7, "bfloat16", 63) == list(range(7))
    assert ko.kron_operand_layers(shapes, [DD] * 7, "bfloat16", 10 ** 9) == []


def test_sizes_that_are_no_multiple_of_8_qualify():
    assert ko.kron_operand_layers([(20, 36), (9, 1001)], ["dense", DD], "bfloat16", 9) == [0, 1]


def test_sparse_formats_and_vectors_are_never_chosen():
    shapes = [(128, 128)] * len(ko.KRON_PAIRS)
    assert ko.kron_operand_layers(shapes, list(ko.KRON_PAIRS), "bfloat16", 1) == [ko.KRON_PAIRS.index(DD)]
    layers = ko.kron_layers([(300,), (64, 64), (), (1,)], "dense", any_rank=True)
    assert [kind for kind, _, _ in layers] == ["vector", "matrix", "scalar", "scalar"]
    assert ko.kron_operand_layers([s for _, s, _ in layers], [f for _, _, f in layers], "bfloat16", 2) == [1]


def test_operands_none_gives_nothing_and_the_default_threshold_is_the_measured_one():
    """profiles/kron_class_operands.txt: 768 is the smallest short side at which the bf16 route wins on both shapes"""
    shapes, fmts = [(4096, 4096), (768, 3072), (767, 4096)], [DD] * 3
    assert ko.kron_operand_layers(shapes, fmts, None, 1) == []
    assert ko.kron_operand_layers(shapes, fmts) == []
    assert ko.OPERAND_MIN_DIM == 768
    assert ko.kron_operand_layers(shapes, fmts, "bfloat16") == [0, 1]


def test_any_rank_views_are_judged_by_their_layer_shape():
    """(16, 2, 2, 2) is the layer (16, 8): its short side is 8, not 2; (4, 30, 30) is (4, 900): short side 4"""
    true_shapes = [(16, 2, 2, 2), (4, 30, 30), (12, 3, 4)]
    layers = ko.kron_layers(true_shapes, "dense", any_rank=True)
    shapes, fmts = [s for _, s, _ in layers], [f for _, _, f in layers]
    assert shapes == [(16, 8), (4, 900), (12, 12)]
    assert ko.kron_operand_layers(shapes, fmts, "bfloat16", 8) == [0, 2]
    assert ko.kron_operand_layers(shapes, fmts, "bfloat16", 9) == [2]
    assert ko.kron_operand_layers(shapes, fmts, "bfloat16", 4) == [0, 1, 2]
    with pytest.raises(ValueError, match=r"a layer shape is \(M, N\)"):
        ko.kron_operand_layers(true_shapes, fmts, "bfloat16", 8)
    with pytest.raises(ValueError, match="3 layer shapes and 2 formats"):
        ko.kron_operand_layers(shapes, fmts[:2], "bfloat16", 8)


BAD_OPERANDS = ["float16", torch.float16, "bf16", torch.float32, "float32", 16, True, ""]
BAD_MIN_DIM = [0, -1, 7.5, "8", None, True, 1024.0]


@pytest.mark.parametrize("bad", BAD_OPERANDS, ids=repr)
def test_bad_operands_raise(bad):
    with pytest.raises(ValueError, match="operands must be None, 'bfloat16' or torch.bfloat16"):
        ko.kron_operand_layers([(8, 8)], [DD], bad, 8)
    with pytest.raises(ValueError, match="operands must be None, 'bfloat16' or torch.bfloat16"):
        ko.Kron([_param(8, 8)], operands=bad)                  # (a CPU parameter: the check comes before anything touches a device)


@pytest.mark.parametrize("bad", BAD_MIN_DIM, ids=repr)
def test_bad_operand_min_dim_raises(bad):
    with pytest.raises(ValueError, match="operand_min_dim must be an integer >= 1"):
        ko.kron_operand_layers([(8, 8)], [DD], "bfloat16", bad)
    with pytest.raises(ValueError, match="operand_min_dim must be an integer >= 1"):
        ko.Kron([_param(8, 8)], operands="bfloat16", operand_min_dim=bad)
    with pytest.raises(ValueError, match="operand_min_dim must be an integer >= 1"):
        ko.Kron([_param(8, 8)], operand_min_dim=bad)           # ... whatever operands


def test_good_values_reach_the_device_check_and_the_keywords_are_keyword_only():
    for kw in (dict(operands=None), dict(operands="bfloat16"), dict(operands=torch.bfloat16, operand_min_dim=8),
               dict(operand_min_dim=1)):
        with pytest.raises(ValueError, match="one HIP device"):
            ko.Kron([_param(8, 8)], **kw)
    import inspect
    sig = inspect.signature(ko.Kron.__init__).parameters
    assert sig["operands"].kind is sig["operand_min_dim"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["operands"].default is None and sig["operand_min_dim"].default == ko.OPERAND_MIN_DIM


def test_the_docstring_moved_the_item_out_of_scope():
    doc = ko.Kron.__doc__
    scope = doc[doc.index("Out of scope"):]
    assert "bf16-operand" not in scope and "operands=\"bfloat16\"" in doc and "6 bytes per" in doc


# ------------------------------------------------------------------------------------------------------------------- C ABI
def test_exports_are_bound_and_the_version_did_not_move(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.psgd_abi_version() == 7 == _lib.PSGD_ABI_VERSION


def test_signatures_match_the_header():
    text = open(HEADER).read()
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "int32_t": ctypes.c_int32}
    for name in NAMES:
        m = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
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
    assert re.search(r"psgd_multi_narrow_bf16, psgd_multi_sumsq_mixed and psgd_multi_param_update_mixed.*still 7", text, re.S)


def test_argument_checks(lib):
    """null tables, negative counts, a source without its destination, a missing workspace, an unknown dtype code: an error code
    with no device present; nchunks == 0 launches nothing.  The dtype code the host can see is the parameters' (dtype of
    psgd_multi_param_update_mixed); the per-segment codes of a mixed list live in the device table (the `start` fields), where a
    segment with an unknown code is skipped by the kernel -- the GPU tests cover that."""
    BAD, OK, WS = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_OK, _lib.PSGD_ERR_WORKSPACE
    s0, s1, s2, d0, d1, d2, chunks, out, ws = (0x10000 * k for k in range(1, 10))        # never dereferenced: the checks fail first
    narrow, sumsq, upd = lib.psgd_multi_narrow_bf16, lib.psgd_multi_sumsq_mixed, lib.psgd_multi_param_update_mixed
    assert narrow(None, s1, s2, d0, d1, d2, 3, chunks, 5, None) == BAD
    assert narrow(s0, s1, s2, None, d1, d2, 3, chunks, 5, None) == BAD
    assert narrow(s0, s1, s2, d0, None, d2, 3, chunks, 5, None) == BAD                   # a source without a destination
    assert narrow(s0, None, s2, d0, d1, d2, 3, chunks, 5, None) == BAD                   # ... and the reverse
    assert narrow(s0, s1, None, d0, d1, d2, 3, chunks, 5, None) == BAD
    assert narrow(s0, s1, s2, d0, d1, d2, 3, None, 5, None) == BAD
    assert narrow(s0, s1, s2, d0, d1, d2, -1, chunks, 5, None) == BAD
    assert narrow(s0, s1, s2, d0, d1, d2, 3, chunks, -5, None) == BAD
    assert narrow(s0, s1, s2, d0, d1, d2, 3, chunks, 0, None) == OK
    assert narrow(s0, None, None, d0, None, None, 3, chunks, 0, None) == OK
    assert narrow(s0, s1, None, d0, d1, None, 0, chunks, 0, None) == OK
    nb = _lib.MULTI_SUMSQ_WS_BYTES
    assert sumsq(None, 3, chunks, 5, out, ws, nb, None) == BAD
    assert sumsq(s0, 3, None, 5, out, ws, nb, None) == BAD
    assert sumsq(s0, 3, chunks, 5, None, ws, nb, None) == BAD
    assert sumsq(s0, 3, chunks, 5, out + 4, ws, nb, None) == BAD                         # a misaligned double
    assert sumsq(s0, 3, chunks, 5, out, None, nb, None) == BAD
    assert sumsq(s0, -3, chunks, 5, out, ws, nb, None) == BAD
    assert sumsq(s0, 3, chunks, -5, out, ws, nb, None) == BAD
    assert sumsq(s0, 3, chunks, 5, out, ws, nb - 1, None) == WS
    assert sumsq(s0, 3, chunks, 5, out, ws + 4, nb, None) == WS
    assert sumsq(s0, 3, chunks, 0, out, ws, nb, None) == OK
    tail = (0.1, None, 0.0, 1e-38)
    for dt in (-1, 3, 99):                                                               # an unknown dtype code
        assert upd(s0, s1, None, 3, chunks, 0, dt, *tail, 0.0, None) == BAD
        assert upd(s0, s1, s2, 3, chunks, 5, dt, *tail, 0.01, None) == BAD
    for dt in (_lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16):
        assert upd(None, s1, None, 3, chunks, 5, dt, *tail, 0.01, None) == BAD
        assert upd(s0, None, s2, 3, chunks, 5, dt, *tail, 0.0, None) == BAD              # p + v keeps its entry points
        assert upd(s0, None, None, 3, chunks, 0, dt, *tail, 0.0, None) == BAD            # ... whatever nchunks
        assert upd(s0, s1, None, 3, None, 5, dt, *tail, 0.01, None) == BAD
        assert upd(s0, s1, None, -3, chunks, 5, dt, *tail, 0.01, None) == BAD
        assert upd(s0, s1, None, 3, chunks, -1, dt, *tail, 0.01, None) == BAD
        assert upd(s0, s1, s2, 3, chunks, 0, dt, *tail, 0.01, None) == OK
        assert upd(s0, s1, None, 3, chunks, 0, dt, 0.1, out, 1.0, 1e-38, 0.0, None) == OK


def test_the_wrappers_are_exported_like_their_siblings():
    import preconditioned_stochastic_gradient_descent as shim
    from psgd_tf_amd import psgd
    assert shim.multi_narrow is psgd.multi_narrow is ko.multi_narrow
    assert shim.kron_operand_layers is psgd.kron_operand_layers is ko.kron_operand_layers
    assert shim.multi_sumsq is ko.multi_sumsq and shim.multi_param_update is ko.multi_param_update


def test_wrappers_refuse_what_the_kernels_cannot_take():
    t = torch.zeros(3, 4)
    h = t.bfloat16()
    with pytest.raises(ValueError, match="one to three source lists"):
        ko.multi_narrow([], [])
    with pytest.raises(ValueError, match="one to three source lists"):
        ko.multi_narrow([[t]], [[h], [h]])
    with pytest.raises(ValueError, match="a list is None"):
        ko.multi_narrow([[t]], [None])
    with pytest.raises(TypeError, match=r"srcs\[0\]\[0\] must be float32, got torch.bfloat16"):
        ko.multi_narrow([[h]], [[h]])
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        ko.multi_narrow([[t]], [[h]])
    with pytest.raises(TypeError, match=r"tensors\[0\] must be float32, got torch.bfloat16"):
        ko.multi_sumsq([h])                                    # a bfloat16 tensor off the device is no mixed list
