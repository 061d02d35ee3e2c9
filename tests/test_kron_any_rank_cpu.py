"""Kron(any_rank=True) and the vector-layer kernels, the part that needs no GPU: the layout of parameters of any rank as layers, the
constructor's refusals, the host part of the checkpoint, the C ABI of the two new entry points (header = exports = ctypes table,
argument checks that return before any HIP call), and the specification of the kernels pinned to the fp64 oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from psgd_tf_amd import _lib
from psgd_tf_amd import kron_optimizer as ko
from tests import multi_vec_cases as mv

NAMES = ("psgd_multi_vec_update_f32", "psgd_multi_vec_apply_f32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")
# the module of the class tests: a conv kernel and its bias, a linear layer and its bias, the two vectors of a LayerNorm
MODULE_SHAPES = [(4, 3, 3, 3), (4,), (12, 7), (12,), (7,), (7,)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def _param(*shape, **kw):
    return torch.zeros(shape, requires_grad=True, **kw)


# ----------------------------------------------------------------------------------------------------------------- layout
def test_exported_from_the_package_module_and_the_shim():
    import preconditioned_stochastic_gradient_descent as shim
    from psgd_tf_amd import psgd
    assert shim.multi_vec_precond_update is psgd.multi_vec_precond_update is ko.multi_vec_precond_update
    assert shim.multi_vec_precond_grad is psgd.multi_vec_precond_grad is ko.multi_vec_precond_grad
    assert shim.kron_layers is ko.kron_layers


def test_any_rank_accepts_ranks_0_1_3_4_and_lays_them_out():
    shapes = [(), (1,), (5,), (2, 3, 4), (4, 3, 3, 3), (6, 5)]
    layers = ko.kron_layers(shapes, ("norm", "dense"), any_rank=True)
    assert layers == [("scalar", (1, 1), ("dense", "dense")), ("scalar", (1, 1), ("dense", "dense")),
                      ("vector", (1, 5), ("dense", "scale")), ("matrix", (2, 12), ("norm", "dense")),
                      ("matrix", (4, 27), ("norm", "dense")), ("matrix", (6, 5), ("norm", "dense"))]
    # the constructor gets past the rank check with these parameters: what stops it on this machine is the device
    for shape in shapes[:5]:
        with pytest.raises(ValueError, match="one HIP device"):
            ko.Kron([_param(*shape)], any_rank=True)
    # ... and with the switch off, or left out, ranks other than 2 are refused with the messages they always had
    for kw in ({}, {"any_rank": False}):
        with pytest.raises(ValueError, match=r"parameter 0 \(shape \(5,\).*rank 2"):
            ko.Kron([_param(5)], **kw)
        with pytest.raises(ValueError, match=r"parameter 1 .*rank 2"):
            ko.Kron([_param(3, 4), _param(2, 3, 4)], **kw)
    with pytest.raises(ValueError, match="vector_route"):
        ko.Kron([_param(5)], any_rank=True, vector_route="batched")


def test_factor_shapes_of_the_layers():
    scale = 0.25
    for kind, shape, pair in ko.kron_layers(MODULE_SHAPES + [(), (1,)], "dense", any_rank=True):
        Ql, Qr = ko.kron_initial_factors(shape, pair, scale)
        assert Ql.dtype == Qr.dtype == torch.float32
        if kind == "vector":
            n = shape[1]
            assert pair == ko.VECTOR_FORMAT and tuple(Ql.shape) == (1, 1) and tuple(Qr.shape) == (1, n)
            assert float(Ql) == scale and torch.equal(Qr, torch.ones(1, n))          # Ql = preconditioner_init_scale, Qr = ones
        elif kind == "scalar":
            assert tuple(Ql.shape) == tuple(Qr.shape) == (1, 1) and float(Ql) == scale and float(Qr) == 1.0
        else:
            assert tuple(Ql.shape) == (shape[0], shape[0]) and tuple(Qr.shape) == (shape[1], shape[1])
    kinds = [k for k, _, _ in ko.kron_layers(MODULE_SHAPES, "dense", any_rank=True)]
    assert kinds == ["matrix", "vector", "matrix", "vector", "vector", "vector"]
    assert ko.kron_layers(MODULE_SHAPES, "dense", any_rank=True)[0][1] == (4, 27)   # the conv kernel, folded
    with pytest.raises(ValueError, match="square like a dense one"):               # a scaling side of length 1 stays refused
        ko.kron_initial_factors((1, 1), ko.VECTOR_FORMAT)


def test_per_parameter_formats_of_vectors_and_scalars():
    shapes = [(6, 5), (5,), ()]
    ok = ko.kron_layers(shapes, [("scale", "dense"), ("dense", "scale"), "dense"], any_rank=True)
    assert [f for _, _, f in ok] == [("scale", "dense"), ("dense", "scale"), ("dense", "dense")]
    assert ko.kron_layers(shapes, ["dense", "dense", ("dense", "dense")], any_rank=True)[1][2] == ("dense", "scale")
    for bad in (("dense", "dense"), ("dense", "norm"), ("scale", "dense"), "scale", 3):
        with pytest.raises(ValueError, match=r"parameter 1 \(shape \(5,\)\) is a vector layer.*\('dense', 'scale'\)"):
            ko.kron_layers(shapes, ["dense", bad, "dense"], any_rank=True)
        with pytest.raises(ValueError, match=r"parameter 1 \(shape \(5,\)\) is a vector layer"):
            ko.Kron([_param(*s) for s in shapes], ["dense", bad, "dense"], any_rank=True)        # refused before any device is asked
    with pytest.raises(ValueError, match=r"parameter 2 \(shape \(\)\) is a scalar layer"):
        ko.kron_layers(shapes, ["dense", "dense", ("dense", "scale")], any_rank=True)
    with pytest.raises(ValueError, match="2 formats for 3 parameters"):
        ko.kron_layers(shapes, [("dense", "dense"), "dense"], any_rank=True)
    # one format for all parameters applies to the matrix layers only
    assert [f for _, _, f in ko.kron_layers(shapes, ("dense", "norm"), any_rank=True)] == \
        [("dense", "norm"), ("dense", "scale"), ("dense", "dense")]


def test_all_rank_2_layout_does_not_depend_on_the_switch():
    shapes, formats = [(5, 7), (4, 3)], [("dense", "norm"), ("scale", "dense")]
    for f in (formats, "dense", ("norm", "scale")):
        assert ko.kron_layers(shapes, f, any_rank=True) == ko.kron_layers(shapes, f, any_rank=False)
        assert [x for _, _, x in ko.kron_layers(shapes, f, any_rank=True)] == ko.kron_formats(f, 2)
    with pytest.raises(ValueError, match="does not exist"):
        ko.kron_layers(shapes, ("norm", "norm"), any_rank=True)


# ----------------------------------------------------------------------------------------------------------------- checkpoint
def _state(shapes, formats, any_rank, seed=5):
    layers = ko.kron_layers(shapes, formats, any_rank)
    g = torch.Generator().manual_seed(seed)
    factors = [[torch.randn(q.shape, generator=g) for q in ko.kron_initial_factors(s, f)] for _, s, f in layers]
    hyper = dict(lr_params=0.02, lr_preconditioner=0.05, grad_clip_max_norm=float("inf"), preconditioner_update_probability=0.5,
                 exact_hessian_vector_product=False)
    return layers, ko._encode_state(factors, [f for _, _, f in layers], shapes, hyper, g.get_state())


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return type(a) is type(b) and a == b


def test_all_rank_2_state_dict_is_unchanged_by_the_switch():
    import io
    shapes, formats = [(5, 7), (4, 3)], [("dense", "norm"), ("scale", "dense")]
    blobs = []
    for any_rank in (False, True):
        _, sd = _state(shapes, formats, any_rank)
        buf = io.BytesIO()
        torch.save(sd, buf)
        blobs.append((sd, buf.getvalue()))
    assert _same(blobs[0][0], blobs[1][0])
    assert blobs[0][1] == blobs[1][1]                                             # byte for byte
    assert blobs[0][0]["param_shapes"] == [[5, 7], [4, 3]]


def test_state_dict_with_vectors_holds_true_shapes_and_layer_factors():
    layers, sd = _state(MODULE_SHAPES, "dense", True)
    assert sd["param_shapes"] == [list(s) for s in MODULE_SHAPES]                 # the parameters' true shapes
    assert sd["preconditioner_formats"] == [["dense", "dense"], ["dense", "scale"], ["dense", "dense"], ["dense", "scale"],
                                            ["dense", "scale"], ["dense", "scale"]]
    assert [tuple(q.shape) for q in sd["factors"][1]] == [(1, 1), (1, 4)] and sd["factors"][1][0].dtype == torch.float32
    assert [tuple(q.shape) for q in sd["factors"][0]] == [(4, 4), (27, 27)]
    formats, shapes2d = [f for _, _, f in layers], [s for _, s, _ in layers]
    factors, _, _ = ko._decode_state(sd, formats, MODULE_SHAPES, shapes2d)
    assert all(torch.equal(a, b) for pa, pb in zip(factors, sd["factors"]) for a, b in zip(pa, pb))
    # an optimizer of other shapes refuses it with the messages there always were
    other = [(4, 3, 3, 3), (4,), (12, 7), (12,), (7,), (8,)]
    lo = ko.kron_layers(other, "dense", True)
    with pytest.raises(ValueError, match="param_shapes"):
        ko._decode_state(sd, [f for _, _, f in lo], other, [s for _, s, _ in lo])
    folded = [(4, 27), (4,), (12, 7), (12,), (7,), (7,)]                         # the same layers, another parameter shape
    with pytest.raises(ValueError, match="param_shapes"):
        ko._decode_state(sd, formats, folded, shapes2d)
    as_matrices = [(4, 27), (1, 4), (12, 7), (1, 12), (1, 7), (1, 7)]            # an all-rank-2 optimizer of the same layers
    with pytest.raises(ValueError, match="param_shapes"):
        ko._decode_state(sd, formats, as_matrices)
    with pytest.raises(ValueError, match=r"'factors'\[1\]"):
        ko._decode_state(dict(sd, factors=[sd["factors"][0], sd["factors"][4]] + sd["factors"][2:]), formats, MODULE_SHAPES, shapes2d)


# ----------------------------------------------------------------------------------------------------------------- C ABI
def test_exports_are_bound(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.psgd_abi_version() == 7                      # additive: the version did not move


def test_signatures_match_the_header():
    text = open(HEADER).read()
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
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


def test_argument_checks(lib):
    """a null table, k < 1, a vector shorter than 2: an error code with no device present"""
    BAD = _lib.PSGD_ERR_BAD_ARG
    a, b, c, d = (0x10000 * k for k in range(1, 5))                     # never dereferenced: the checks fail first
    upd, app = lib.psgd_multi_vec_update_f32, lib.psgd_multi_vec_apply_f32
    for i in range(4):
        tabs = [a, b, c, d]
        tabs[i] = None
        assert upd(*tabs, 3, 5, 0.01, 1e-38, None) == BAD
        assert app(*tabs, 3, 5, None) == BAD
    for k in (0, -1):
        assert upd(a, b, c, d, k, 5, 0.01, 1e-38, None) == BAD
        assert app(a, b, c, d, k, 5, None) == BAD
    for n in (1, 0, -7):
        assert upd(a, b, c, d, 3, n, 0.01, 1e-38, None) == BAD
        assert app(a, b, c, d, 3, n, None) == BAD


def test_wrappers_refuse_what_the_kernels_cannot_take():
    """checked before a plan is made or the library is called: a CPU machine sees the same errors"""
    q, v = torch.ones(1, 1), torch.ones(1, 5)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        ko.multi_vec_precond_update([q], [v], [v], [v], 0.01)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        ko.multi_vec_precond_grad([q], [v], [v], [v])
    with pytest.raises(ValueError, match="empty tensor list"):
        ko.multi_vec_precond_update([], [], [], [], 0.01)
    with pytest.raises(TypeError, match=r"qrs\[0\] must be float32"):
        ko.multi_vec_precond_update([q], [v.double()], [v], [v], 0.01)
    with pytest.raises(TypeError, match=r"qrs\[0\] is not a torch tensor"):
        ko.multi_vec_precond_grad([q], [3.0], [v], [v])


# ----------------------------------------------------------------------------------------------------------------- specification
@pytest.mark.parametrize("state", mv.STATES)
def test_fp64_oracle_reproduces_the_three_phase_formulas(state):
    """the kernel's specification (mv.three_phase, mv.apply_formula) is what oracle.update_precond_kron / precond_grad_kron compute
    on the [1, n] layer, to 1e-13 in fp64: the GPU tests compare the kernels with the oracle, this pins the formulas to it"""
    worst = 0.0
    for n in mv.LENGTHS[:-1]:
        ql, qr, dx, dg, g = (np.asarray(a, dtype=np.float64) for a in mv.case(n, state))
        ref_ql, ref_qr = mv.oracle_update(ql, qr, dx, dg, mv.STEP)
        got_ql, got_qr = mv.three_phase(ql, qr, dx, dg, mv.STEP, np.finfo(np.float64).tiny)
        e = max(mv.rel(got_ql, ref_ql), mv.rel(got_qr, ref_qr), mv.rel(got_qr - qr, ref_qr - qr), abs((got_ql - ql) / (ref_ql - ql) - 1),
                mv.rel(mv.apply_formula(ql, qr, g), mv.oracle_apply(ql, qr, g)))
        worst = max(worst, e)
        assert e < 1e-13, (n, state, e)
    print("%s: three-phase formulas against the fp64 oracle, worst relative error %.2e" % (state, worst))


@pytest.mark.parametrize("state", mv.STATES)
def test_fp32_oracle_stays_inside_the_bars(state):
    """the bars of the GPU tests (factors 1e-5, increments 2e-3, apply 1e-5) are not asked of inputs on which fp32 arithmetic in
    the reference's order cannot meet them: the oracle run in float32 on every test input stays inside them, with room"""
    worst = [0.0, 0.0, 0.0]
    for n in mv.LENGTHS:
        ql, qr, dx, dg, g = mv.case(n, state)
        new_ql, new_qr = mv.oracle_update(ql, qr, dx, dg, np.float32(mv.STEP), dtype=np.float32)
        assert new_qr.dtype == np.float32
        e_fac, e_inc = mv.update_errors(new_ql, new_qr, ql, qr, dx, dg)
        e_app = mv.rel(mv.oracle_apply(ql, qr, g, dtype=np.float32), mv.oracle_apply(ql, qr, g))
        worst = [max(a, b) for a, b in zip(worst, (e_fac, e_inc, e_app))]
        assert e_fac < mv.BAR_FACTORS / 4 and e_inc < mv.BAR_INCREMENT / 4 and e_app < mv.BAR_APPLY / 4, (n, state, e_fac, e_inc, e_app)
    print("%s: fp32 oracle against fp64, worst factors %.2e, increments %.2e, apply %.2e" % ((state,) + tuple(worst)))
