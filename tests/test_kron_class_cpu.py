"""class Kron and the list kernels of its step tail, the part that needs no GPU: constructor and wrapper argument errors, the format
table, initial factors, the host part of the checkpoint, the C ABI of psgd_multi_tail.hip (header = exports = ctypes table, argument
checks that return before any HIP call) and the fp64 restatement of the step that the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from psgd_tf_amd import _lib
from psgd_tf_amd import kron_optimizer as ko
from tests import kron_class_cases as kc

NAMES = ("psgd_multi_sumsq_f32", "psgd_multi_param_update_f32", "psgd_multi_diff_scale_f32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def _param(*shape, **kw):
    return torch.zeros(*shape, requires_grad=True, **kw)


# ----------------------------------------------------------------------------------------------------------------- constructor
def test_exported_from_the_package_module_and_the_shim():
    import preconditioned_stochastic_gradient_descent as shim
    from psgd_tf_amd import psgd
    assert shim.Kron is psgd.Kron is ko.Kron
    assert shim.multi_sumsq is ko.multi_sumsq and shim.multi_param_update is ko.multi_param_update
    assert shim.multi_diff_scale is ko.multi_diff_scale


def test_the_step_layer_is_the_one_copy_under_the_flat_classes():
    """what class Kron shares with class UVd, class SPLU and class Dense in step() and __init__ lives on _StepFeatures alone"""
    from psgd_tf_amd import psgd
    base = psgd._StepFeatures
    assert issubclass(ko.Kron, base) and not issubclass(ko.Kron, psgd._FlatStep)
    for f in ("_HYPER_KEYS", "_init_step_hypers", "_step_route", "_closure_gradients", "_tail_coefficients", "_fused_tail_kwargs"):
        assert getattr(ko.Kron, f) is getattr(base, f), f
        assert f not in vars(ko.Kron), f
    assert ko.Kron._HYPER_KEYS is psgd.UVd._HYPER_KEYS is ko._HYPER_KEYS


@pytest.mark.parametrize("make, exc, match", [
    (lambda: ko.Kron([_param(3, 4), np.zeros((3, 4))]), TypeError, "parameter 1 is not a torch tensor"),
    (lambda: ko.Kron([_param(3, 4), _param(3, 4, dtype=torch.bfloat16)]), TypeError, r"parameter 1 \(shape \(3, 4\).*float32"),
    (lambda: ko.Kron([_param(3, 4, dtype=torch.float64)]), TypeError, "parameter 0"),
    (lambda: ko.Kron([_param(5)]), ValueError, r"parameter 0 \(shape \(5,\).*rank 2"),
    (lambda: ko.Kron([_param(3, 4), _param(2, 3, 4)]), ValueError, r"parameter 1 .*rank 2"),
    (lambda: ko.Kron([torch.zeros(3, 4)]), ValueError, "parameter 0.*require grad"),
    (lambda: ko.Kron([_param(4, 3).t()]), ValueError, "parameter 0.*contiguous"),
    (lambda: ko.Kron([_param(3, 4)]), ValueError, "parameter 0.*one HIP device"),          # a CPU tensor
    (lambda: ko.Kron([]), ValueError, "no parameters"),
    (lambda: ko.Kron([_param(3, 4)], step_tail="foreach"), ValueError, "step_tail"),
    (lambda: ko.Kron([_param(3, 4)], [("dense", "dense"), ("dense", "dense")]), ValueError, "2 formats for 1 parameters"),
    (lambda: ko.Kron([_param(3, 4)], ("norm", "norm")), ValueError, "does not exist"),
    (lambda: ko.Kron([_param(3, 4)], ("dense", "diag")), ValueError, "pair of"),
])
def test_constructor_argument_errors(make, exc, match):
    with pytest.raises(exc, match=match):
        make()


# ----------------------------------------------------------------------------------------------------------------- formats
def test_format_table():
    from psgd_tf_amd import kron
    sides = ("dense", "norm", "scale")
    accepted = [(a, b) for a in sides for b in sides if (a, b) not in (("norm", "norm"), ("scale", "scale"))]
    assert sorted(accepted) == sorted(ko.KRON_PAIRS) and len(accepted) == 7
    for pair in accepted:
        assert ko.kron_formats(pair, 3) == [pair] * 3
        Ql, Qr = ko.kron_initial_factors((5, 7), pair)
        assert kron.kron_format(Ql.shape, Qr.shape) == "%s_%s" % pair            # the dispatcher sees the format that was asked for
    for pair in (("norm", "norm"), ("scale", "scale")):
        with pytest.raises(ValueError, match="does not exist"):
            ko.kron_formats(pair, 1)
        with pytest.raises(ValueError, match="does not exist"):
            ko.kron_formats([("dense", "dense"), pair], 2)
    assert ko.kron_formats("dense", 2) == [("dense", "dense")] * 2
    assert ko.kron_formats(("dense", "scale"), 2) == [("dense", "scale")] * 2          # two names: ONE pair, also for two parameters
    assert ko.kron_formats([("scale", "dense"), "dense", ["norm", "scale"]], 3) == \
        [("scale", "dense"), ("dense", "dense"), ("norm", "scale")]
    for bad in ("norm", "scale", 3, [("dense",)], ("dense", "dense", "dense")):
        with pytest.raises(ValueError):
            ko.kron_formats(bad, 1)


@pytest.mark.parametrize("pair", ko.KRON_PAIRS)
def test_initial_factors(pair):
    M, N, scale = 5, 7, 0.25
    Ql, Qr = ko.kron_initial_factors((M, N), pair, scale)
    want = {"dense": lambda n: np.eye(n), "scale": lambda n: np.ones((1, n)),
            "norm": lambda n: np.stack([np.ones(n), np.zeros(n)])}
    assert Ql.dtype == Qr.dtype == torch.float32
    np.testing.assert_array_equal(Ql.numpy(), (want[pair[0]](M) * scale).astype(np.float32))     # the LEFT factor carries the scale
    np.testing.assert_array_equal(Qr.numpy(), want[pair[1]](N).astype(np.float32))
    ref = kc.initial_factors((M, N), pair, scale)
    np.testing.assert_array_equal(Ql.numpy(), ref[0])
    np.testing.assert_array_equal(Qr.numpy(), ref[1])


def test_square_sparse_factors_are_refused_with_the_reason():
    """a scaling factor of a side of length 1 is (1, 1), a normalization factor of a side of length 2 is (2, 2): square, so the
    dispatcher would run them as dense factors"""
    for shape, pair in (((1, 7), ("scale", "dense")), ((7, 1), ("dense", "scale")), ((2, 7), ("norm", "dense")),
                        ((7, 2), ("dense", "norm")), ((2, 1), ("norm", "scale"))):
        with pytest.raises(ValueError, match="square like a dense one.*treat it as dense"):
            ko.kron_initial_factors(shape, pair)
    for shape, pair in (((1, 7), ("dense", "scale")), ((2, 7), ("dense", "norm")), ((1, 2), ("dense", "dense")),
                        ((2, 7), ("scale", "dense")), ((1, 7), ("norm", "dense"))):
        from psgd_tf_amd import kron
        Ql, Qr = ko.kron_initial_factors(shape, pair)                              # dense sides of length 1 or 2 are what they say
        assert kron.kron_format(Ql.shape, Qr.shape) == "%s_%s" % pair


# ----------------------------------------------------------------------------------------------------------------- checkpoint
def test_state_dict_round_trip_of_the_host_fields():
    shapes = [(5, 7), (4, 3)]
    formats = [("dense", "norm"), ("scale", "dense")]
    g = torch.Generator().manual_seed(5)
    factors = [[torch.randn(q.shape, generator=g) for q in ko.kron_initial_factors(s, f)] for s, f in zip(shapes, formats)]
    hyper = dict(lr_params=0.02, lr_preconditioner=0.05, grad_clip_max_norm=float("inf"), preconditioner_update_probability=0.5,
                 exact_hessian_vector_product=False)
    sd = ko._encode_state(factors, formats, shapes, hyper, g.get_state())
    assert sd["factors"][0][0] is not factors[0][0]                                  # clones, not views
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd2 = torch.load(buf, weights_only=True)                                        # tensors and plain Python values only
    f2, h2, rng2 = ko._decode_state(sd2, formats, shapes)
    for a, b in zip(factors, f2):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert h2 == hyper and type(h2["exact_hessian_vector_product"]) is bool
    g2 = torch.Generator()
    g2.set_state(rng2)
    assert torch.equal(torch.rand(4, generator=g), torch.rand(4, generator=g2))
    for key in ("format", "kind", "factors", "preconditioner_formats", "param_shapes", "hyper", "rng"):
        with pytest.raises(ValueError, match=key):
            ko._decode_state({k: v for k, v in sd.items() if k != key}, formats, shapes)
    with pytest.raises(ValueError, match="preconditioner_formats"):
        ko._decode_state(sd, formats[::-1], shapes)
    with pytest.raises(ValueError, match="param_shapes"):
        ko._decode_state(sd, formats, [(5, 7), (4, 4)])
    with pytest.raises(ValueError, match=r"'factors'\[1\]"):
        ko._decode_state(dict(sd, factors=[sd["factors"][0], sd["factors"][0]]), formats, shapes)
    with pytest.raises(ValueError, match="lr_params"):
        ko._decode_state(dict(sd, hyper={k: v for k, v in hyper.items() if k != "lr_params"}), formats, shapes)


# ----------------------------------------------------------------------------------------------------------------- C ABI
def test_exports_are_bound(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.psgd_abi_version() == 7                      # additive: the version did not move


def test_signatures_and_constants_match_the_header():
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
    consts = dict(re.findall(r"#define\s+(PSGD_MULTI_SUMSQ_WS_BYTES)\s+(\d+)", text))
    assert int(consts["PSGD_MULTI_SUMSQ_WS_BYTES"]) == _lib.MULTI_SUMSQ_WS_BYTES


def test_argument_checks(lib):
    """null tables, negative counts, a missing workspace: an error code with no device present; nchunks == 0 launches nothing"""
    BAD, OK = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_OK
    a, b, h, v, x, chunks, out, ws = (0x10000 * k for k in range(1, 9))              # never dereferenced: the checks fail first
    sumsq, upd, diff = lib.psgd_multi_sumsq_f32, lib.psgd_multi_param_update_f32, lib.psgd_multi_diff_scale_f32
    W = _lib.MULTI_SUMSQ_WS_BYTES
    assert sumsq(None, 3, chunks, 5, out, ws, W, None) == BAD
    assert sumsq(a, 3, None, 5, out, ws, W, None) == BAD
    assert sumsq(a, 3, chunks, 5, None, ws, W, None) == BAD
    assert sumsq(a, 3, chunks, 5, out + 4, ws, W, None) == BAD
    assert sumsq(a, 3, chunks, 5, out, None, W, None) == BAD
    assert sumsq(a, -1, chunks, 5, out, ws, W, None) == BAD
    assert sumsq(a, 3, chunks, -5, out, ws, W, None) == BAD
    assert sumsq(a, 3, chunks, 5, out, ws, W - 1, None) == _lib.PSGD_ERR_WORKSPACE
    assert sumsq(a, 3, chunks, 5, out, ws + 4, W, None) == _lib.PSGD_ERR_WORKSPACE
    assert sumsq(a, 3, chunks, 0, out, ws, W, None) == OK
    tail = (0.1, None, 0.0, 1e-38, None)
    assert upd(None, b, None, 3, chunks, 5, *tail) == BAD
    assert upd(a, b, None, 3, None, 5, *tail) == BAD
    assert upd(a, b, None, -3, chunks, 5, *tail) == BAD
    assert upd(a, b, None, 3, chunks, -1, *tail) == BAD
    assert upd(a, None, None, 3, chunks, 5, *tail) == BAD                            # neither a gradient nor vs
    assert upd(a, None, v, 3, chunks, 5, 0.1, out, 1.0, 1e-38, None) == BAD          # a clip norm without a gradient
    assert upd(a, b, v, 3, chunks, 0, *tail) == OK
    assert upd(a, None, v, 3, chunks, 0, *tail) == OK
    assert diff(None, b, h, None, None, 3, chunks, 5, 2.0, None) == BAD
    assert diff(a, None, h, None, None, 3, chunks, 5, 2.0, None) == BAD
    assert diff(a, b, None, None, None, 3, chunks, 5, 2.0, None) == BAD
    assert diff(a, b, h, None, None, 3, None, 5, 2.0, None) == BAD
    assert diff(a, b, h, v, None, 3, chunks, 5, 2.0, None) == BAD                    # v and x go together
    assert diff(a, b, h, None, x, 3, chunks, 5, 2.0, None) == BAD
    assert diff(a, b, h, None, None, -1, chunks, 5, 2.0, None) == BAD
    assert diff(a, b, h, None, None, 3, chunks, -5, 2.0, None) == BAD
    assert diff(a, b, h, v, x, 3, chunks, 0, 2.0, None) == OK


def test_wrappers_refuse_what_the_kernels_cannot_take():
    """checked before a plan is made or the library is called: a CPU machine sees the same errors"""
    t = torch.zeros(3, 4)
    with pytest.raises(TypeError, match=r"tensors\[0\] is not a torch tensor"):
        ko.multi_sumsq([3.0, t])
    with pytest.raises(TypeError, match=r"tensors\[0\] must be float32"):
        ko.multi_sumsq([t.double()])
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        ko.multi_sumsq([t])
    with pytest.raises(ValueError, match="empty tensor list"):
        ko.multi_sumsq([])
    with pytest.raises(TypeError, match=r"params\[0\] must be float32"):
        ko.multi_param_update([t.half()], [t])
    with pytest.raises(ValueError, match="v and x go together"):
        ko.multi_diff_scale([t], [t], [t], v=[t])


# ----------------------------------------------------------------------------------------------------------------- restatement
def _two_layer(seed=0):
    shapes = [(6, 4), (3, 5)]
    Ws, Hls, Hrs = kc.quadratic_problem(shapes, seed)
    grad_fn = lambda W: kc.quadratic_grads(W, Hls, Hrs)
    hvp_fn = lambda vs: kc.quadratic_grads(vs, Hls, Hrs)                               # the Hessian of a quadratic is its gradient map
    return shapes, Ws, Hls, Hrs, grad_fn, hvp_fn


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("formats", [[("dense", "dense")] * 2, [("dense", "scale"), ("norm", "dense")]])
def test_restatement_loss_falls(exact, formats):
    shapes, Ws, Hls, Hrs, grad_fn, hvp_fn = _two_layer()
    rng = np.random.default_rng(1)
    Qs = [kc.initial_factors(s, f) for s, f in zip(shapes, formats)]
    loss0 = kc.quadratic_loss(Ws, Hls, Hrs)
    for _ in range(50):
        vs = [rng.standard_normal(s) * (1.0 if exact else kc.DELTA32) for s in shapes]
        Ws, Qs, pre, _ = kc.kron_step_f64(Ws, Qs, grad_fn, hvp_fn, vs, lr_params=0.05, lr_preconditioner=0.05, max_norm=10.0,
                                          exact=exact)
    loss1 = kc.quadratic_loss(Ws, Hls, Hrs)
    assert all(np.isfinite(q).all() for pair in Qs for q in pair)
    assert loss1 < 0.5 * loss0, (loss0, loss1)


@pytest.mark.parametrize("exact", [True, False])
def test_restatement_clipped_step_has_norm_lr_times_max_norm(exact):
    shapes, Ws, Hls, Hrs, grad_fn, hvp_fn = _two_layer(3)
    rng = np.random.default_rng(2)
    Qs = [kc.initial_factors(s, ("dense", "dense")) for s in shapes]
    lr, max_norm = 0.1, 1e-3
    for _ in range(50):
        vs = [rng.standard_normal(s) * (1.0 if exact else kc.DELTA32) for s in shapes]
        new, Qs, pre, lr_eff = kc.kron_step_f64(Ws, Qs, grad_fn, hvp_fn, vs, lr_params=lr, lr_preconditioner=0.05,
                                                max_norm=max_norm, exact=exact)
        assert lr_eff < lr                                                             # the clip is active
        step = np.sqrt(sum(float(np.sum((lr_eff * g) ** 2)) for g in pre))             # the norm of the step the rule takes
        assert abs(step - lr * max_norm) <= 1e-12 * lr * max_norm
        if exact:                                                                      # ... and of the parameters' move
            moved = np.sqrt(sum(float(np.sum((a - b) ** 2)) for a, b in zip(new, Ws)))
            assert abs(moved - lr * max_norm) <= 1e-9 * lr * max_norm                  # (limited by the rounding of W - step)
        Ws = new


def test_restatement_zero_gradient_takes_a_zero_step():
    """the + tiny of psgd.py:753: a zero gradient clips to a zero step, where mnist_with_lenet5.py:54-55 would divide by zero"""
    shapes = [(3, 2)]
    Ws = [np.zeros(shapes[0])]
    Qs = [kc.initial_factors(shapes[0], ("dense", "dense"))]
    zero = lambda W: [np.zeros_like(w) for w in W]
    new, _, pre, lr_eff = kc.kron_step_f64(Ws, Qs, zero, None, None, lr_params=0.1, lr_preconditioner=0.1, max_norm=1.0, update=False)
    assert np.isfinite(lr_eff) and (new[0] == 0).all()
