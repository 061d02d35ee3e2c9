"""Momentum, weight decay, the non-finite guard and the loss scale of class Kron, the part that needs no GPU: the C ABI of the three
list kernels they add (header = exports = ctypes table, argument checks that return before any HIP call), constructor validation,
the host part of the checkpoint, and that the schedule functions are those of class UVd."""
import ctypes
import os
import re

import pytest
import torch

from psgd_tf_amd import _lib
from psgd_tf_amd import kron_optimizer as ko

NAMES = ("psgd_multi_blend_f32", "psgd_multi_scale_check_f32", "psgd_multi_param_update_wd_f32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")
PARENT_KEYS = {"format", "kind", "factors", "preconditioner_formats", "param_shapes", "hyper", "rng"}     # state_dict() before this


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def _param(*shape, **kw):
    return torch.zeros(*shape, requires_grad=True, **kw)


# ------------------------------------------------------------------------------------------------------------------- C ABI
def test_exports_are_bound_and_the_version_did_not_move(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
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
    assert re.search(r"psgd_multi_blend_f32.*still 7", text, re.S)                       # the version note has its line


def test_argument_checks(lib):
    """null tables, negative counts, a flag without a stamp, nothing to do: an error code with no device present; nchunks == 0
    launches nothing"""
    BAD, OK = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_OK
    a, b, c, v, chunks, flag, out = (0x10000 * k for k in range(1, 8))                  # never dereferenced: the checks fail first
    blend, check, upd = lib.psgd_multi_blend_f32, lib.psgd_multi_scale_check_f32, lib.psgd_multi_param_update_wd_f32
    assert blend(None, b, 3, chunks, 5, 0.5, 0.5, None) == BAD
    assert blend(a, None, 3, chunks, 5, 0.5, 0.5, None) == BAD
    assert blend(a, b, 3, None, 5, 0.5, 0.5, None) == BAD
    assert blend(a, b, -1, chunks, 5, 0.5, 0.5, None) == BAD
    assert blend(a, b, 3, chunks, -5, 0.5, 0.5, None) == BAD
    assert blend(a, b, 3, chunks, 0, 0.5, 0.5, None) == OK
    assert blend(a, b, 3, chunks, 0, 0.0, 1.0, None) == OK
    assert check(None, b, c, 0.5, 0.5, 1.0, 3, chunks, 5, flag, 1, None) == BAD
    assert check(a, b, c, 0.5, 0.5, 1.0, 3, None, 5, flag, 1, None) == BAD
    assert check(a, b, c, 0.5, 0.5, 1.0, -3, chunks, 5, flag, 1, None) == BAD
    assert check(a, b, c, 0.5, 0.5, 1.0, 3, chunks, -1, flag, 1, None) == BAD
    assert check(a, b, c, 0.5, 0.5, 1.0, 3, chunks, 5, flag, 0, None) == BAD            # a flag needs a stamp >= 1
    assert check(a, b, c, 0.5, 0.5, 1.0, 3, chunks, 5, flag, -7, None) == BAD
    assert check(a, None, None, 1.0, 1.0, 1.0, 3, chunks, 0, flag, 0, None) == BAD      # ... also when there is nothing to launch
    assert check(a, b, c, 1.0, 1.0, 1.0, 3, chunks, 5, None, 1, None) == BAD            # no flag, every scale 1: nothing to do
    assert check(a, None, None, 1.0, 0.5, 0.5, 3, chunks, 5, None, 0, None) == BAD      # (the scales of absent lists do not count)
    assert check(a, b, c, 0.5, 0.5, 1.0, 3, chunks, 0, flag, 1, None) == OK
    assert check(a, None, None, 1.0, 1.0, 1.0, 3, chunks, 0, flag, 2 ** 31 - 1, None) == OK
    assert check(a, None, c, 0.5, 1.0, 1.0, 3, chunks, 0, None, 0, None) == OK          # a pure rescale ignores the stamp
    tail = (0.1, None, 0.0, 1e-38)
    assert upd(None, b, None, 3, chunks, 5, *tail, 0.01, None) == BAD
    assert upd(a, b, None, 3, None, 5, *tail, 0.01, None) == BAD
    assert upd(a, b, None, -3, chunks, 5, *tail, 0.01, None) == BAD
    assert upd(a, b, None, 3, chunks, -1, *tail, 0.01, None) == BAD
    assert upd(a, None, None, 3, chunks, 5, *tail, 0.0, None) == BAD                    # neither a gradient nor vs
    assert upd(a, None, v, 3, chunks, 5, 0.1, out, 1.0, 1e-38, 0.0, None) == BAD        # a clip norm without a gradient
    assert upd(a, None, v, 3, chunks, 5, *tail, 0.01, None) == BAD                      # the perturbation takes no decay
    assert upd(a, None, v, 3, chunks, 0, *tail, 0.01, None) == BAD                      # ... whatever nchunks
    assert upd(a, b, v, 3, chunks, 0, *tail, 0.01, None) == OK
    assert upd(a, None, v, 3, chunks, 0, *tail, 0.0, None) == OK


def test_wrappers_refuse_what_the_kernels_cannot_take():
    t = torch.zeros(3, 4)
    with pytest.raises(TypeError, match=r"ms\[0\] must be float32"):
        ko.multi_blend([t.double()], [t], 0.5, 0.5)
    with pytest.raises(ValueError, match=r"beta must be in \[0, 1\)"):
        ko.multi_blend([t], [t], 1.0, 0.0)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        ko.multi_blend([t], [t], 0.5, 0.5)
    with pytest.raises(ValueError, match="one to three lists"):
        ko.multi_scale_check([], [])
    with pytest.raises(ValueError, match="one to three lists"):
        ko.multi_scale_check([[t]] * 4, [0.5] * 4)
    with pytest.raises(ValueError, match="one to three lists"):
        ko.multi_scale_check([[t], [t]], [0.5])
    with pytest.raises(ValueError, match="flag and stamp go together"):
        ko.multi_scale_check([[t]], [0.5], stamp=3)
    with pytest.raises(ValueError, match="nothing to do"):
        ko.multi_scale_check([[t], [t]], [1.0, 1.0])
    with pytest.raises(TypeError, match=r"lists\[0\]\[0\] must be float32"):
        ko.multi_scale_check([[t.half()], [t]], [0.5, 1.0])
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        ko.multi_scale_check([[t], [t]], [0.5, 1.0])
    with pytest.raises(ValueError, match="weight_decay must be >= 0"):
        ko.multi_param_update([t], [t], weight_decay=-1.0)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        ko.multi_param_update([t], [t], None, 0.1, None, None, None, weight_decay=0.5)    # the old positional order still holds


# ------------------------------------------------------------------------------------------------------------- constructor
@pytest.mark.parametrize("kw, match", [
    (dict(momentum=1.0), "momentum must be in"),
    (dict(momentum=-0.1), "momentum must be in"),
    (dict(momentum=float("nan")), "momentum must be in"),
    (dict(weight_decay=-1e-3), "weight_decay must be >= 0"),
    (dict(weight_decay=float("nan")), "weight_decay must be >= 0"),
    (dict(nonfinite="raise"), "nonfinite must be"),
    (dict(loss_scale=1024.0), "loss_scale needs nonfinite='skip'"),
    (dict(loss_scale="dynamic"), "loss_scale needs nonfinite='skip'"),
    (dict(nonfinite="skip", loss_scale="auto"), "loss_scale must be None, a power of two or 'dynamic'"),
    (dict(nonfinite="skip", loss_scale=1000.0), "loss_scale must be a power of two"),
    (dict(nonfinite="skip", loss_scale=0.0), "loss_scale must be a power of two"),
    (dict(nonfinite="skip", loss_scale=-4.0), "loss_scale must be a power of two"),
    (dict(nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=0), "loss_scale_growth_interval must be >= 1"),
])
def test_constructor_validation_names_the_argument(kw, match):
    """checked before the parameters' device is looked at: a CPU parameter gets this far"""
    with pytest.raises(ValueError, match=match):
        ko.Kron([_param(3, 4)], **kw)


def test_valid_feature_arguments_reach_the_device_check():
    for kw in (dict(momentum=0.9, weight_decay=0.01), dict(nonfinite="skip"), dict(nonfinite="skip", loss_scale=2.0 ** 8),
               dict(nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=2)):
        with pytest.raises(ValueError, match="one HIP device"):
            ko.Kron([_param(3, 4)], **kw)


def test_the_new_arguments_are_keyword_only():
    with pytest.raises(TypeError):
        ko.Kron([_param(3, 4)], "dense", 1.0, 0.01, 0.01, None, 1.0, True, 0.9)


# -------------------------------------------------------------------------------------------------------------- checkpoint
def _host_state():
    shapes = [(5, 7), (4, 3)]
    formats = [("dense", "norm"), ("scale", "dense")]
    g = torch.Generator().manual_seed(5)
    factors = [[torch.randn(q.shape, generator=g) for q in ko.kron_initial_factors(s, f)] for s, f in zip(shapes, formats)]
    hyper = dict(lr_params=0.02, lr_preconditioner=0.05, grad_clip_max_norm=float("inf"), preconditioner_update_probability=0.5,
                 exact_hessian_vector_product=False)
    return shapes, formats, hyper, ko._encode_state(factors, formats, shapes, hyper, g.get_state()), g


def test_state_dict_keys_with_the_features_off_are_the_parents():
    shapes, formats, hyper, sd, _ = _host_state()
    assert set(sd) == PARENT_KEYS
    sd = ko._encode_features(sd, 0.0, 0.0)
    assert set(sd) == PARENT_KEYS
    assert set(sd["hyper"]) == set(hyper) | {"momentum", "weight_decay"}
    assert sd["hyper"]["momentum"] == 0.0 and sd["hyper"]["weight_decay"] == 0.0
    sd = ko._encode_features(sd, 0.0, 0.01)                                             # weight decay has no state of its own
    assert set(sd) == PARENT_KEYS and sd["hyper"]["weight_decay"] == 0.01


def test_state_dict_keys_with_the_features_on():
    shapes, formats, hyper, sd, g = _host_state()
    bufs = [torch.randn(s, generator=g) for s in shapes]
    sd = ko._encode_features(sd, 0.9, 0.01, bufs, 4, True, 2, 2.0 ** 15, 7)
    assert set(sd) == PARENT_KEYS | {"momentum_buffers", "momentum_step", "nonfinite", "skipped_steps", "loss_scale",
                                     "loss_scale_good_steps"}
    assert sd["momentum_step"] == 4 and sd["nonfinite"] == "skip" and sd["skipped_steps"] == 2
    assert sd["loss_scale"] == 2.0 ** 15 and sd["loss_scale_good_steps"] == 7
    assert all(m is not b and torch.equal(m, b) and m.device.type == "cpu" for m, b in zip(sd["momentum_buffers"], bufs))
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    sd2 = torch.load(buf, weights_only=True)                                            # tensors and plain Python values only
    m2, k2 = ko._decode_features(sd2, shapes)
    assert k2 == 4 and all(torch.equal(a, b) for a, b in zip(m2, bufs))
    only_guard = ko._encode_features(_host_state()[3], 0.0, 0.0, None, 0, True, 0, None, 0)
    assert set(only_guard) == PARENT_KEYS | {"nonfinite", "skipped_steps", "loss_scale", "loss_scale_good_steps"}
    assert only_guard["loss_scale"] is None
    only_momentum = ko._encode_features(_host_state()[3], 0.5, 0.0, bufs, 1)
    assert set(only_momentum) == PARENT_KEYS | {"momentum_buffers", "momentum_step"}


def test_an_old_style_dict_loads_and_bad_buffers_are_named():
    shapes, formats, hyper, sd, g = _host_state()
    ko._decode_state(sd, formats, shapes)                                               # 'hyper' without momentum / weight_decay
    assert ko._decode_features(sd, shapes) == (None, 0)
    bufs = [torch.zeros(s) for s in shapes]
    with pytest.raises(ValueError, match="momentum_step"):
        ko._decode_features(dict(sd, momentum_buffers=bufs), shapes)
    with pytest.raises(ValueError, match="momentum_buffers"):
        ko._decode_features(dict(sd, momentum_buffers=bufs[:1], momentum_step=1), shapes)
    with pytest.raises(ValueError, match="momentum_buffers"):
        ko._decode_features(dict(sd, momentum_buffers=[b.double() for b in bufs], momentum_step=1), shapes)
    with pytest.raises(ValueError, match="momentum_buffers"):
        ko._decode_features(dict(sd, momentum_buffers=[bufs[0], bufs[1].t()], momentum_step=1), shapes)


# ---------------------------------------------------------------------------------------------------------------- schedules
def test_the_schedules_are_those_of_class_uvd(monkeypatch):
    """class Kron looks uvd_momentum_coefficients and uvd_loss_scale_next up on the UVd module at the call: no restatement"""
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as m
    assert ko._psgd is m
    assert not hasattr(ko, "uvd_momentum_coefficients") and not hasattr(ko, "uvd_loss_scale_next")
    opt = object.__new__(ko.Kron)                                                      # the book-keeping needs no device
    opt._params, opt._dynamic_scale, opt._good_steps = [], True, 0
    opt.skipped_steps, opt.last_step_skipped = 0, False
    opt.loss_scale, opt.loss_scale_growth_interval = m._Hyper(2.0 ** 16), 2
    calls = []
    real = m.uvd_loss_scale_next
    monkeypatch.setattr(m, "uvd_loss_scale_next", lambda *a, **k: calls.append((a, k)) or real(*a, **k))
    opt._guard_outcome(True)
    assert float(opt.loss_scale) == 2.0 ** 15 and opt.skipped_steps == 1 and opt.last_step_skipped
    opt._guard_outcome(False)
    opt._guard_outcome(False)
    assert float(opt.loss_scale) == 2.0 ** 16 and opt.skipped_steps == 1 and not opt.last_step_skipped
    assert len(calls) == 3 and calls[0][1] == {"growth_interval": 2}
    seen = []
    real_c = m.uvd_momentum_coefficients
    monkeypatch.setattr(m, "uvd_momentum_coefficients", lambda k, mom: seen.append((k, mom)) or real_c(k, mom))
    opt._m_step, opt._tail, opt._m = 0, None, [torch.full((2, 3), float("nan"))]
    g = [torch.arange(6.0).reshape(2, 3)]
    with torch.no_grad():
        out = opt._blend(g, 0.9)
        assert out is opt._m and torch.equal(out[0], g[0])                              # beta_0 = 0: the NaN buffer is not read
        opt._blend(g, 0.9)
    assert seen == [(0, 0.9), (1, 0.9)] and opt._m_step == 2
    assert opt._blend(g, 0.0) is g and opt._m_step == 0                                 # momentum == 0 resets the warm-up
