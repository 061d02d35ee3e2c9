"""The host side of the guarded step of class UVd (nonfinite="skip", loss_scale): the dynamic-scale schedule against a table written
out by hand, what the constructor refuses, the two new symbols of the C ABI (psgd_uvd_pack_check_f32, psgd_uvd_check_multi: in the
header, exported, bound, argument checks before any HIP call, ABI still 7), and what a checkpoint holds.  The kernels and the step
are checked on the GPU in test_uvd_guard_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

from psgd_tf_amd import _lib, sharded
from psgd_tf_amd.preconditioned_stochastic_gradient_descent import UVd, _Hyper, uvd_loss_scale_next

NAMES = ("psgd_uvd_pack_check_f32", "psgd_uvd_check_multi")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")
UNGUARDED_KEYS = {"format", "U", "V", "d", "rank", "num_params", "num_params_global", "row0", "param_sizes", "state_dtype",
                  "state_route", "state_rounding", "hyper", "branch_rng"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def test_loss_scale_schedule_table():
    # (scale, good_steps, skipped) -> (scale, good_steps), growth_interval = 3
    table = [
        ((65536.0, 0, False), (65536.0, 1)),
        ((65536.0, 1, False), (65536.0, 2)),
        ((65536.0, 2, False), (131072.0, 0)),          # the third good step in a row doubles and resets
        ((131072.0, 0, True), (65536.0, 0)),           # a skip halves
        ((65536.0, 2, True), (32768.0, 0)),            # ... and resets the counter whatever it was
        ((32768.0, 0, False), (32768.0, 1)),
        ((2.0, 0, True), (1.0, 0)),
        ((1.0, 0, True), (1.0, 0)),                    # clamp below: min_scale = 1
        ((1.0, 1, True), (1.0, 0)),
        ((2.0 ** 24, 2, False), (2.0 ** 24, 0)),       # clamp above: max_scale = 2^24, the counter resets all the same
        ((2.0 ** 23, 2, False), (2.0 ** 24, 0)),
    ]
    for (scale, good, skipped), want in table:
        assert uvd_loss_scale_next(scale, good, skipped, growth_interval=3) == want, (scale, good, skipped)
    assert uvd_loss_scale_next(8.0, 0, False, growth_interval=1) == (16.0, 0)
    assert uvd_loss_scale_next(8.0, 0, True, growth_interval=5, backoff=0.25, min_scale=4.0) == (4.0, 0)
    assert uvd_loss_scale_next(8.0, 4, False, growth_interval=5, growth=4.0, max_scale=16.0) == (16.0, 0)
    # a run: 2^16, two skips, then growth every 2 good steps -- powers of two throughout
    scale, good, seen = 2.0 ** 16, 0, []
    for skipped in (True, True, False, False, False, True, False, False):
        scale, good = uvd_loss_scale_next(scale, good, skipped, growth_interval=2)
        seen.append((scale, good))
    assert seen == [(32768.0, 0), (16384.0, 0), (16384.0, 1), (32768.0, 0), (32768.0, 1), (16384.0, 0), (16384.0, 1), (32768.0, 0)]


def test_constructor_validation():
    p = [torch.zeros(3, requires_grad=True)]
    kw = dict(rank_of_modification=2, placement=None)
    with pytest.raises(ValueError, match="nonfinite"):
        UVd(p, nonfinite="ignore", **kw)
    for scale in (1024.0, "dynamic"):
        with pytest.raises(ValueError, match="loss_scale needs nonfinite='skip'"):
            UVd(p, loss_scale=scale, **kw)
        with pytest.raises(ValueError, match="loss_scale needs nonfinite='skip'"):
            UVd(p, loss_scale=scale, nonfinite="propagate", **kw)
    for scale in (1000.0, 3.0, 0.0, -2.0, float("inf"), float("nan"), "auto"):
        with pytest.raises(ValueError, match="loss_scale"):
            UVd(p, nonfinite="skip", loss_scale=scale, **kw)
    with pytest.raises(ValueError, match="loss_scale_growth_interval"):
        UVd(p, nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=0, **kw)
    opt = UVd(p, nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=7, **kw)
    assert isinstance(opt.loss_scale, _Hyper) and float(opt.loss_scale) == 2.0 ** 16 and opt.loss_scale_growth_interval == 7
    assert opt.last_step_skipped is False and opt.skipped_steps == 0
    assert float(UVd(p, nonfinite="skip", loss_scale=0.5, **kw).loss_scale) == 0.5          # a power of two below 1 is one too
    off = UVd(p, **kw)
    assert off.loss_scale.value is None and off.last_step_skipped is False and off.skipped_steps == 0
    assert UVd(p, nonfinite="skip", **kw).loss_scale.value is None


def test_symbols_are_declared_exported_and_bound(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "int32_t": ctypes.c_int32}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "not declared in psgd_hip.h: " + name
        assert hasattr(raw, name), "not exported: " + name
        assert name in _lib.SIGNATURES, "not bound in _lib.py: " + name
        restype, argtypes = _lib.SIGNATURES[name]
        params = [q.strip() for q in m.group(1).split(",")]
        assert restype is ctypes.c_int and len(params) == len(argtypes), name
        for q, t in zip(params, argtypes):
            assert t is (ctypes.c_void_p if "*" in q else kinds[q.split()[0]]), (name, q)
    assert lib.psgd_abi_version() == _lib.PSGD_ABI_VERSION == 7
    # the checked pack takes the plain pack's arguments with (flag, stamp) in front of the stream; the check has no `out`
    old = _lib.SIGNATURES["psgd_uvd_pack_f32"][1]
    assert _lib.SIGNATURES[NAMES[0]][1] == old[:-1] + [ctypes.c_void_p, ctypes.c_int32] + old[-1:]
    assert _lib.SIGNATURES[NAMES[1]][1] == old[:6] + [ctypes.c_void_p, ctypes.c_int32] + old[-1:]


def test_argument_checks_return_before_any_hip_call(lib):
    BAD = _lib.PSGD_ERR_BAD_ARG
    segs, chunks, out, flag = (0x10000 * k for k in range(1, 5))                    # never dereferenced: the checks fail first
    pack, check = lib.psgd_uvd_pack_check_f32, lib.psgd_uvd_check_multi
    assert pack(segs, 3, chunks, 5, 0, 1.0, out, None, 1, None) == BAD              # no flag
    assert check(segs, 3, chunks, 5, 0, 1.0, None, 1, None) == BAD
    for stamp in (0, -1, -2 ** 31):
        assert pack(segs, 3, chunks, 5, 0, 1.0, out, flag, stamp, None) == BAD
        assert check(segs, 3, chunks, 5, 0, 1.0, flag, stamp, None) == BAD
    assert pack(segs, 3, chunks, 0, 0, 1.0, out, flag, 0, None) == BAD              # ... also where there is nothing to launch
    assert check(segs, 3, chunks, 0, 0, 1.0, None, 1, None) == BAD
    assert pack(None, 3, chunks, 5, 0, 1.0, out, flag, 1, None) == BAD
    assert pack(segs, 3, None, 5, 0, 1.0, out, flag, 1, None) == BAD
    assert pack(segs, 3, chunks, 5, 0, 1.0, None, flag, 1, None) == BAD
    assert pack(segs, -1, chunks, 5, 0, 1.0, out, flag, 1, None) == BAD
    assert pack(segs, 3, chunks, -5, 0, 1.0, out, flag, 1, None) == BAD
    assert pack(segs, 3, chunks, 5, 3, 1.0, out, flag, 1, None) == BAD
    assert check(None, 3, chunks, 5, 0, 1.0, flag, 1, None) == BAD
    assert check(segs, 3, None, 5, 0, 1.0, flag, 1, None) == BAD
    assert check(segs, -1, chunks, 5, 0, 1.0, flag, 1, None) == BAD
    assert check(segs, 3, chunks, -5, 0, 1.0, flag, 1, None) == BAD
    assert check(segs, 3, chunks, 5, -1, 1.0, flag, 1, None) == BAD
    for stamp in (1, 2 ** 31 - 1):
        assert pack(segs, 3, chunks, 0, 2, 1.0, out, flag, stamp, None) == _lib.PSGD_OK     # no chunk: nothing to launch
        assert check(segs, 3, chunks, 0, 1, 1.0, flag, stamp, None) == _lib.PSGD_OK


def test_state_dict_keys():
    p = [torch.zeros(5, requires_grad=True)]
    kw = dict(rank_of_modification=2, placement=None)
    assert set(UVd(p, **kw).state_dict()) == UNGUARDED_KEYS                         # what it is without the feature
    assert set(UVd(p, momentum=0.5, **kw).state_dict()) == UNGUARDED_KEYS | {"momentum_buffer", "momentum_step"}
    opt = UVd(p, nonfinite="skip", loss_scale="dynamic", **kw)
    opt.skipped_steps, opt._good_steps = 3, 5
    opt.loss_scale.assign(2.0 ** 12)
    sd = opt.state_dict()
    assert set(sd) == UNGUARDED_KEYS | {"nonfinite", "skipped_steps", "loss_scale", "loss_scale_good_steps"}
    assert (sd["nonfinite"], sd["skipped_steps"], sd["loss_scale"], sd["loss_scale_good_steps"]) == ("skip", 3, 4096.0, 5)
    fresh = UVd(p, nonfinite="skip", loss_scale="dynamic", **kw)
    fresh.load_state_dict(sd)
    assert (fresh.skipped_steps, float(fresh.loss_scale), fresh._good_steps, fresh.last_step_skipped) == (3, 4096.0, 5, False)
    fresh.load_state_dict(UVd(p, **kw).state_dict())                                # a dict of an unguarded optimizer: a fresh start
    assert (fresh.skipped_steps, float(fresh.loss_scale), fresh._good_steps) == (0, 4096.0, 0)
    assert UVd(p, nonfinite="skip", **kw).state_dict()["loss_scale"] is None
    UVd(p, **kw).load_state_dict(sd)                                                # an unguarded optimizer ignores the keys


def test_reshard_carries_the_guard_keys_and_requires_them_equal():
    def dicts():
        out = []
        for lo, hi in ((0, 128), (128, 200)):
            out.append({"format": 1, "U": torch.ones(hi - lo, 2), "V": torch.ones(hi - lo, 2), "d": torch.ones(hi - lo, 1), "rank": 2,
                        "num_params": hi - lo, "num_params_global": 200, "row0": lo, "param_sizes": [hi - lo],
                        "state_dtype": "torch.float32", "state_route": "widen", "state_rounding": "none", "hyper": {"lr_params": 0.01},
                        "branch_rng": torch.Generator().manual_seed(3).get_state(), "nonfinite": "skip", "skipped_steps": 2,
                        "loss_scale": 1024.0, "loss_scale_good_steps": 7})
        return out
    three = sharded.reshard_uvd_state(dicts(), [64, 64, 72])
    for s in three:
        assert (s["nonfinite"], s["skipped_steps"], s["loss_scale"], s["loss_scale_good_steps"]) == ("skip", 2, 1024.0, 7)
    for key, other in (("skipped_steps", 3), ("loss_scale", 512.0), ("loss_scale_good_steps", 0), ("nonfinite", None)):
        sds = dicts()
        sds[1][key] = other
        with pytest.raises(ValueError, match=key):
            sharded.reshard_uvd_state(sds, [200])
