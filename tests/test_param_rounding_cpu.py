"""param_rounding="stochastic" of class UVd and class Kron, the part that needs no GPU: the C ABI of the three stochastic step-tail
entry points (header = exports = ctypes table, argument checks that return before any HIP call), the torch restatement of the hash
against a pure-Python restatement of bf16s::narrow's mode 1 (bf16_state.h), constructor errors, and the checkpoint rules."""
import ctypes
import os
import re
import struct

import pytest
import torch

from psgd_tf_amd import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, sharded
from psgd_tf_amd import kron_optimizer as ko

NAMES = ("psgd_uvd_param_update_multi_sr", "psgd_multi_param_update_sr", "psgd_multi_param_update_mixed_sr")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")
M32, M64 = 2 ** 32 - 1, 2 ** 64 - 1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------- C ABI
def test_exports_are_bound_and_the_version_did_not_move(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.psgd_abi_version() == 7 == _lib.PSGD_ABI_VERSION


def test_signatures_match_the_header():
    text = open(HEADER).read()
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
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
        assert params[-3].startswith("uint64_t seed") and params[-2].startswith("int64_t index0"), name
    assert re.search(r"psgd_uvd_param_update_multi_sr.*still 7", text, re.S)             # the version note has its line
    assert "16" in open(os.path.join(os.path.dirname(_lib.LIB_PATH), "bf16_state.h")).read().split("#pragma once")[0]


def test_argument_checks(lib):
    """the checks of the siblings, bf16 only, index0 >= 0, a gradient required: an error code with no device present"""
    BAD, OK, BF, F32, F16 = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_OK, _lib.DTYPE_BF16, _lib.DTYPE_F32, _lib.DTYPE_F16
    p, g, v, chunks, out = (0x10000 * k for k in range(1, 6))                           # never dereferenced: the checks fail first
    tail = (0.1, None, 0.0, 1e-38, 0.01, 7, 0, None)                                    # lr, sumsq, max_norm, tiny, wd, seed, index0
    uvd = lib.psgd_uvd_param_update_multi_sr
    assert uvd(None, v, 3, chunks, 5, BF, g, *tail) == BAD
    assert uvd(p, v, 3, None, 5, BF, g, *tail) == BAD
    assert uvd(p, v, -1, chunks, 5, BF, g, *tail) == BAD
    assert uvd(p, v, 3, chunks, -5, BF, g, *tail) == BAD
    assert uvd(p, v, 3, chunks, 5, F32, g, *tail) == BAD
    assert uvd(p, v, 3, chunks, 5, F16, g, *tail) == BAD
    assert uvd(p, v, 3, chunks, 5, 3, g, *tail) == BAD
    assert uvd(p, v, 3, chunks, 5, BF, None, *tail) == BAD                              # p + v stays round-to-nearest
    assert uvd(p, v, 3, chunks, 5, BF, g, 0.1, None, 0.0, 1e-38, 0.01, 7, -1, None) == BAD
    assert uvd(p, v, 3, chunks, 0, BF, g, *tail) == OK
    assert uvd(p, None, 3, chunks, 0, BF, g, 0.1, out, 1.0, 1e-38, 0.0, 2 ** 64 - 1, 2 ** 40, None) == OK
    for name in NAMES[1:]:
        upd = getattr(lib, name)
        assert upd(None, g, v, 3, chunks, 5, BF, *tail) == BAD
        assert upd(p, None, v, 3, chunks, 5, BF, *tail) == BAD                          # p + v stays round-to-nearest
        assert upd(p, g, v, 3, None, 5, BF, *tail) == BAD
        assert upd(p, g, v, -3, chunks, 5, BF, *tail) == BAD
        assert upd(p, g, v, 3, chunks, -1, BF, *tail) == BAD
        assert upd(p, g, v, 3, chunks, 5, F32, *tail) == BAD
        assert upd(p, g, v, 3, chunks, 5, F16, *tail) == BAD
        assert upd(p, g, v, 3, chunks, 5, BF, 0.1, None, 0.0, 1e-38, 0.01, 7, -1, None) == BAD
        assert upd(p, g, v, 3, chunks, 0, BF, *tail) == OK
        assert upd(p, g, None, 3, chunks, 0, BF, 0.1, out, 1.0, 1e-38, 0.0, 2 ** 64 - 1, 2 ** 40, None) == OK


# ------------------------------------------------------------------------------------------------------------------- the hash
def _mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _key(seed, tensor):
    """bf16s::key64 / make_key"""
    z = _mix64(_mix64((seed + 0x9E3779B97F4A7C15) & M64) ^ ((0xD1B54A32D192ED03 * (tensor + 1)) & M64))
    return z & M32, z >> 32


def _addend(a, b, idx):
    """the `add` of bf16s::narrow(x, 1, key, idx), line by line"""
    z = ((idx & M32) * 0x9E3779B1 + a + (idx >> 32) * 0x85EBCA77) & M32
    z ^= z >> 16
    z = (z * 0x7FEB352D) & M32
    z ^= b
    z ^= z >> 15
    z = (z * 0x846CA68B) & M32
    z ^= z >> 16
    return z >> 16


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


SEEDS = [0, 1, 0x50534744, 2 ** 62 - 1, 2 ** 64 - 1]
INDICES = [0, 1, 2, 255, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 3 * 2 ** 32 + 12345, 2 ** 40 + 7,
           2 ** 62 + 2 ** 32 + 5]


def test_the_key_is_make_key_of_tensor_16(lib):
    for seed in SEEDS:
        want = lib.psgd_uvd_bf16_rounding_key(seed, 16)
        assert _key(seed, 16) == (want & M32, want >> 32)
        assert psgd.rounding_stream_key(seed, 16) == _key(seed, 16)
        assert psgd.rounding_stream_key(seed, 16) != psgd.rounding_stream_key(seed, 0)


def test_the_torch_hash_is_the_python_restatement():
    idx = torch.tensor(INDICES, dtype=torch.int64)
    for seed in SEEDS:
        a, b = _key(seed, 16)
        got = psgd.param_rounding_addend(seed, idx).tolist()
        assert got == [_addend(a, b, i) for i in INDICES], seed
        assert all(0 <= u < 2 ** 16 for u in got)
    # the high half of the index enters: idx and idx + 2^32 draw differently somewhere
    lo = psgd.param_rounding_addend(5, torch.arange(64))
    hi = psgd.param_rounding_addend(5, torch.arange(64) + 2 ** 32)
    assert not torch.equal(lo, hi)


def test_the_torch_narrowing_is_the_python_restatement():
    """(bits + u) >> 16 with the rules for NaN, Inf and exact values; index0 >= 2^32"""
    xs = [1.0, -1.0, 1.0 + 2.0 ** -12, -(1.0 + 2.0 ** -9), 3.0e-39, -1e-45, 0.0, -0.0, float("inf"), -float("inf"), float("nan"),
          3.3895313892515355e38, 3.4028234663852886e38, -3.4028234663852886e38, 0.3337, 1234.5678]
    x = torch.tensor(xs, dtype=torch.float32)
    for seed in SEEDS[:3]:
        for index0 in (0, 17, 2 ** 32 - 3, 2 ** 33 + 1):
            got = psgd.stochastic_narrow_bf16(x, seed, index0).view(torch.int16).to(torch.int32) & 0xFFFF
            a, b = _key(seed, 16)
            want = []
            for j, v in enumerate(x.tolist()):
                bits = _bits(v)
                want.append(0x7FC0 if v != v else ((bits + _addend(a, b, index0 + j)) >> 16) & 0xFFFF)
            assert got.tolist() == want, (seed, index0)
    y = psgd.stochastic_narrow_bf16(x, 3, 0).float()
    assert y[0] == 1.0 and y[1] == -1.0 and y[8] == float("inf") and y[9] == -float("inf") and y[10] != y[10]
    assert _bits(float(y[6])) == 0 and _bits(float(y[7])) == 0x80000000                   # +-0 keep their sign
    assert float(y[11]) == 3.3895313892515355e38                                          # the largest finite bf16 value: exact
    with pytest.raises(TypeError, match="float32"):
        psgd.stochastic_narrow_bf16(x.double(), 3)


def test_the_torch_update_is_formed_once_and_narrowed_once():
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(5, 7, generator=g).to(torch.bfloat16)
    gr, v = torch.randn(5, 7, generator=g), (torch.randn(5, 7, generator=g) * 2.0 ** -6).to(torch.bfloat16)
    lr, c = 0.0123000003397464752197265625, 1.2300000526010990142822265625e-4          # float32 values
    p = p0.clone()
    psgd.param_update_stochastic_(p, gr.reshape(-1), v, lr, c, 11, 2 ** 32 + 5)
    w = p0.float()
    x = w - ((gr * lr + v.float()) + w * c)
    assert torch.equal(p.view(torch.int16), psgd.stochastic_narrow_bf16(x, 11, 2 ** 32 + 5).view(torch.int16))
    lo = x.view(torch.int32) & -65536                                                    # the neighbour towards zero
    hi = lo + 65536
    pb = p.float().view(torch.int32)
    assert bool(((pb == lo) | (pb == hi)).all())


# ------------------------------------------------------------------------------------------------------------- constructors
def _param(*shape, **kw):
    return torch.zeros(*shape, requires_grad=True, **kw)


@pytest.mark.parametrize("cls", ["UVd", "Kron"])
def test_constructor_errors_come_before_any_device_call(cls, monkeypatch):
    """CPU parameters get this far, and nothing is loaded or launched on the way"""
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    make = psgd.UVd if cls == "UVd" else ko.Kron
    for dt in (torch.float32, torch.float16):
        with pytest.raises(ValueError, match="param_rounding='stochastic' needs bfloat16 parameters"):
            make([_param(3, 4, dtype=dt)], param_rounding="stochastic")
    for dt in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError, match="param_rounding must be 'nearest' or 'stochastic'"):
            make([_param(3, 4, dtype=dt)], param_rounding="random")
    with pytest.raises(TypeError):                                                        # keyword-only
        if cls == "UVd":
            psgd.UVd([_param(3, 4)], 10, 1.0, 0.01, 0.01, None, 1.0, True, None, None, None, None, "auto", "widen", None, "torch",
                     0.0, 0.0, "propagate", None, 2000, "nearest")
        else:
            ko.Kron([_param(3, 4)], "dense", 1.0, 0.01, 0.01, None, 1.0, True, "nearest")


def test_kron_with_valid_arguments_reaches_the_device_check():
    for kw in (dict(param_rounding="nearest"), dict(param_rounding="stochastic", param_rounding_seed=5)):
        with pytest.raises(ValueError, match="one HIP device"):
            ko.Kron([_param(3, 4, dtype=torch.bfloat16)], **kw)


def test_wrappers_judge_the_rounding_arguments_first():
    t = torch.zeros(3, 4, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="rounding must be 'nearest' or 'stochastic'"):
        ko.multi_param_update([t], [t.float()], rounding="random")
    with pytest.raises(ValueError, match="apply to rounding='stochastic' only"):
        ko.multi_param_update([t], [t.float()], rounding_seed=3)
    with pytest.raises(ValueError, match="apply to rounding='stochastic' only"):
        ko.multi_param_update([t], [t.float()], index0=8)
    with pytest.raises(ValueError, match="needs grads"):
        ko.multi_param_update([t], None, [t], rounding="stochastic", rounding_seed=3)
    with pytest.raises(ValueError, match="index0 >= 0"):
        ko.multi_param_update([t], [t.float()], rounding="stochastic", rounding_seed=3, index0=-1)
    with pytest.raises(ValueError, match="rounding must be 'nearest' or 'stochastic'"):
        psgd.uvd_step_tail([t], t.float().reshape(-1), 0.1, rounding="random")
    with pytest.raises(ValueError, match="apply to rounding='stochastic' only"):
        psgd.uvd_step_tail([t], t.float().reshape(-1), 0.1, rounding_seed=3)
    with pytest.raises(ValueError, match="needs pre_grad"):
        psgd.uvd_step_tail([t], None, 0.1, vs=[t], rounding="stochastic", rounding_seed=3)


# -------------------------------------------------------------------------------------------------------------- checkpoint
def test_the_checkpoint_rules():
    enc, dec = psgd._param_rounding_encode, psgd._param_rounding_decode
    assert enc({"format": 1}, False, None, 0) == {"format": 1}                           # off: the keys of before
    sd = enc({"format": 1}, True, 2 ** 61 + 3, 9)
    assert sd == {"format": 1, "param_round_seed0": 2 ** 61 + 3, "param_round_step": 9}
    assert dec("x", sd, True, 77) == (2 ** 61 + 3, 9)                                    # restored
    assert dec("x", {"format": 1}, True, 77) == (77, 0)                                  # without them: own seed, counter 0
    assert dec("x", sd, False, None) == (None, 0)                                        # a nearest optimizer ignores them
    with pytest.raises(ValueError, match="param_round_step"):
        dec("x", {"param_round_seed0": 1}, True, 77)


def _uvd(**kw):
    gen = torch.Generator().manual_seed(4)
    ps = [_param(64, 2, dtype=torch.bfloat16), _param(64, dtype=torch.bfloat16)]
    return psgd.UVd(ps, rank_of_modification=2, generator=gen, placement=None, **kw)


def test_uvd_state_dict_keys_and_load_rules():
    near, sr = _uvd(), _uvd(param_rounding="stochastic")
    assert "param_round_seed0" not in near.state_dict() and "param_round_step" not in near.state_dict()
    assert set(sr.state_dict()) == set(near.state_dict()) | {"param_round_seed0", "param_round_step"}
    assert sr.state_dict()["param_round_step"] == 0 and 0 <= sr.state_dict()["param_round_seed0"] < 2 ** 62
    assert _uvd(param_rounding="stochastic").state_dict()["param_round_seed0"] == sr.state_dict()["param_round_seed0"]   # from generator=
    assert _uvd(param_rounding="stochastic", param_rounding_seed=12345).state_dict()["param_round_seed0"] == 12345
    explicit = _uvd(param_rounding="nearest").state_dict()
    assert set(explicit) == set(near.state_dict())
    sd = sr.state_dict()
    sd["param_round_seed0"], sd["param_round_step"] = 99, 7
    other = _uvd(param_rounding="stochastic", param_rounding_seed=5)
    other.load_state_dict(sd)
    assert (other._param_round_seed0, other._param_round_step) == (99, 7)
    other._param_round_step = 3
    other.load_state_dict(near.state_dict())                                             # no keys: own seed, counter 0
    assert (other._param_round_seed0, other._param_round_step) == (99, 0)
    near.load_state_dict(sd)                                                             # ignored
    assert "param_round_seed0" not in near.state_dict()
    import io
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    assert torch.load(buf, weights_only=True)["param_round_seed0"] == 99


def test_reshard_carries_the_keys_through():
    sr = _uvd(param_rounding="stochastic", param_rounding_seed=31)
    sr._param_round_step = 4
    sd = sr.state_dict()
    parts = sharded.reshard_uvd_state([sd], [64, 128])
    assert [(q["param_round_seed0"], q["param_round_step"]) for q in parts] == [(31, 4), (31, 4)]
    back = sharded.reshard_uvd_state(parts, [192])
    assert (back[0]["param_round_seed0"], back[0]["param_round_step"]) == (31, 4)
    parts[1]["param_round_step"] = 5
    with pytest.raises(ValueError, match="param_round_step"):
        sharded.reshard_uvd_state(parts, [192])
