"""The counter-based probe vectors of class Kron(preconditioner_fit="whitening"), the part that needs no GPU: the C ABI of
psgd_multi_randn_f32 (header = export = ctypes table, argument checks that return before any HIP call), the float64 restatement
counter_randn (indexing, seeds, pinned values, moments of one fixed stream), constructor validation and the checkpoint keys."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from psgd_tf_amd import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib
from psgd_tf_amd import kron_optimizer as ko
from tests.multi_randn_cases import MOMENT_N, MOMENT_SEED, moment_figures

NAME = "psgd_multi_randn_f32"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------- C ABI
def test_export_is_bound_and_the_version_did_not_move(lib):
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.SIGNATURES
    assert lib.psgd_abi_version() == 7 == _lib.PSGD_ABI_VERSION
    assert psgd.multi_randn is ko.multi_randn and callable(psgd.counter_randn)


def test_signature_matches_the_header_and_the_stream_is_documented():
    text = open(HEADER).read()
    kinds = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64}
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is ctypes.c_int
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(argtypes)
    for p, t in zip(params, argtypes):
        assert t is (ctypes.c_void_p if "*" in p else kinds[p.split()[0]]), p
    assert re.search(r"%s.*still 7" % NAME, text, re.S)
    ids = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "bf16_state.h")).read().split("#pragma once")[0]
    assert "17" in ids and "PROBE" in ids


def test_argument_checks(lib):
    """k >= 1, index0 >= 0, a finite scale, no null table: an error code with no device present"""
    BAD, OK = _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_OK
    segs, chunks = 0x10000, 0x20000                     # never dereferenced: the checks fail first
    call = lambda segs=segs, k=3, chunks=chunks, nchunks=5, seed=1, index0=0, scale=1.0: \
        lib.psgd_multi_randn_f32(segs, k, chunks, nchunks, seed, index0, scale, None)
    assert call(k=0) == BAD and call(k=-1) == BAD
    assert call(index0=-1) == BAD
    assert call(scale=float("inf")) == BAD and call(scale=-float("inf")) == BAD and call(scale=float("nan")) == BAD
    assert call(segs=None) == BAD and call(chunks=None) == BAD
    assert call(nchunks=-1) == BAD
    assert call(nchunks=0) == OK                        # nothing to do: no launch, so no device is needed either


# ----------------------------------------------------------------------------------------------------------- counter_randn
def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("index0", [0, 1, 2 ** 32 + 6, 2 ** 33 + 1])
def test_counter_randn_is_a_function_of_the_global_index(index0):
    seed = psgd.uvd_step_rounding_seed(99, 3)
    whole = psgd.counter_randn(seed, index0, 70)
    assert whole.dtype == np.float32 and whole.shape == (70,)
    for a, b in [(0, 70), (1, 2), (1, 70), (2, 69), (7, 8), (13, 40), (64, 64), (69, 70)]:       # odd and even a, empty, one element
        assert np.array_equal(_bits(whole[a:b]), _bits(psgd.counter_randn(seed, index0 + a, b - a))), (index0, a, b)


def test_counter_randn_scale_and_errors():
    seed = 12345
    z = psgd.counter_randn(seed, 5, 33)
    assert np.array_equal(_bits(psgd.counter_randn(seed, 5, 33, 2.0 ** -12)), _bits(z * np.float32(2.0 ** -12)))
    assert np.array_equal(_bits(psgd.counter_randn(seed, 5, 33, 3.0)), _bits(np.float32(3.0) * z))
    with pytest.raises(ValueError):
        psgd.counter_randn(seed, -1, 4)
    with pytest.raises(ValueError):
        psgd.counter_randn(seed, 0, 4, float("inf"))


def test_counter_randn_seeds_tensor_id_and_known_values():
    s0, s1 = psgd.uvd_step_rounding_seed(2026, 0), psgd.uvd_step_rounding_seed(2026, 1)
    a, b = psgd.counter_randn(s0, 0, 256), psgd.counter_randn(s1, 0, 256)
    assert s0 != s1 and not np.any(_bits(a) == _bits(b))
    assert psgd.rounding_stream_key(s0, 17) != psgd.rounding_stream_key(s0, 16)         # the probe is not the parameters' stream
    assert psgd._PROBE_TENSOR_ID == 17 and psgd._PARAM_TENSOR_ID == 16
    # computed once from the restatement itself: what pins the stream definition (key, pair, parity, u1 / theta) against drift
    assert s0 == 15966651630623008361
    assert psgd.rounding_stream_key(s0, 17) == (3824243591, 1922111058)
    assert [int(v) for v in _bits(a[:6])] == [0x3f5b5ad6, 0xbeadd9a8, 0xbdb095c6, 0x3db43baa, 0x3fb62bac, 0x3f5ab850]
    assert [int(v) for v in _bits(psgd.counter_randn(s0, 2 ** 33 + 1, 5))] == [0xbef6cc4e, 0x3f510588, 0xbf0f51c8, 0xbd91560a,
                                                                               0x3e9d24e9]


def test_counter_randn_extreme_hash_words_are_finite(monkeypatch):
    """u1 = 2^-32 (the largest radius, 6.66) and u1 = 1 (radius 0) both give finite values"""
    for h in (0x00000000_40000000, 0xFFFFFFFF_40000000):
        monkeypatch.setattr(psgd, "_mix64", lambda z, h=h: z * 0 + h)
        z = psgd.counter_randn(1, 0, 4)
        assert np.all(np.isfinite(z)) and np.abs(z).max() <= 6.67
    monkeypatch.undo()


def test_moments_of_the_fixed_stream():
    z = psgd.counter_randn(MOMENT_SEED, 0, MOMENT_N)
    assert np.all(np.isfinite(z))
    for name, (value, bound) in moment_figures(z).items():
        print("%-17s %.3e (bound %.3e)" % (name, value, bound))
        assert value <= bound, name


# -------------------------------------------------------------------------------------------------- constructor, checkpoint
def test_a_bad_preconditioner_fit_is_refused_before_any_device_error():
    p = torch.zeros(3, 4, requires_grad=True)                        # a CPU tensor: the device check would refuse it later
    for bad in ("whiten", "Hessian", None, 1):
        with pytest.raises(ValueError, match="preconditioner_fit"):
            ko.Kron([p], preconditioner_fit=bad)
    for good in ("hessian", "whitening"):                           # ... and the good ones get as far as the device check
        with pytest.raises(ValueError, match="HIP device"):
            ko.Kron([p], preconditioner_fit=good)


def test_state_dict_keys_of_the_probe_stream():
    sd = ko._probe_encode({}, True, 2 ** 63 + 5, 7)
    assert sd == {"probe_seed0": 2 ** 63 + 5, "probe_step": 7}
    assert ko._probe_encode({}, False, None, 0) == {}               # a hessian-fit optimizer adds nothing
    assert ko._probe_decode(sd, True, 11) == (2 ** 63 + 5, 7)       # restored
    assert ko._probe_decode({}, True, 11) == (11, 0)                # a dict without the keys: this object's seed, counter 0
    assert ko._probe_decode(sd, False, None) == (None, 0)           # a hessian-fit optimizer ignores the keys
    with pytest.raises(ValueError, match="probe_step"):
        ko._probe_decode({"probe_seed0": 1}, True, 11)
