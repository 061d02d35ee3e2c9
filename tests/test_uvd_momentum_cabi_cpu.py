"""The C ABI of momentum and decoupled weight decay in the UVd step tail (psgd_uvd_pack_blend_f32, psgd_uvd_param_update_multi_wd):
exported with the header's signatures, ABI still 7, argument checks that return before any HIP call; and what class UVd and
sharded.reshard_uvd_state decide on the host.  The arithmetic is checked on the GPU in test_uvd_momentum_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from psgd_tf_amd import _lib, sharded

NAMES = ("psgd_uvd_pack_blend_f32", "psgd_uvd_param_update_multi_wd")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_hip.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def test_exports_are_bound_and_the_abi_did_not_move(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.psgd_abi_version() == _lib.PSGD_ABI_VERSION == 7


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
    # the new entry points take the old ones' arguments plus their own, in the places the header documents
    old_pack, new_pack = _lib.SIGNATURES["psgd_uvd_pack_f32"][1], _lib.SIGNATURES["psgd_uvd_pack_blend_f32"][1]
    assert new_pack == old_pack[:6] + [ctypes.c_float, ctypes.c_float] + old_pack[6:]
    old_upd, new_upd = _lib.SIGNATURES["psgd_uvd_param_update_multi"][1], _lib.SIGNATURES["psgd_uvd_param_update_multi_wd"][1]
    assert new_upd == old_upd[:-1] + [ctypes.c_float] + old_upd[-1:]


def test_argument_checks(lib):
    """the checks of psgd_uvd_pack_f32 / psgd_uvd_param_update_multi, and weight decay on the perturbation: PSGD_ERR_BAD_ARG (-1)
    with no device present"""
    BAD = _lib.PSGD_ERR_BAD_ARG
    segs, vsegs, chunks, out, pre, sq = (0x10000 * k for k in range(1, 7))            # never dereferenced: the checks fail first
    blend, upd = lib.psgd_uvd_pack_blend_f32, lib.psgd_uvd_param_update_multi_wd
    for beta, omb in ((0.0, 1.0), (0.9, 0.1)):
        assert blend(None, 3, chunks, 5, 0, 1.0, beta, omb, out, None) == BAD
        assert blend(segs, 3, None, 5, 0, 1.0, beta, omb, out, None) == BAD
        assert blend(segs, 3, chunks, 5, 0, 1.0, beta, omb, None, None) == BAD
        assert blend(segs, -1, chunks, 5, 0, 1.0, beta, omb, out, None) == BAD
        assert blend(segs, 3, chunks, -5, 0, 1.0, beta, omb, out, None) == BAD
        assert blend(segs, 3, chunks, 5, 3, 1.0, beta, omb, out, None) == BAD
        assert blend(segs, 3, chunks, 5, -1, 1.0, beta, omb, out, None) == BAD
        assert blend(segs, 3, chunks, 0, 1, 1.0, beta, omb, out, None) == _lib.PSGD_OK  # no chunk: nothing to launch
    for wd in (0.0, 0.01):
        tail = (0.1, None, 0.0, 1e-38, wd, None)
        assert upd(None, None, 3, chunks, 5, 0, pre, *tail) == BAD
        assert upd(segs, None, 3, None, 5, 0, pre, *tail) == BAD
        assert upd(segs, None, -3, chunks, 5, 0, pre, *tail) == BAD
        assert upd(segs, None, 3, chunks, -1, 0, pre, *tail) == BAD
        assert upd(segs, None, 3, chunks, 5, 7, pre, *tail) == BAD
        assert upd(segs, None, 3, chunks, 5, 0, None, *tail) == BAD                   # neither a gradient nor vs
        assert upd(segs, vsegs, 3, chunks, 5, 0, None, 0.1, sq, 1.0, 1e-38, wd, None) == BAD   # a clip norm without a gradient
        assert upd(segs, vsegs, 3, chunks, 0, 2, pre, *tail) == _lib.PSGD_OK
    assert upd(segs, vsegs, 3, chunks, 5, 0, None, 0.0, None, 0.0, 1e-38, 0.01, None) == BAD   # the perturbation decays nothing
    assert upd(segs, vsegs, 3, chunks, 0, 0, None, 0.0, None, 0.0, 1e-38, 0.0, None) == _lib.PSGD_OK


def test_momentum_coefficients_are_float32_and_warm_up():
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import uvd_momentum_coefficients
    assert uvd_momentum_coefficients(0, 0.9) == (0.0, 1.0)
    for k, mom in ((1, 0.9), (3, 0.9), (8, 0.9), (9, 0.9), (100, 0.9), (5, 0.0), (7, 0.999)):
        beta, omb = uvd_momentum_coefficients(k, mom)
        want = np.float32(min(k / (k + 1.0), mom))
        assert beta == float(want) and np.float32(beta) == want
        assert omb == float(np.float32(1.0) - want) and float(np.float32(omb)) == omb
    assert uvd_momentum_coefficients(8, 0.9)[0] == float(np.float32(8.0 / 9.0))          # still warming up
    assert uvd_momentum_coefficients(9, 0.9)[0] == float(np.float32(0.9))                # 9 / 10 = momentum


def test_class_arguments_are_checked_before_anything_runs():
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import UVd, _Hyper
    p = [torch.zeros(3, requires_grad=True)]
    for bad in (dict(momentum=1.0), dict(momentum=-0.1), dict(weight_decay=-1e-3), dict(momentum=float("nan"))):
        with pytest.raises(ValueError, match="momentum|weight_decay"):
            UVd(p, rank_of_modification=2, placement=None, **bad)
    opt = UVd(p, rank_of_modification=2, placement=None, momentum=0.5, weight_decay=0.01)
    assert isinstance(opt.momentum, _Hyper) and isinstance(opt.weight_decay, _Hyper)
    assert float(opt.momentum.assign(0.25)) == 0.25 and float(opt.weight_decay.assign(0.0)) == 0.0
    off = UVd(p, rank_of_modification=2, placement=None)
    assert float(off.momentum) == 0.0 and float(off.weight_decay) == 0.0 and off._m is None
    assert "momentum_buffer" not in off.state_dict() and off.state_dict()["hyper"]["momentum"] == 0.0


# ------------------------------------------------------------------------------------------------ reshard
R = 3


def _checkpoint(cuts, with_buffer=True):
    total = cuts[-1]
    g = torch.Generator().manual_seed(7)
    U, V = torch.randn(total, R, generator=g), torch.randn(total, R, generator=g)
    d, m = torch.rand(total, 1, generator=g).add(0.5), torch.randn(total, generator=g)
    rng = torch.Generator().manual_seed(9).get_state()
    sds = []
    for lo, hi in zip(cuts, cuts[1:]):
        sd = {"format": 1, "U": U[lo:hi].clone(), "V": V[lo:hi].clone(), "d": d[lo:hi].clone(), "rank": R,
              "num_params": hi - lo, "num_params_global": total, "row0": lo, "param_sizes": [hi - lo],
              "state_dtype": "torch.float32", "state_route": "widen", "state_rounding": "none",
              "hyper": {"lr_params": 0.01, "lr_preconditioner": 0.02, "grad_clip_max_norm": float("inf"),
                        "preconditioner_update_probability": 0.5, "exact_hessian_vector_product": True,
                        "momentum": 0.9, "weight_decay": 0.01},
              "branch_rng": rng.clone()}
        if with_buffer:
            sd["momentum_buffer"], sd["momentum_step"] = m[lo:hi].clone(), 4
        sds.append(sd)
    return sds, m


def test_reshard_carries_the_momentum_rows_2_3_1():
    sds, m = _checkpoint((0, 192, 357))
    three = sharded.reshard_uvd_state([sds[1], sds[0]], [128, 192, 37])
    assert [s["momentum_buffer"].numel() for s in three] == [128, 192, 37]
    assert torch.equal(torch.cat([s["momentum_buffer"] for s in three]), m)
    assert all(s["momentum_step"] == 4 and s["hyper"]["momentum"] == 0.9 for s in three)
    assert all(s["momentum_buffer"].dtype == torch.float32 and s["momentum_buffer"].is_contiguous() for s in three)
    one = sharded.reshard_uvd_state(three, [357])
    assert torch.equal(one[0]["momentum_buffer"], m) and one[0]["momentum_step"] == 4
    three[0]["momentum_buffer"][0] = 7.0                                  # clones, not views of one another
    assert one[0]["momentum_buffer"][0] == m[0]


def test_reshard_without_a_buffer_everywhere_drops_it_and_disagreement_is_named():
    sds, _ = _checkpoint((0, 192, 357))
    del sds[1]["momentum_buffer"]
    sds[1].pop("momentum_step")
    sds[0].pop("momentum_step")
    out = sharded.reshard_uvd_state(sds, [357])
    assert "momentum_buffer" not in out[0] and "momentum_step" not in out[0]
    old, _ = _checkpoint((0, 192, 357), with_buffer=False)
    for s in old:
        del s["hyper"]["momentum"], s["hyper"]["weight_decay"]            # a checkpoint from before the arguments
    out = sharded.reshard_uvd_state(old, [64, 293])
    assert all("momentum_buffer" not in s for s in out)
    sds, _ = _checkpoint((0, 192, 357))
    sds[1]["momentum_step"] = 5
    with pytest.raises(ValueError, match="momentum_step"):
        sharded.reshard_uvd_state(sds, [357])
    sds, _ = _checkpoint((0, 192, 357))
    sds[0]["momentum_buffer"] = sds[0]["momentum_buffer"][:-1]
    with pytest.raises(ValueError, match="momentum_buffer"):
        sharded.reshard_uvd_state(sds, [357])
