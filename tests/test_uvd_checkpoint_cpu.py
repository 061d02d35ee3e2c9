"""UVd checkpoints without a GPU: the narrowing entry point is exported (ABI still 7) and its argument checks return before any
HIP call; sharded.reshard_uvd_state on hand-built state dicts."""
import copy
import ctypes

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, sharded


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build_extension()
    return _lib.load()


def test_library_exports_the_narrowing_kernel(lib):
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "psgd_uvd_bf16_narrow_f32")
    assert "psgd_uvd_bf16_narrow_f32" in _lib.SIGNATURES
    assert lib.psgd_abi_version() == _lib.PSGD_ABI_VERSION == 7


def test_narrowing_argument_checks(lib):
    f = lib.psgd_uvd_bf16_narrow_f32
    src, dst = 0x1000, 0x2000                        # never dereferenced: every call below returns from its checks
    assert f(None, dst, 8, 0, 0, 0, 1, None) == _lib.PSGD_ERR_BAD_ARG
    assert f(src, None, 8, 0, 0, 0, 1, None) == _lib.PSGD_ERR_BAD_ARG
    assert f(src, dst, -1, 0, 0, 0, 1, None) == _lib.PSGD_ERR_BAD_ARG
    assert f(src, dst, 8, -1, 0, 0, 1, None) == _lib.PSGD_ERR_BAD_ARG
    for tensor in (-1, 3):
        assert f(src, dst, 8, 0, tensor, 0, 1, None) == _lib.PSGD_ERR_BAD_ARG
    for rounding in (-1, 2):
        assert f(src, dst, 8, 0, 0, rounding, 1, None) == _lib.PSGD_ERR_BAD_ARG
    assert f(src + 2, dst, 8, 0, 0, 0, 1, None) == _lib.PSGD_ERR_ALIGN
    assert f(src, dst + 1, 8, 0, 0, 0, 1, None) == _lib.PSGD_ERR_ALIGN
    assert f(src, dst, 0, 0, 2, 1, 1, None) == _lib.PSGD_OK               # count = 0: a no-op


# ------------------------------------------------------------------------------------------------ reshard
R = 3
CUTS3 = (0, 128, 320, 357)                          # three ranks; the last one holds 37 rows


def _checkpoint(cuts=CUTS3, dtype=torch.bfloat16):
    total = cuts[-1]
    g = torch.Generator().manual_seed(7)
    U = torch.randn(total, R, generator=g).to(dtype)
    V = torch.randn(total, R, generator=g).to(dtype)
    d = torch.rand(total, 1, generator=g).add(0.5).to(dtype)
    rng = torch.Generator().manual_seed(9).get_state()
    sds = []
    for lo, hi in zip(cuts, cuts[1:]):
        sds.append({"format": 1, "U": U[lo:hi].clone(), "V": V[lo:hi].clone(), "d": d[lo:hi].clone(), "rank": R,
                    "num_params": hi - lo, "num_params_global": total, "row0": lo, "param_sizes": [hi - lo],
                    "state_dtype": str(dtype), "state_route": "native", "state_rounding": "stochastic",
                    "round_seed0": 2 ** 61 + 12345, "round_step": 17,
                    "hyper": {"lr_params": 0.01, "lr_preconditioner": 0.02, "grad_clip_max_norm": float("inf"),
                              "preconditioner_update_probability": 0.5, "exact_hessian_vector_product": True},
                    "branch_rng": rng.clone()})
    return sds, (U, V, d)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def test_reshard_3_2_3_reproduces_the_rows():
    sds, (U, V, d) = _checkpoint()
    two = sharded.reshard_uvd_state([sds[2], sds[0], sds[1]], [192, 165])          # any order in
    assert [s["row0"] for s in two] == [0, 192] and [s["num_params"] for s in two] == [192, 165]
    assert all(s["param_sizes"] is None and s["num_params_global"] == 357 for s in two)
    for k, whole in (("U", U), ("V", V), ("d", d)):
        assert torch.equal(_bits(torch.cat([s[k] for s in two], 0)), _bits(whole))
    three = sharded.reshard_uvd_state(two, [128, 192, 37])                          # a last entry of 37 is accepted
    for a, b in zip(three, sds):
        for k in ("U", "V", "d"):
            assert a[k].dtype == b[k].dtype and torch.equal(_bits(a[k]), _bits(b[k])), k
        assert torch.equal(a["branch_rng"], b["branch_rng"])
        for k in ("format", "rank", "num_params", "num_params_global", "row0", "state_dtype", "state_route", "state_rounding",
                  "round_seed0", "round_step", "hyper"):
            assert a[k] == b[k], k
    three[0]["U"].zero_()                                                            # outputs own their memory
    assert torch.equal(_bits(two[0]["U"]), _bits(U[:192]))


def test_reshard_one_to_many_and_back():
    sds, (U, _, _) = _checkpoint(cuts=(0, 357), dtype=torch.float32)
    many = sharded.reshard_uvd_state(sds, [64, 64, 64, 64, 101])
    assert [s["row0"] for s in many] == [0, 64, 128, 192, 256]
    back = sharded.reshard_uvd_state(many, [357])
    assert torch.equal(back[0]["U"], U) and back[0]["row0"] == 0 and back[0]["num_params"] == 357


def test_reshard_errors_name_what_is_wrong():
    sds, _ = _checkpoint()
    gap = copy.deepcopy(sds)
    gap[1]["row0"] += 64
    with pytest.raises(ValueError, match="row0.*gap"):
        sharded.reshard_uvd_state(gap, [192, 165])
    overlap = copy.deepcopy(sds)
    overlap[2]["row0"] -= 64
    with pytest.raises(ValueError, match="row0.*overlap"):
        sharded.reshard_uvd_state(overlap, [192, 165])
    with pytest.raises(ValueError, match="num_params_global"):
        sharded.reshard_uvd_state(sds[:2], [192, 165])                               # the last rank is missing
    seed = copy.deepcopy(sds)
    seed[1]["round_seed0"] += 1
    with pytest.raises(ValueError, match="round_seed0"):
        sharded.reshard_uvd_state(seed, [192, 165])
    hyper = copy.deepcopy(sds)
    hyper[2]["hyper"]["lr_params"] = 0.5
    with pytest.raises(ValueError, match="hyper"):
        sharded.reshard_uvd_state(hyper, [192, 165])
    rng = copy.deepcopy(sds)
    rng[0]["branch_rng"][0] ^= 1
    with pytest.raises(ValueError, match="branch_rng"):
        sharded.reshard_uvd_state(rng, [192, 165])
    dt = copy.deepcopy(sds)
    dt[1]["V"] = dt[1]["V"].float()
    with pytest.raises(ValueError, match="dtype"):
        sharded.reshard_uvd_state(dt, [192, 165])
    with pytest.raises(ValueError, match="multiple of 64"):
        sharded.reshard_uvd_state(sds, [100, 257])                                   # 100: not a multiple of 64, not last
    with pytest.raises(ValueError, match="sum"):
        sharded.reshard_uvd_state(sds, [192, 64])
    fmt = copy.deepcopy(sds)
    for s in fmt:
        s["format"] = 2
    with pytest.raises(ValueError, match="format"):
        sharded.reshard_uvd_state(fmt, [192, 165])


def test_state_dict_values_survive_weights_only_loading():
    """what state_dict() holds besides tensors -- a seed of 62 bits, an infinite clip norm, None -- through torch.save /
    torch.load(weights_only=True)"""
    import io
    sds, _ = _checkpoint()
    sd = sharded.reshard_uvd_state(sds, [357])[0]
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    got = torch.load(buf, weights_only=True)
    assert got["round_seed0"] == 2 ** 61 + 12345 and isinstance(got["round_seed0"], int)
    assert got["hyper"] == sd["hyper"] and got["param_sizes"] is None
    assert got["U"].dtype == torch.bfloat16 and torch.equal(_bits(got["U"]), _bits(sd["U"]))
    assert got["branch_rng"].dtype == torch.uint8 and torch.equal(got["branch_rng"], sd["branch_rng"])


# ------------------------------------------------------------------------------- class UVd: judge first, then commit or draw
SHAPES = [(5, 7), (4, 3), (7,)]
FEATURES = dict(momentum=0.9, nonfinite="skip", loss_scale=2 ** 4, preconditioner_fit="whitening")


def _class_params(dtype=torch.float32):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(s, generator=g).to(dtype).requires_grad_(True) for s in SHAPES]


def _raw(t):
    return t.detach().reshape(-1).view(torch.uint8).clone()


def _uvd_pair(dtype=torch.float32, **kw):
    """an optimizer and the state dict of a differently-seeded twin that differs from it in every value a load restores"""
    g = torch.Generator().manual_seed(3)
    opt = psgd.UVd(_class_params(dtype), 3, generator=g, **dict(FEATURES, **kw))
    opt._momentum_buffer().copy_(torch.arange(54.0))
    opt._m_step, opt._probe_step = 3, 2
    twin = psgd.UVd(_class_params(dtype), 3, generator=torch.Generator().manual_seed(9), lr_params=0.5,
                    **dict(FEATURES, momentum=0.8, loss_scale=2 ** 6, **kw))
    twin._momentum_buffer().copy_(torch.arange(54.0).flip(0))
    twin._m_step, twin._probe_step, twin._param_round_step = 5, 7, 11
    twin._U.mul_(2)
    return g, opt, twin.state_dict()


def _held(g, opt):
    return (_raw(g.get_state()), float(opt.lr_params), float(opt.momentum), float(opt.loss_scale), opt.probe_seed0, opt.probe_step,
            _raw(opt._m), opt._m_step, _raw(opt._U), opt._param_round_seed0, opt._param_round_step)


def _same(a, b):
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))


def test_a_refused_state_dict_leaves_the_optimizer_as_it_was():
    g, opt, sd = _uvd_pair()
    refused = [dict(sd, loss_scale=3.0), {k: v for k, v in sd.items() if k != "probe_step"},
               dict(sd, branch_rng=torch.zeros(3, dtype=torch.uint8)), dict(sd, momentum_buffer=torch.zeros(53))]
    gb, optb, sdb = _uvd_pair(torch.bfloat16, param_rounding="stochastic")
    cases = [(g, opt, bad) for bad in refused] + [(gb, optb, {k: v for k, v in sdb.items() if k != "param_round_step"})]
    for gen, o, bad in cases:
        before = _held(gen, o)
        with pytest.raises(ValueError):
            o.load_state_dict(bad)
        assert _same(_held(gen, o), before)
    for gen, o, good in ((g, opt, sd), (gb, optb, sdb)):
        before = _held(gen, o)
        o.load_state_dict(good)
        want = (_raw(good["branch_rng"]), good["hyper"]["lr_params"], good["hyper"]["momentum"], good["loss_scale"],
                good["probe_seed0"], good["probe_step"], _raw(good["momentum_buffer"]), good["momentum_step"], _raw(good["U"]),
                good.get("param_round_seed0"), good.get("param_round_step", 0))
        assert _same(_held(gen, o), want) and not any(_same([x], [y]) for x, y in zip(before[:9], want[:9]))


BAD_ARGUMENTS = [(dict(step_tail="x"), "step_tail"), (dict(placement="x"), "placement"), (dict(state_route="x"), "state_route"),
                 (dict(state_dtype=torch.bfloat16, state_route="native", state_rounding="up"), "state_rounding must be"),
                 (dict(state_rounding="nearest"), "state_rounding applies"), (dict(preconditioner_fit="x"), "preconditioner_fit"),
                 (dict(param_rounding="x"), "param_rounding"), (dict(momentum=1.0), "momentum"), (dict(nonfinite="x"), "nonfinite"),
                 (dict(loss_scale=2.0), "loss_scale needs"), (dict(nonfinite="skip", loss_scale=3.0), "loss_scale must be a power of two"),
                 (dict(nonfinite="skip", loss_scale="x"), "loss_scale must be None"),
                 (dict(loss_scale_growth_interval=0), "loss_scale_growth_interval"), (dict(rank_of_modification=0), "rank_of_modification")]


@pytest.mark.parametrize("bad, match", BAD_ARGUMENTS, ids=[m.split()[0] + str(i) for i, (_, m) in enumerate(BAD_ARGUMENTS)])
def test_a_bad_argument_is_refused_before_anything_is_drawn(bad, match):
    """each call would draw all three construction seeds if it were accepted (a native bfloat16 state, stochastic parameter
    rounding, the whitening fit): the generator behind them is left as it was"""
    g = torch.Generator().manual_seed(7)
    before = g.get_state().clone()
    kw = dict(rank_of_modification=3, generator=g, state_dtype=torch.bfloat16, state_route="native", param_rounding="stochastic",
              preconditioner_fit="whitening")
    if "state_rounding" in bad and "state_route" not in bad:
        kw.update(state_dtype=None, state_route="widen")
    with pytest.raises(ValueError, match="UVd: " + match):
        psgd.UVd(_class_params(torch.bfloat16), **dict(kw, **bad))
    assert torch.equal(g.get_state(), before)


def test_a_good_construction_draws_state_parameters_probe_in_this_order():
    g = torch.Generator().manual_seed(7)
    opt = psgd.UVd(_class_params(torch.bfloat16), 3, generator=g, state_dtype=torch.bfloat16, state_route="native",
                   param_rounding="stochastic", preconditioner_fit="whitening")
    twin = torch.Generator().manual_seed(7)
    want = [int(torch.randint(0, 2 ** 62, (), generator=twin).item()) for _ in range(3)]
    assert [opt._round_seed0, opt._param_round_seed0, opt.probe_seed0] == want and torch.equal(g.get_state(), twin.get_state())
