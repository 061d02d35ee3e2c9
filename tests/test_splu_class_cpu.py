"""class SPLU without a device: the constructor's checks in their order (each raises before a device is touched: the parameters
here are CPU tensors and nothing is launched), the defaults, the initial state of demo_usage_of_all_preconditioners.py:47-51, the
parameter index and the unchanged C ABI."""
import inspect
import math

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl

SHAPES = [(7, 5), (5,), (3, 4, 2), ()]                   # N = 65


def _params(dtype=torch.float32, shapes=SHAPES):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(s, generator=g).to(dtype).requires_grad_(True) for s in shapes]


def test_the_class_is_public_and_the_abi_did_not_move():
    from psgd_tf_amd import _lib, splu_optimizer
    assert psgd.SPLU is splu_optimizer.SPLU and issubclass(psgd.SPLU, impl._StepFeatures)
    assert _lib.PSGD_ABI_VERSION == 7
    assert _lib.load().psgd_abi_version() == 7


def test_signature_follows_class_uvd():
    """the same names in the same order (without the row-shard and placement arguments), so that a user swaps the class name; the
    defaults that differ are the demo's"""
    s, u = inspect.signature(psgd.SPLU.__init__).parameters, inspect.signature(psgd.UVd.__init__).parameters
    dropped = ("group", "stage_backend", "placement", "state_route")
    assert list(s) == [k for k in u if k not in dropped]
    for k in s:
        assert s[k].kind == u[k].kind
        if k not in ("preconditioner_init_scale", "lr_preconditioner"):
            assert s[k].default == u[k].default, k
    assert s["preconditioner_init_scale"].default == 0.1 and s["lr_preconditioner"].default == 0.1


def test_defaults():
    opt = psgd.SPLU(_params())
    assert float(opt.lr_params) == 0.01 and float(opt.lr_preconditioner) == 0.1
    assert math.isinf(float(opt.grad_clip_max_norm)) and float(opt.preconditioner_update_probability) == 1.0
    assert bool(opt.exact_hessian_vector_product) and float(opt.momentum) == 0.0 and float(opt.weight_decay) == 0.0
    assert all(isinstance(getattr(opt, k), impl._Hyper) for k in psgd.UVd._HYPER_KEYS + ("momentum", "weight_decay", "loss_scale"))
    assert opt.loss_scale.value is None and opt.skipped_steps == 0 and opt.preconditioner_fit == "hessian"
    assert opt.probe_seed0 is None and opt._tail is None and opt._in_place
    assert opt._L12.shape == (65, 10) and all(t.dtype == torch.float32 for t in opt.factors)
    assert opt._tiny == torch.finfo(torch.float32).tiny and opt._delta_param_scale == torch.finfo(torch.float32).eps ** 0.5


@pytest.mark.parametrize("r, dtype", [(4, torch.float32), (65, torch.float32), (4, torch.bfloat16)])
def test_initial_state(r, dtype):
    s = 0.25 if dtype == torch.float32 else 0.1
    opt = psgd.SPLU(_params(), r, s, state_dtype=dtype)
    L12, l3, U12, u3 = opt.factors
    assert L12.shape == (65, r) and l3.shape == (65 - r, 1) and U12.shape == (r, 65) and u3.shape == (65 - r, 1)
    assert all(t.dtype == dtype and t.is_contiguous() for t in opt.factors)
    sv = torch.tensor(s).to(dtype)                                                  # rounded once
    assert torch.equal(L12[:r], sv * torch.eye(r, dtype=dtype)) and not bool(L12[r:].any())
    assert torch.equal(U12[:, :r], sv * torch.eye(r, dtype=dtype)) and not bool(U12[:, r:].any())
    assert bool((l3 == sv).all()) and bool((u3 == sv).all())
    for k in ("v", "h", "g"):
        assert opt._flat_bufs[k].shape == (65,) and opt._flat_bufs[k].dtype == torch.float32
    assert opt._out.shape == (65,)


def test_rank_above_the_parameter_count_raises():
    with pytest.raises(ValueError, match="rank_of_modification"):
        psgd.SPLU(_params(), 66)
    with pytest.raises(ValueError, match="rank_of_modification"):
        psgd.SPLU(_params(), 0)


def test_parameter_index_is_uvd_param_index():
    frozen = torch.zeros(3)                                                         # requires_grad False: filtered out
    nested = {"b": [_params()[0], frozen], "a": (_params()[1], [_params()[2], _params()[3]])}
    opt = psgd.SPLU(nested, 4)
    flat = [p for p in impl._flatten_params(nested) if p.requires_grad]
    assert [tuple(p.shape) for p in opt._params] == [(5,), (3, 4, 2), (), (7, 5)]   # dict keys sorted, depth first
    assert (opt._param_sizes, opt._param_cumsizes) == psgd.uvd_param_index(flat) == ([5, 24, 1, 35], [5, 29, 30, 65])
    assert all(a is b for a, b in zip(opt._params, flat))


def test_constructor_checks_in_their_order():
    """every call below is wrong in the argument under test AND in every argument checked after it: the first check speaks"""
    bad_later = dict(rank_of_modification=0, state_rounding="up", momentum=2.0, step_tail="x")
    with pytest.raises(TypeError, match="parameters must be"):
        psgd.SPLU(_params(torch.float64), param_rounding="x", **bad_later)
    with pytest.raises(ValueError, match="param_rounding"):
        psgd.SPLU(_params(), param_rounding="x", preconditioner_fit="x", **bad_later)
    with pytest.raises(ValueError, match="param_rounding='stochastic' needs bfloat16"):
        psgd.SPLU(_params(), param_rounding="stochastic", preconditioner_fit="x", **bad_later)
    with pytest.raises(ValueError, match="preconditioner_fit"):
        psgd.SPLU(_params(), preconditioner_fit="x", state_dtype=torch.float16, **bad_later)
    with pytest.raises(TypeError, match="float16 state"):
        psgd.SPLU(_params(), state_dtype=torch.float16, **bad_later)
    with pytest.raises(TypeError, match="float16 state"):
        psgd.SPLU(_params(torch.float16), state_dtype="param", **bad_later)
    with pytest.raises(TypeError, match="state_dtype"):
        psgd.SPLU(_params(), state_dtype=torch.float64, **bad_later)
    with pytest.raises(ValueError, match="rank_of_modification must be >= 1"):
        psgd.SPLU(_params(), **bad_later)
    later = dict(bad_later, rank_of_modification=33)
    with pytest.raises(ValueError, match="bfloat16 state supports ranks up to 32"):
        psgd.SPLU(_params(), state_dtype=torch.bfloat16, **later)
    with pytest.raises(ValueError, match="bfloat16 state supports ranks up to 32"):
        psgd.SPLU(_params(torch.bfloat16), state_dtype="param", **later)
    with pytest.raises(ValueError, match="state_rounding must be"):
        psgd.SPLU(_params(), state_dtype=torch.bfloat16, **dict(bad_later, rank_of_modification=4))
    with pytest.raises(ValueError, match="state_rounding applies"):
        psgd.SPLU(_params(), **dict(bad_later, rank_of_modification=4))
    with pytest.raises(ValueError, match="momentum"):
        psgd.SPLU(_params(), 4, momentum=2.0, weight_decay=-1.0, step_tail="x")
    with pytest.raises(ValueError, match="weight_decay"):
        psgd.SPLU(_params(), 4, weight_decay=-1.0, nonfinite="x", step_tail="x")
    with pytest.raises(ValueError, match="nonfinite"):
        psgd.SPLU(_params(), 4, nonfinite="x", loss_scale=3.0, step_tail="x")
    with pytest.raises(ValueError, match="loss_scale needs"):
        psgd.SPLU(_params(), 4, loss_scale=2.0, step_tail="x")
    with pytest.raises(ValueError, match="power of two"):
        psgd.SPLU(_params(), 4, nonfinite="skip", loss_scale=3.0, step_tail="x")
    with pytest.raises(ValueError, match="step_tail"):
        psgd.SPLU(_params(), 4, step_tail="x")


def test_bad_arguments_draw_nothing_and_good_ones_draw_in_uvd_order():
    """a refused constructor leaves the generator alone; an accepted one draws the state's seed, the parameters', the probe's"""
    g = torch.Generator().manual_seed(7)
    before = g.get_state()
    with pytest.raises(ValueError):
        psgd.SPLU(_params(torch.bfloat16), 4, generator=g, state_dtype="param", param_rounding="stochastic",
                  preconditioner_fit="whitening", step_tail="x")
    assert torch.equal(g.get_state(), before)
    opt = psgd.SPLU(_params(torch.bfloat16), 4, generator=g, state_dtype="param", param_rounding="stochastic",
                    preconditioner_fit="whitening")
    g2 = torch.Generator().manual_seed(7)
    want = [int(torch.randint(0, 2 ** 62, (), generator=g2).item()) for _ in range(3)]
    assert [opt._round_seed0, opt._param_round_seed0, opt.probe_seed0] == want
    assert opt._state_rounding == "stochastic" and opt._bf16 and not opt._in_place
    assert psgd.SPLU(_params(), 4, probe_seed=2 ** 64 + 5, preconditioner_fit="whitening").probe_seed0 == 5


def test_routes_by_rank():
    shapes = [(10, 15)]
    assert psgd.SPLU(_params(shapes=shapes), 64)._in_place
    assert not psgd.SPLU(_params(shapes=shapes), 70)._in_place                      # column chunks: the functions' route


def test_step_on_the_cpu_is_an_error_not_a_fallback():
    from psgd_tf_amd._lib import PsgdHipError
    params = _params()
    opt = psgd.SPLU(params, 4)
    with pytest.raises(PsgdHipError, match="no CPU fallback"):
        opt.step(lambda: sum(torch.sum(p * p) for p in params))


def test_state_dict_keys_and_refusals():
    g = torch.Generator().manual_seed(3)
    opt = psgd.SPLU(_params(), 4, generator=g, momentum=0.9, nonfinite="skip", preconditioner_fit="whitening")
    sd = opt.state_dict()
    assert sd["preconditioner"] == "splu" and sd["format"] == 1 and sd["rank"] == 4 and sd["num_params"] == 65
    assert sd["L12"].dtype == torch.float32 and sd["L12"].data_ptr() != opt._L12.data_ptr()
    assert {"l3", "U12", "u3", "hyper", "branch_rng", "probe_seed0", "probe_step", "momentum_buffer", "momentum_step",
            "skipped_steps", "loss_scale"} <= set(sd)
    twin = psgd.SPLU(_params(), 4, generator=torch.Generator().manual_seed(99), momentum=0.9, nonfinite="skip",
                     preconditioner_fit="whitening")
    twin.lr_params.assign(0.5)
    twin.load_state_dict(sd)
    assert float(twin.lr_params) == 0.01 and twin.probe_seed0 == opt.probe_seed0
    assert torch.equal(twin._generator.get_state(), g.get_state())
    with pytest.raises(ValueError, match="'rank'"):
        psgd.SPLU(_params(), 5).load_state_dict(sd)
    with pytest.raises(ValueError, match="'preconditioner'"):
        twin.load_state_dict(dict(sd, preconditioner="uvd"))
    with pytest.raises(TypeError, match="cannot be loaded"):
        psgd.SPLU(_params(), 4, state_dtype=torch.bfloat16).load_state_dict(sd)       # fp32 -> bf16: out of scope
    wide = psgd.SPLU(_params(), 4)
    bf = psgd.SPLU(_params(), 4, state_dtype=torch.bfloat16).state_dict()
    wide.load_state_dict(bf)                                                           # bf16 -> fp32 widens exactly
    assert torch.equal(wide._l3, bf["l3"].float())


SHARED = ("step", "_pack_scale", "_flat", "_momentum_buffer", "_grad_flat", "_grad_cat", "_guarded_grad", "_whitening_inputs",
          "_draw_probe", "_step_grad")
# the members of a step that class Kron shares too: they live on _StepFeatures, and no class below it has a copy
STEP_LAYER = ("_HYPER_KEYS", "_init_step_hypers", "_step_route", "_closure_gradients", "_tail_coefficients", "_fused_tail_kwargs")
SUBCLASS_STATE = ("_arena", "_U", "_V", "_d", "_L12", "_l3", "_U12", "_u3", "_native", "_in_place", "_out")


def test_the_flat_step_is_one_copy_under_both_classes():
    """class UVd and class SPLU are subclasses of _FlatStep and override none of the shared members"""
    base = impl._FlatStep
    assert issubclass(psgd.UVd, base) and issubclass(psgd.SPLU, base) and issubclass(base, impl._StepFeatures)
    for f in SHARED:
        assert getattr(psgd.UVd, f) is getattr(psgd.SPLU, f) is getattr(base, f), f
        assert f not in vars(psgd.UVd) and f not in vars(psgd.SPLU), f
    for f in STEP_LAYER:
        assert getattr(psgd.UVd, f) is getattr(psgd.SPLU, f) is getattr(impl._StepFeatures, f), f
        assert f not in vars(psgd.UVd) and f not in vars(psgd.SPLU) and f not in vars(base), f
    assert psgd.UVd._HYPER_KEYS is psgd.SPLU._HYPER_KEYS is base._HYPER_KEYS


FEATURES = dict(momentum=0.9, nonfinite="skip", loss_scale="dynamic", preconditioner_fit="whitening")


def test_the_base_class_reads_only_what_both_subclasses_provide():
    """every self.<name> in the source of _FlatStep exists on an object of each subclass built without a device, with the defaults
    and with the features on, except the two that only the row-sharded branches touch; and the source names no subclass's state
    or placement"""
    import re
    source = inspect.getsource(impl._FlatStep)
    names = set(re.findall(r"\bself\.(\w+)", source))
    assert {"_flat_region", "_precondition", "_state_encode", "_state_judge", "_state_commit", "_group"} <= names
    for opt in [cls(_params(), 4, **kw) for kw in ({}, FEATURES) for cls in (psgd.UVd, psgd.SPLU)]:
        missing = sorted(n for n in names if not hasattr(opt, n))
        assert missing == ["_coins", "_sharded"], (type(opt).__name__, missing)
        assert opt._group is None
    named = sorted(a for a in SUBCLASS_STATE if re.search(r"(?<!\w)%s\b" % a, source))
    assert named == [], named
    assert not hasattr(psgd.SPLU(_params(), 4), "_arena")


def test_a_refused_state_dict_leaves_the_optimizer_as_it_was():
    g = torch.Generator().manual_seed(3)
    opt = psgd.SPLU(_params(), 4, generator=g, nonfinite="skip", loss_scale=2 ** 4, preconditioner_fit="whitening", probe_seed=8)
    sd = psgd.SPLU(_params(), 4, generator=torch.Generator().manual_seed(9), nonfinite="skip", loss_scale=2 ** 6, lr_params=0.5,
                   preconditioner_fit="whitening", probe_seed=1).state_dict()
    sd["L12"] = sd["L12"] * 2
    before = (g.get_state().clone(), float(opt.lr_params), float(opt.loss_scale), opt.probe_seed0, opt._L12.clone())
    for bad in (dict(sd, loss_scale=3.0), {k: v for k, v in sd.items() if k != "probe_step"},
                dict(sd, branch_rng=torch.zeros(3, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            opt.load_state_dict(bad)
        assert torch.equal(g.get_state(), before[0]) and float(opt.lr_params) == before[1] and float(opt.loss_scale) == before[2]
        assert opt.probe_seed0 == before[3] and torch.equal(opt._L12, before[4])
    opt.load_state_dict(sd)
    assert float(opt.lr_params) == 0.5 and float(opt.loss_scale) == 64.0 and opt.probe_seed0 == 1 and torch.equal(opt._L12, sd["L12"])
