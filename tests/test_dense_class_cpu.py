"""class Dense without a device: the class is public and sits on _FlatStep, the constructor's signature and its checks in their
order (each raises before a device is touched: the parameters here are CPU tensors and nothing is launched), the initial state
of demo_usage_of_all_preconditioners.py:28, the checkpoint on CPU tensors, and the unchanged C ABI."""
import inspect
import math
import re

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl

SHAPES = [(3,), (4, 5), (2, 3, 2)]                       # N = 35


def _params(dtype=torch.float32, shapes=SHAPES):
    g = torch.Generator().manual_seed(0)
    return [torch.randn(s, generator=g).to(dtype).requires_grad_(True) for s in shapes]


def test_the_class_is_public_and_sits_on_the_flat_step():
    from psgd_tf_amd import dense_optimizer
    assert psgd.Dense is dense_optimizer.Dense is impl.Dense
    assert psgd.dense_initial_factor is dense_optimizer.dense_initial_factor
    assert issubclass(psgd.Dense, impl._FlatStep) and issubclass(psgd.Dense, impl._StepFeatures)


def test_the_abi_did_not_move():
    """no new exported symbol: the class calls the three dense entry points that were there"""
    from psgd_tf_amd import _lib
    assert _lib.PSGD_ABI_VERSION == 7
    assert _lib.load().psgd_abi_version() == 7
    assert {k for k in _lib.SIGNATURES if k.startswith("psgd_dense_")} == {"psgd_dense_workspace_bytes", "psgd_dense_update_f32",
                                                                           "psgd_dense_apply_f32"}


def test_signature_follows_class_splu():
    """the same names in the same order without the three arguments of the state, so that a user swaps the class name; one
    keyword-only argument more, at the end"""
    d, s = inspect.signature(psgd.Dense.__init__).parameters, inspect.signature(psgd.SPLU.__init__).parameters
    dropped = ("rank_of_modification", "state_dtype", "state_rounding")
    assert list(d) == [k for k in s if k not in dropped] + ["max_num_params"]
    for k in d:
        if k != "max_num_params":
            assert d[k].kind == s[k].kind and d[k].default == s[k].default, k
    assert d["max_num_params"].kind == inspect.Parameter.KEYWORD_ONLY and d["max_num_params"].default == 32768
    assert (d["preconditioner_init_scale"].default, d["lr_params"].default, d["lr_preconditioner"].default) == (0.1, 0.01, 0.1)


def test_defaults_and_initial_state():
    opt = psgd.Dense(_params())
    assert float(opt.lr_params) == 0.01 and float(opt.lr_preconditioner) == 0.1
    assert math.isinf(float(opt.grad_clip_max_norm)) and float(opt.preconditioner_update_probability) == 1.0
    assert bool(opt.exact_hessian_vector_product) and float(opt.momentum) == 0.0 and float(opt.weight_decay) == 0.0
    assert all(isinstance(getattr(opt, k), impl._Hyper) for k in psgd.UVd._HYPER_KEYS + ("momentum", "weight_decay", "loss_scale"))
    assert opt.loss_scale.value is None and opt.skipped_steps == 0 and opt.preconditioner_fit == "hessian"
    assert opt.probe_seed0 is None and opt._tail is None
    assert (opt._rank, opt._store_dtype, opt._state_rounding) == (0, torch.float32, None)
    assert opt._tiny == torch.finfo(torch.float32).tiny and opt._delta_param_scale == torch.finfo(torch.float32).eps ** 0.5
    assert opt.Q.shape == (35, 35) and opt.Q.dtype == torch.float32 and opt.Q.is_contiguous()
    assert torch.equal(opt.Q, torch.tensor(0.1) * torch.eye(35))                    # 0.1 I, the demo's
    assert len(opt._Qs) == 2 and opt.Q is opt._Qs[0] and opt._Qs[1].shape == (35, 35) and opt._Qs[1].dtype == torch.float32
    assert opt._Qs[0].data_ptr() != opt._Qs[1].data_ptr()
    for k in ("v", "h", "g"):
        assert opt._flat_bufs[k].shape == (35,) and opt._flat_bufs[k].dtype == torch.float32
        assert opt._flat_region(k) is opt._flat_bufs[k]
    assert opt._flat_region("probe") is opt._flat_bufs["v"] and opt._flat_region("m") is None
    assert opt._out.shape == (35,) and opt._out.dtype == torch.float32
    half = psgd.Dense(_params(torch.bfloat16), 0.25)                                 # the state is float32 whatever the parameters are
    assert half.Q.dtype == torch.float32 and torch.equal(half.Q, 0.25 * torch.eye(35))
    assert half._tiny == torch.finfo(torch.bfloat16).tiny


def test_dense_initial_factor():
    Q = psgd.dense_initial_factor(5, 0.1)
    assert Q.dtype == torch.float32 and Q.shape == (5, 5) and torch.equal(Q, torch.tensor(0.1) * torch.eye(5))
    assert not bool(torch.triu(Q, 1).any()) and not bool(torch.tril(Q, -1).any())
    Qb = psgd.dense_initial_factor(3, 0.1, torch.bfloat16)
    assert Qb.dtype == torch.bfloat16 and torch.equal(Qb, torch.tensor(0.1).to(torch.bfloat16) * torch.eye(3, dtype=torch.bfloat16))
    assert psgd.dense_initial_factor(1, 2.0).tolist() == [[2.0]]
    assert psgd.dense_initial_factor(4, 1.0, torch.float64, torch.device("cpu")).dtype == torch.float64
    with pytest.raises(ValueError, match="num_params"):
        psgd.dense_initial_factor(0, 1.0)


def test_constructor_checks_in_their_order():
    """every call below is wrong in the argument under test AND in every argument checked after it: the first check speaks"""
    bad_later = dict(max_num_params=34, momentum=2.0, step_tail="x")
    with pytest.raises(TypeError, match="parameters must be"):
        psgd.Dense(_params(torch.float64), param_rounding="x", preconditioner_fit="x", **bad_later)
    with pytest.raises(ValueError, match="param_rounding"):
        psgd.Dense(_params(), param_rounding="x", preconditioner_fit="x", **bad_later)
    with pytest.raises(ValueError, match="param_rounding='stochastic' needs bfloat16"):
        psgd.Dense(_params(), param_rounding="stochastic", preconditioner_fit="x", **bad_later)
    with pytest.raises(ValueError, match="preconditioner_fit"):
        psgd.Dense(_params(), preconditioner_fit="x", **bad_later)
    with pytest.raises(ValueError, match="max_num_params"):
        psgd.Dense(_params(), **bad_later)
    with pytest.raises(ValueError, match="momentum"):
        psgd.Dense(_params(), momentum=2.0, weight_decay=-1.0, step_tail="x")
    with pytest.raises(ValueError, match="weight_decay"):
        psgd.Dense(_params(), weight_decay=-1.0, nonfinite="x", step_tail="x")
    with pytest.raises(ValueError, match="nonfinite"):
        psgd.Dense(_params(), nonfinite="x", loss_scale=3.0, step_tail="x")
    with pytest.raises(ValueError, match="loss_scale needs"):
        psgd.Dense(_params(), loss_scale=2.0, step_tail="x")
    with pytest.raises(ValueError, match="power of two"):
        psgd.Dense(_params(), nonfinite="skip", loss_scale=3.0, step_tail="x")
    with pytest.raises(ValueError, match="step_tail"):
        psgd.Dense(_params(), step_tail="x")


def test_too_many_parameters_names_n_the_bytes_and_the_other_classes():
    with pytest.raises(ValueError) as e:
        psgd.Dense(_params(), max_num_params=34)
    msg = str(e.value)
    assert re.search(r"\b35\b", msg) and str(2 * 4 * 35 * 35) in msg and "SPLU" in msg and "UVd" in msg
    assert psgd.Dense(_params(), max_num_params=35).Q.shape == (35, 35)             # N == max_num_params is allowed
    big = torch.zeros(32769, requires_grad=True)                                     # the default bar; refused before anything is allocated
    with pytest.raises(ValueError, match=str(2 * 4 * 32769 * 32769)):
        psgd.Dense([big])


def test_bad_arguments_draw_nothing_and_good_ones_draw_in_uvd_order():
    """a refused constructor leaves the generator alone; an accepted one draws the parameters' seed, then the probe's (there is no
    rounded state)"""
    g = torch.Generator().manual_seed(7)
    before = g.get_state()
    for bad in (dict(step_tail="x"), dict(max_num_params=3), dict(momentum=2.0)):
        with pytest.raises(ValueError):
            psgd.Dense(_params(torch.bfloat16), generator=g, param_rounding="stochastic", preconditioner_fit="whitening", **bad)
    assert torch.equal(g.get_state(), before)
    opt = psgd.Dense(_params(torch.bfloat16), generator=g, param_rounding="stochastic", preconditioner_fit="whitening")
    g2 = torch.Generator().manual_seed(7)
    want = [int(torch.randint(0, 2 ** 62, (), generator=g2).item()) for _ in range(2)]
    assert [opt._param_round_seed0, opt.probe_seed0] == want and opt._round_seed0 is None
    assert psgd.Dense(_params(), probe_seed=2 ** 64 + 5, preconditioner_fit="whitening").probe_seed0 == 5


def test_parameter_index_is_uvd_param_index():
    two = [torch.tensor(-1.0, requires_grad=True), torch.tensor(1.0, requires_grad=True)]       # hello_psgd.py:7
    opt = psgd.Dense(two)
    assert (opt._param_sizes, opt._param_cumsizes) == psgd.uvd_param_index(two) == ([1, 1], [1, 2]) and opt.Q.shape == (2, 2)
    frozen = torch.zeros(3)                                                                       # requires_grad False: filtered out
    nested = {"b": [_params()[0], frozen], "a": (_params()[1], [_params()[2]])}
    opt = psgd.Dense(nested)
    assert [tuple(p.shape) for p in opt._params] == [(4, 5), (2, 3, 2), (3,)]                    # dict keys sorted, depth first
    assert opt._param_cumsizes == [20, 32, 35]


def test_step_on_the_cpu_is_an_error_not_a_fallback():
    from psgd_tf_amd._lib import PsgdHipError
    params = _params()
    for kw in ({}, dict(preconditioner_update_probability=0.0)):
        opt = psgd.Dense(params, **kw)
        with pytest.raises(PsgdHipError, match="no CPU fallback"):
            opt.step(lambda: sum(torch.sum(p * p) for p in params))
        assert opt._cur == 0 and torch.equal(opt.Q, torch.tensor(0.1) * torch.eye(35))           # refused before the state is touched


FEATURES = dict(momentum=0.9, nonfinite="skip", loss_scale=2 ** 4, preconditioner_fit="whitening")


def test_state_dict_round_trip_on_cpu_tensors():
    g = torch.Generator().manual_seed(3)
    opt = psgd.Dense(_params(), 0.5, lr_params=0.25, generator=g, probe_seed=8, **FEATURES)
    with torch.no_grad():
        opt.Q.copy_(torch.randn(35, 35, generator=torch.Generator().manual_seed(1)))             # a full matrix: the lower triangle travels
        opt._momentum_buffer().copy_(torch.arange(35.0))
    opt._m_step, opt._probe_step = 4, 6
    sd = opt.state_dict()
    assert sd["preconditioner"] == "dense" and sd["format"] == 1 and sd["rank"] == 0 and sd["num_params"] == 35
    assert sd["param_sizes"] == [3, 20, 12] and sd["state_dtype"] == "torch.float32" and sd["state_rounding"] == "none"
    assert sd["Q"].dtype == torch.float32 and sd["Q"].shape == (35, 35) and sd["Q"].data_ptr() != opt.Q.data_ptr()
    assert torch.equal(sd["Q"], opt.Q) and bool(torch.tril(sd["Q"], -1).any())
    assert {"hyper", "branch_rng", "probe_seed0", "probe_step", "momentum_buffer", "momentum_step", "skipped_steps",
            "loss_scale"} <= set(sd)
    assert "round_seed0" not in sd
    twin = psgd.Dense(_params(), generator=torch.Generator().manual_seed(99), probe_seed=1, **FEATURES)
    twin._cur = 1                                           # whichever buffer is the current one takes the load
    other = twin._Qs[0].clone()
    twin.load_state_dict(sd)
    assert twin._cur == 1 and torch.equal(twin.Q, sd["Q"]) and torch.equal(twin._Qs[0], other)
    assert float(twin.lr_params) == 0.25 and twin.probe_seed0 == 8 and twin.probe_step == 6 and twin._m_step == 4
    assert torch.equal(twin._momentum_buffer(), torch.arange(35.0)) and torch.equal(twin._generator.get_state(), g.get_state())
    again = twin.state_dict()
    assert set(again) == set(sd)
    for k in sd:
        if isinstance(sd[k], torch.Tensor):
            assert torch.equal(again[k], sd[k]), k
        else:
            assert again[k] == sd[k], k


def test_a_refused_state_dict_leaves_the_optimizer_as_it_was():
    g = torch.Generator().manual_seed(3)
    opt = psgd.Dense(_params(), generator=g, probe_seed=8, **FEATURES)
    sd = psgd.Dense(_params(), 0.7, lr_params=0.5, generator=torch.Generator().manual_seed(9), probe_seed=1,
                    **dict(FEATURES, loss_scale=2 ** 6)).state_dict()
    splu = psgd.SPLU(_params(), 4, generator=torch.Generator().manual_seed(9), probe_seed=1, **FEATURES).state_dict()

    def snapshot():
        return (g.get_state().clone(), float(opt.lr_params), float(opt.loss_scale), opt.probe_seed0, opt.probe_step, opt._m_step,
                opt.skipped_steps, opt._cur, opt._Qs[0].clone(), opt.Q.data_ptr())
    before = snapshot()
    refused = [(ValueError, dict(sd, Q=sd["Q"][:34])), (ValueError, dict(sd, Q=sd["Q"].reshape(-1))),
               (ValueError, dict(sd, Q=sd["Q"].tolist())),
               (TypeError, dict(sd, Q=sd["Q"].double())), (TypeError, dict(sd, Q=sd["Q"].to(torch.bfloat16))),
               (ValueError, dict(sd, preconditioner="splu")), (ValueError, splu),
               (ValueError, {k: v for k, v in sd.items() if k != "Q"}),
               (ValueError, dict(sd, loss_scale=3.0)), (ValueError, dict(sd, branch_rng=torch.zeros(3, dtype=torch.uint8)))]
    for err, bad in refused:
        with pytest.raises(err):
            opt.load_state_dict(bad)
        after = snapshot()
        assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for a, b in zip(after, before))
    with pytest.raises(ValueError, match="'preconditioner'"):
        opt.load_state_dict(dict(sd, preconditioner="splu"))
    with pytest.raises(ValueError, match="'num_params'"):
        psgd.Dense(_params(shapes=[(6, 6)])).load_state_dict(sd)
    low = dict(sd, Q=sd["Q"] + torch.tril(torch.ones(35, 35), -1))                   # a non-zero lower triangle is accepted
    opt.load_state_dict(low)
    assert float(opt.lr_params) == 0.5 and float(opt.loss_scale) == 64.0 and opt.probe_seed0 == 1 and torch.equal(opt.Q, low["Q"])


SHARED = ("step", "_pack_scale", "_flat", "_momentum_buffer", "_grad_flat", "_grad_cat", "_guarded_grad", "_whitening_inputs",
          "_draw_probe", "_row0", "_init_params", "_init_hypers", "_init_tail", "_draw_seeds", "state_dict", "load_state_dict",
          "_step_grad")
# the members of a step that class Kron shares too: they live on _StepFeatures, and no class below it has a copy
STEP_LAYER = ("_HYPER_KEYS", "_init_step_hypers", "_step_route", "_closure_gradients", "_tail_coefficients", "_fused_tail_kwargs")
SUBCLASS_STATE = ("_Qs", "_cur", "_flat_bufs", "_out")


def test_the_flat_step_is_one_copy_under_the_three_classes():
    """class Dense overrides none of the shared members (tests/test_splu_class_cpu.py holds class UVd and class SPLU to the same)"""
    base = impl._FlatStep
    for f in SHARED:
        assert getattr(psgd.Dense, f) is getattr(base, f), f
        assert f not in vars(psgd.Dense), f
    for f in STEP_LAYER:
        assert getattr(psgd.Dense, f) is getattr(impl._StepFeatures, f), f
        assert f not in vars(psgd.Dense) and f not in vars(base), f
    assert psgd.Dense._HYPER_KEYS is psgd.SPLU._HYPER_KEYS is base._HYPER_KEYS
    own = {k for k in vars(psgd.Dense) if not k.startswith("__")}
    assert own == {"Q", "_flat_region", "_precondition", "_state_encode", "_state_judge", "_state_commit"}, own
    assert "Dense" in base.__doc__ and "SPLU" in base.__doc__ and "UVd" in base.__doc__


def test_the_base_class_reads_only_what_class_dense_provides():
    """every self.<name> in the source of _FlatStep exists on a Dense object built without a device, with the defaults and with
    the features on, except the two that only the row-sharded branches touch; and the source names nothing of this class's state"""
    source = inspect.getsource(impl._FlatStep)
    names = set(re.findall(r"\bself\.(\w+)", source))
    for kw in ({}, dict(FEATURES, loss_scale="dynamic")):
        opt = psgd.Dense(_params(), **kw)
        missing = sorted(n for n in names if not hasattr(opt, n))
        assert missing == ["_coins", "_sharded"], missing
        assert opt._group is None and not hasattr(opt, "_arena")
    named = sorted(a for a in SUBCLASS_STATE if re.search(r"(?<!\w)%s\b" % a, source))
    assert named == [], named
