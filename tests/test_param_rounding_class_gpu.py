"""param_rounding="stochastic" through class Kron and class UVd with every switch on (momentum, weight decay, clipping, the guard
with a loss scale, any_rank and bf16 operands for Kron; the plain, placed and native-bf16 routes for UVd): the torch tail and the
fused tail end bit-identical, a skipped step leaves the parameters and the rounding counter alone, a resumed run is the
uninterrupted one, a 1-rank group is the unsharded optimizer, and "nearest" passed explicitly is the default constructor.

Kron: the LeNet5 layer set in bf16, one 768 x 768 operand layer and one bias vector.  UVd: the 1021 parameters of the RNN demo
(rnn_xor_UVd_preconditioner.py:28-31), r = 10.  Quadratic losses; the closures widen the parameters and compute in float32.
The Inf gradient here is data that the guard must catch."""
import numpy as np
import pytest
import torch

from tests import kron_class_cases as kc

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
KRON_SHAPES = kc.LENET5 + [(768, 768), (84,)]
UVD_SHAPES = [(2, 30), (30, 30), (30,), (30, 1), (1,)]
ON = dict(momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale=2.0 ** 8)
SR = dict(param_rounding="stochastic", param_rounding_seed=0x5EED)


@pytest.fixture(scope="module")
def psgd():
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().reshape(-1).view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(xs, ys):
    return all(x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


# ---------------------------------------------------------------------------------------------------------------------- Kron
_kron_data = {}


def _kron_problem():
    if not _kron_data:
        mats = [s for s in KRON_SHAPES if len(s) == 2]
        Ws, Hls, Hrs = kc.quadratic_problem(mats, 3, scale=0.5)
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(_dev())
        rng = np.random.default_rng(5)
        _kron_data.update(W=[f(w) for w in Ws] + [f(rng.standard_normal(84) * 0.5)], Hl=[f(h) for h in Hls], Hr=[f(h) for h in Hrs],
                          a=f(rng.uniform(0.5, 2.0, 84)))
    return _kron_data


def _kron(psgd, tail, exact, params=None, seed=11, **kw):
    d = _kron_problem()
    params = [w.to(BF).clone().requires_grad_(True) for w in d["W"]] if params is None else params
    bad = {"on": False}

    def closure():
        loss = sum(0.5 * torch.sum(W.float() * (hl @ W.float() @ hr)) for W, hl, hr in zip(params[:-1], d["Hl"], d["Hr"]))
        loss = loss + 0.5 * torch.sum(d["a"] * params[-1].float() ** 2)
        return loss + float("inf") * params[0].float().sum() if bad["on"] else loss
    opt = psgd.Kron(params, "dense", 1.0, 0.05, 0.1, 2.0, 1.0, exact, step_tail=tail,
                    generator=torch.Generator(device=_dev()).manual_seed(seed), any_rank=True, operands="bfloat16", **kw)
    return params, opt, closure, bad


def _kron_state(params, opt):
    return [p.detach().clone() for p in params] + [q.clone() for pair in opt.factors for q in pair] + [m.clone() for m in opt._m or ()]


_kron_runs = {}


def _kron_run(psgd, tail, exact, steps, **kw):
    key = (tail, exact, steps, tuple(sorted(kw.items())))
    if key not in _kron_runs:
        params, opt, closure, _ = _kron(psgd, tail, exact, **kw)
        for _ in range(steps):
            opt.step(closure)
        _kron_runs[key] = (_kron_state(params, opt), opt)
    return _kron_runs[key]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fd"])
def test_kron_tails_agree_with_everything_on(psgd, exact):
    t, topt = _kron_run(psgd, "torch", exact, 3, **ON, **SR)
    f, fopt = _kron_run(psgd, "fused", exact, 3, **ON, **SR)
    assert fopt.operand_layers == [5] and fopt._vec == [6]
    assert _same(f, t)
    assert topt._param_round_step == fopt._param_round_step == 3 and fopt.skipped_steps == 0
    near, _ = _kron_run(psgd, "fused", exact, 3, **ON)
    assert not _same(f[:7], near[:7])                                   # the switch does something
    assert all(bool(torch.isfinite(p.float()).all()) for p in f[:7])


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_kron_skipped_step_leaves_parameters_and_counter(psgd, tail):
    params, opt, closure, bad = _kron(psgd, tail, True, **ON, **SR)
    opt.step(closure)
    before = _kron_state(params, opt)
    bad["on"] = True
    opt.step(closure)
    assert opt.last_step_skipped and opt.skipped_steps == 1 and opt._param_round_step == 1
    assert _same(_kron_state(params, opt), before)
    bad["on"] = False
    opt.step(closure)
    assert opt._param_round_step == 2 and not _same(_kron_state(params, opt)[:7], before[:7])


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_kron_resume_is_the_uninterrupted_run(psgd, tail):
    whole, _ = _kron_run(psgd, tail, False, 4, **ON, **SR)
    half, hopt = _kron_run(psgd, tail, False, 2, **ON, **SR)
    sd = hopt.state_dict()
    assert sd["param_round_step"] == 2 and sd["param_round_seed0"] == 0x5EED
    params = [p.clone().requires_grad_(True) for p in half[:7]]
    params, opt, closure, _ = _kron(psgd, tail, False, params=params, seed=77, **ON, param_rounding="stochastic")
    assert opt._param_round_seed0 != 0x5EED
    opt.load_state_dict(sd)
    assert (opt._param_round_seed0, opt._param_round_step) == (0x5EED, 2)
    for _ in range(2):
        opt.step(closure)
    assert _same(_kron_state(params, opt), whole)
    # a dict without the keys: the optimizer keeps its own seed and counts from 0; a nearest optimizer ignores them
    old = {k: v for k, v in sd.items() if not k.startswith("param_round")}
    opt._param_round_seed0 = 123
    opt.load_state_dict(old)
    assert (opt._param_round_seed0, opt._param_round_step) == (123, 0)
    _, nopt, _, _ = _kron(psgd, tail, False, **ON)
    nopt.load_state_dict(sd)
    assert "param_round_seed0" not in nopt.state_dict()


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_kron_nearest_passed_explicitly_is_the_default(psgd, hip_lib, tail):
    from psgd_tf_amd import _lib
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.endswith("_sr"):
                calls.append(name)
            return getattr(hip_lib, name)
    real = _lib._lib
    _lib._lib = Spy()
    try:
        a, _ = _kron_run(psgd, tail, False, 3, **ON)
        b, bopt = _kron_run(psgd, tail, False, 3, **ON, param_rounding="nearest")
        assert not calls                                                # no new entry point is called
        _kron_run(psgd, tail, False, 1, **ON, **SR)
        assert (sorted(set(calls)) == ["psgd_multi_param_update_mixed_sr"]) == (tail == "fused")
    finally:
        _lib._lib = real
    assert _same(a, b) and bopt._param_round_step == 0 and "param_round_seed0" not in bopt.state_dict()


def test_kron_without_operand_layers_takes_the_fp32_gradient_entry(psgd, hip_lib):
    from psgd_tf_amd import _lib
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.endswith("_sr"):
                calls.append(name)
            return getattr(hip_lib, name)
    d = _kron_problem()
    outs = []
    for tail in ("torch", "fused"):
        params = [w.to(BF).clone().requires_grad_(True) for w in d["W"][:5]]
        opt = psgd.Kron(params, "dense", 1.0, 0.05, 0.1, 2.0, 1.0, False, step_tail=tail,
                        generator=torch.Generator(device=_dev()).manual_seed(3), **ON, **SR)
        closure = lambda: sum(0.5 * torch.sum(W.float() * (hl @ W.float() @ hr)) for W, hl, hr in zip(params, d["Hl"], d["Hr"]))
        real = _lib._lib
        _lib._lib = Spy()
        try:
            for _ in range(3):
                opt.step(closure)
        finally:
            _lib._lib = real
        outs.append([p.detach().clone() for p in params])
    assert sorted(set(calls)) == ["psgd_multi_param_update_sr"]
    assert _same(outs[0], outs[1])


# ----------------------------------------------------------------------------------------------------------------------- UVd
ROUTES = {"plain": dict(placement=None), "placed": dict(placement="packed"),
          "native": dict(placement=None, state_dtype=torch.bfloat16, state_route="native")}


def _uvd(psgd, tail, exact, route, params=None, seed=103, group=None, **kw):
    rng = np.random.default_rng(4)
    n = 1021
    a = torch.from_numpy(rng.uniform(0.5, 3.0, n).astype(np.float32)).to(_dev())
    c = torch.from_numpy((rng.standard_normal(n) * 0.03).astype(np.float32)).to(_dev())
    w0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(_dev())
    cuts = np.cumsum([0] + [int(np.prod(s)) for s in UVD_SHAPES])
    if params is None:
        params = [w0[cuts[k]:cuts[k + 1]].to(BF).view(s).clone().requires_grad_(True) for k, s in enumerate(UVD_SHAPES)]
    bad = {"on": False}

    def closure():
        w = torch.cat([p.reshape(-1) for p in params]).float()
        loss = 0.5 * torch.sum(a * w * w) + 0.5 * torch.sum(c * w) ** 2
        return loss + float("inf") * w[17] if bad["on"] else loss
    opt = psgd.UVd(params, rank_of_modification=10, lr_params=0.1, lr_preconditioner=0.05, grad_clip_max_norm=0.5,
                   exact_hessian_vector_product=exact, generator=torch.Generator().manual_seed(seed), group=group, step_tail=tail,
                   **ROUTES[route], **kw)
    assert (opt._tail is not None) == (tail == "fused") and (opt._arena is not None) == (route == "placed")
    return params, opt, closure, bad


def _uvd_state(params, opt):
    return [p.detach().clone() for p in params] + [opt._U.clone(), opt._V.clone(), opt._d.clone(), opt._momentum_buffer().clone()]


_uvd_runs = {}


def _uvd_run(psgd, tail, exact, route, steps, group=None, **kw):
    key = (tail, exact, route, steps, group is not None, tuple(sorted(kw.items())))
    if key not in _uvd_runs:
        torch.manual_seed(100)
        params, opt, closure, _ = _uvd(psgd, tail, exact, route, group=group, **kw)
        for _ in range(steps):
            opt.step(closure)
        _uvd_runs[key] = (_uvd_state(params, opt), opt, torch.cuda.get_rng_state())
    return _uvd_runs[key]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fd"])
def test_uvd_tails_agree_with_everything_on(psgd, exact, route):
    t, topt, _ = _uvd_run(psgd, "torch", exact, route, 3, **ON, **SR)
    f, fopt, _ = _uvd_run(psgd, "fused", exact, route, 3, **ON, **SR)
    assert _same(f, t)
    assert topt._param_round_step == fopt._param_round_step == 3 and fopt.skipped_steps == 0
    near, _, _ = _uvd_run(psgd, "fused", exact, route, 3, **ON)
    assert not _same(f[:5], near[:5])
    assert all(bool(torch.isfinite(p.float()).all()) for p in f[:5])


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_uvd_skipped_step_leaves_parameters_and_counter(psgd, tail):
    torch.manual_seed(100)
    params, opt, closure, bad = _uvd(psgd, tail, True, "native", **ON, **SR)
    opt.step(closure)
    before = _uvd_state(params, opt)
    bad["on"] = True
    opt.step(closure)
    assert opt.last_step_skipped and opt.skipped_steps == 1 and opt._param_round_step == 1
    assert _same(_uvd_state(params, opt), before)
    bad["on"] = False
    opt.step(closure)
    assert opt._param_round_step == 2 and not _same(_uvd_state(params, opt)[:5], before[:5])


@pytest.mark.parametrize("tail,route", [("torch", "plain"), ("fused", "placed"), ("fused", "native")])
def test_uvd_resume_is_the_uninterrupted_run(psgd, tail, route):
    whole, _, _ = _uvd_run(psgd, tail, False, route, 4, **ON, **SR)
    half, hopt, cuda_rng = _uvd_run(psgd, tail, False, route, 2, **ON, **SR)
    sd = hopt.state_dict()
    assert sd["param_round_step"] == 2 and sd["param_round_seed0"] == 0x5EED
    params = [p.clone().requires_grad_(True) for p in half[:5]]
    torch.manual_seed(999)
    params, opt, closure, _ = _uvd(psgd, tail, False, route, params=params, seed=7, **ON, param_rounding="stochastic")
    assert opt._param_round_seed0 != 0x5EED
    opt.load_state_dict(sd)
    assert (opt._param_round_seed0, opt._param_round_step) == (0x5EED, 2)
    torch.cuda.set_rng_state(cuda_rng)
    for _ in range(2):
        opt.step(closure)
    assert _same(_uvd_state(params, opt), whole)


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_uvd_nearest_passed_explicitly_is_the_default(psgd, hip_lib, tail):
    from psgd_tf_amd import _lib
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.endswith("_sr"):
                calls.append(name)
            return getattr(hip_lib, name)
    real = _lib._lib
    _lib._lib = Spy()
    try:
        a, _, _ = _uvd_run(psgd, tail, False, "plain", 3, **ON)
        b, bopt, _ = _uvd_run(psgd, tail, False, "plain", 3, **ON, param_rounding="nearest")
        assert not calls
        _uvd_run(psgd, tail, False, "plain", 1, **ON, **SR)
        assert (sorted(set(calls)) == ["psgd_uvd_param_update_multi_sr"]) == (tail == "fused")
    finally:
        _lib._lib = real
    assert _same(a, b) and bopt._param_round_step == 0 and "param_round_seed0" not in bopt.state_dict()


# ------------------------------------------------------------------------------------------------------------------- sharded
@pytest.fixture(scope="module")
def pg():
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29581", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("tail,route", [("fused", "plain"), ("torch", "plain"), ("fused", "native")])
def test_one_rank_group_equals_the_unsharded_run(psgd, pg, tail, route):
    """a 1-rank RCCL group: every exchange and the all-reduce of the clip norm are the identity, and row0 = 0"""
    grouped, gopt, _ = _uvd_run(psgd, tail, False, route, 3, group=pg, **ON, **SR)
    alone, _, _ = _uvd_run(psgd, tail, False, route, 3, **ON, **SR)
    assert gopt._param_round_step == 3
    assert _same(grouped, alone)


# ------------------------------------------------------------------------------------------------------------------- example
def test_the_example_stalls_under_nearest_and_progresses_under_stochastic():
    """examples/kron_bf16_stochastic_params.py, 60 steps: under round to nearest no weight is ever rewritten with another value
    and the loss stays where it was; with stochastic rounding it falls"""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "kron_bf16_stochastic_params.py")
    spec = importlib.util.spec_from_file_location("kron_bf16_stochastic_params", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(60)
    first, last, moved = out["nearest"]
    assert moved == 0 and last == first
    first, last, moved = out["stochastic"]
    assert moved > 0 and last < 0.9 * first
