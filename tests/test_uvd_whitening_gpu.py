"""UVd(preconditioner_fit="whitening") on the GPU: one step against the fp64 oracle fed counter_randn's probe on every rank family;
the flat probe against multi_randn bit for bit; the two step tails bit for bit; the default path untouched (bits and entry points);
launch counts; one backward only; the guard; native and widened narrow states; row shards (one process, and two processes with
real collectives); resume; and the convergence case of tests/uvd_whitening_cases.py through the class."""
import contextlib
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
from torch.autograd.function import once_differentiable

from oracle import psgd_oracle as orc
from tests import uvd_whitening_cases as wc
from tests.uvd_cases import TINY32, check_bf16_state, rel_err, to_bf16_np
from tests.test_multi_randn_gpu import BAR as PROBE_BAR               # |kernel - counter_randn| per element, that file's bar

pytestmark = pytest.mark.gpu

MIXED = [(7, 5), (3,), (64, 9), (1,)]                                  # 615 elements in four tensors
LR, LR_Q, MAX_NORM, SEED0 = 0.01, 0.1, 0.5, 0x5EED


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import psgd_tf_amd.preconditioned_stochastic_gradient_descent as m      # (the module itself: its globals are patched below)
    return m


def _dev():
    return torch.device("cuda:0")


_data = {}


def _problem(shapes):
    """the initial parameters and the weights a of the loss, float32 device tensors made once per shape list"""
    key = tuple(shapes)
    if key not in _data:
        rng = np.random.default_rng(2026)
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev())
        _data[key] = ([f(rng.standard_normal(s) * 0.5) for s in shapes], [f(np.exp(rng.uniform(-1.0, 1.0, s))) for s in shapes])
    return _data[key]


class _OnceTanh(torch.autograd.Function):
    """tanh whose backward cannot be differentiated again: the stand-in for a fused kernel"""

    @staticmethod
    def forward(ctx, x):
        y = torch.tanh(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return gy * (1.0 - y * y)


def _closure(params, shapes, once=False, calls=None, poison=None):
    """0.5 sum a W^2 + 0.25 sum a tanh(W)^2 in float32; once: the tanh term alone, through the once_differentiable Function;
    poison: a dict whose "x" multiplies the loss (inf: every gradient element that is not 0 overflows)"""
    a_s = _problem(shapes)[1]
    tanh = _OnceTanh.apply if once else torch.tanh

    def closure():
        if calls is not None:
            calls.append(1)
        loss = 0.0
        for p, a in zip(params, a_s):
            W = p.float()
            loss = loss + (0.0 if once else 0.5 * torch.sum(a * W * W)) + 0.25 * torch.sum(a * tanh(W) ** 2)
        if poison is not None and poison["x"] != 1.0:
            loss = loss + params[0].float().reshape(-1)[0] * poison["x"]
        return loss
    return closure


def _make(psgd, tail="fused", *, shapes=MIXED, r=10, dtype=torch.float32, clip=False, prob=1.0, seed=11, fit="whitening", once=False,
          calls=None, poison=None, placement=None, coins=None, **kw):
    params = [w.clone().to(dtype).requires_grad_(True) for w in _problem(shapes)[0]]
    if fit is not None:
        kw = dict(kw, preconditioner_fit=fit)
        if fit == "whitening":
            kw.setdefault("probe_seed", SEED0)
    torch.manual_seed(1234)                                            # the initial U and V come from the global generator
    opt = psgd.UVd(params, r, 1.0, LR, LR_Q, MAX_NORM if clip else None, prob, True, generator=torch.Generator().manual_seed(seed),
                   step_tail=tail, placement=placement, **kw)
    if coins is not None:                                              # (balance, update_U) of every updating call, forced
        opt._update_kw.update(balance=coins[0], update_U=coins[1])
    return params, opt, _closure(params, shapes, once, calls, poison)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy().copy()


def _state(params, opt):
    mom = opt._momentum_buffer() if float(opt.momentum) > 0.0 else None
    return {"tensors": [_bits(t) for t in list(params) + [opt._U, opt._V, opt._d] + ([mom] if mom is not None else [])],
            "counters": (opt._m_step, opt.probe_step, opt._param_round_step, getattr(opt, "_round_step", None), opt.skipped_steps)}


def _assert_same(a, b, what):
    assert len(a["tensors"]) == len(b["tensors"]), what
    for i, (x, y) in enumerate(zip(a["tensors"], b["tensors"])):
        assert x.tobytes() == y.tobytes(), "%s: tensor %d differs" % (what, i)
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])


def _run(psgd, tail, steps, **kw):
    params, opt, closure = _make(psgd, tail, **kw)
    for _ in range(steps):
        opt.step(closure)
    return _state(params, opt), opt


@contextlib.contextmanager
def _recorded(hip_lib):
    """every C-ABI entry point the block calls, in order (the size queries left out)"""
    from psgd_tf_amd import _lib
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("psgd_") and not name.endswith("_bytes"):
                calls.append(name)
            return getattr(hip_lib, name)
    real = _lib._lib
    _lib._lib = Spy()
    try:
        yield calls
    finally:
        _lib._lib = real


def _flat64(ts):
    return np.concatenate([t.detach().float().reshape(-1).cpu().numpy().astype(np.float64) for t in ts])[:, None]


def _n64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# --------------------------------------------------------------------------------------------- one step against the fp64 oracle
ORACLE_CASES = [(MIXED, r, (False, r % 2 == 0)) for r in (1, 10, 20, 32, 33, 64, 70)] + [
    (MIXED, 10, (True, True)), (MIXED, 33, (True, False)),             # the balance branch, below and above rank 32
    ([(1021,)], 10, (False, False)), ([(1021,)], 20, (True, True)), ([(4099,)], 20, (False, True)), ([(4099,)], 33, (False, False)),
    ([(7,)], 10, (False, True)), ([(7,)], 10, (False, False))]         # N < r


@pytest.mark.parametrize("shapes,r,coins", ORACLE_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_one_step_equals_the_oracle_fed_counter_randn(psgd, shapes, r, coins):
    params, opt, closure = _make(psgd, "fused", shapes=shapes, r=r, clip=True, coins=coins)
    N = sum(int(p.numel()) for p in params)
    U, V, d = (_n64(t) for t in (opt._U, opt._V, opt._d))
    start = {"U": U.copy(), "V": V.copy(), "d": d.copy()}
    p0 = _flat64(params)
    with torch.enable_grad():
        g = _flat64(torch.autograd.grad(closure(), params))
    opt.step(closure)
    v32 = psgd.counter_randn(psgd.uvd_step_rounding_seed(SEED0, 0), 0, N)
    perr = float(np.max(np.abs(opt._probe.cpu().numpy().astype(np.float64) - v32.astype(np.float64))))
    assert opt._probe.numel() == N and perr <= PROBE_BAR, perr
    orc.update_precond_UVd_math_(U, V, d, v32.astype(np.float64)[:, None], g, float(np.float32(LR_Q)), TINY32, balance=coins[0],
                                 update_U=coins[1])
    for k, got, ref in (("U", opt._U, U), ("V", opt._V, V), ("d", opt._d, d)):
        got = _n64(got)
        e = rel_err(got, ref)
        moved = np.linalg.norm(ref - start[k])
        inc = np.linalg.norm((got - start[k]) - (ref - start[k])) / moved if moved > 0 else 0.0
        print("N=%d r=%d %s: state %.2e increment %.2e probe %.2e" % (N, r, k, e, inc, perr))
        assert e < 1e-5 and inc < 2e-3, (k, e, inc)
        if moved == 0:
            assert np.array_equal(got, start[k]), k                    # the factor this branch leaves alone
    pre = orc.precond_grad_UVd_math(U, V, d, g)
    want = p0 - float(orc.uvd_clip_lr(pre, LR, MAX_NORM, TINY32)) * pre
    assert rel_err(_flat64(params), want) < 1e-5
    assert opt.probe_step == 1


# ------------------------------------------------------------------------------------------------------------ the probe stream
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("placement", [None, "packed"])
def test_the_flat_probe_is_multi_randn_and_the_counter_counts_updating_steps(psgd, tail, placement):
    poison = {"x": 1.0}
    params, opt, closure = _make(psgd, tail, placement=placement, nonfinite="skip", poison=poison)
    N = sum(int(p.numel()) for p in params)
    want = torch.empty(N, device=_dev())
    for k in range(2):
        opt.step(closure)
        assert opt.probe_step == k + 1
        psgd.multi_randn([want], psgd.uvd_step_rounding_seed(SEED0, k), 0)
        assert _bits(opt._probe).tobytes() == _bits(want).tobytes()
        assert (opt._arena is not None) == (placement is not None)
        assert placement is None or opt._probe.data_ptr() == opt._arena.v.data_ptr()      # drawn into the arena's v region
    kept = _bits(opt._probe)
    opt.preconditioner_update_probability.assign(0.0)                  # a step that leaves the preconditioner alone
    opt.step(closure)
    assert opt.probe_step == 2 and not opt.last_step_skipped
    opt.preconditioner_update_probability.assign(1.0)
    poison["x"] = float("inf")                                         # a skipped step
    opt.step(closure)
    assert opt.probe_step == 2 and opt.last_step_skipped and _bits(opt._probe).tobytes() == kept.tobytes()
    poison["x"] = 1.0
    opt.step(closure)
    assert opt.probe_step == 3 and not opt.last_step_skipped


# ----------------------------------------------------------------------------------------------------- both tails, bit for bit
TAIL_CASES = {
    "plain": {},
    "momentum": dict(momentum=0.9),
    "momentum, weight decay, clipping": dict(momentum=0.9, weight_decay=0.01, clip=True),
    "weight decay, clipping": dict(weight_decay=0.01, clip=True),
    "bfloat16 parameters": dict(dtype=torch.bfloat16, momentum=0.5),
    "bfloat16, stochastic rounding": dict(dtype=torch.bfloat16, param_rounding="stochastic", param_rounding_seed=5, weight_decay=0.01),
    "placed": dict(placement="packed"),
    "placed, momentum, clipping": dict(placement="packed", momentum=0.9, clip=True),
    "rank 40": dict(r=40, momentum=0.9),
}


@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_both_tails_bit_identical_over_five_steps(psgd, name):
    kw = TAIL_CASES[name]
    a, oa = _run(psgd, "torch", 5, prob=0.7, **kw)
    b, ob = _run(psgd, "fused", 5, prob=0.7, **kw)
    _assert_same(b, a, "whitening, %s" % name)
    assert 0 < oa.probe_step == ob.probe_step <= 5
    assert _bits(oa._probe).tobytes() == _bits(ob._probe).tobytes()


# ---------------------------------------------------------------------------------------------------------------- off means off
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_hessian_spelled_out_is_the_default_bit_for_bit_on_the_same_entry_points(psgd, hip_lib, tail, monkeypatch):
    drawn = []
    real = psgd.multi_randn
    monkeypatch.setattr(psgd, "multi_randn", lambda *a, **k: drawn.append(1) or real(*a, **k))
    out = []
    for fit in (None, "hessian"):
        with _recorded(hip_lib) as calls:
            torch.manual_seed(99)
            params, opt, closure = _make(psgd, tail, fit=fit, clip=True, prob=0.7, momentum=0.5)
            torch.manual_seed(7)                                       # the probes of the Hessian fit: the global generator
            for _ in range(5):
                opt.step(closure)
        out.append((_state(params, opt), set(calls), opt))
    _assert_same(out[1][0], out[0][0], "preconditioner_fit='hessian' against no keyword")
    assert out[0][1] == out[1][1] and "psgd_multi_randn_f32" not in out[0][1]
    assert not drawn and all(o.probe_seed0 is None and o._probe is None and o.probe_step == 0 for _, _, o in out)
    assert torch.equal(out[0][2].state_dict()["branch_rng"], out[1][2].state_dict()["branch_rng"])


# ---------------------------------------------------------------------------------------------------------------- launch count
TAIL_ENTRIES = ("psgd_multi_randn_f32", "psgd_uvd_pack", "psgd_uvd_check", "psgd_uvd_sumsq", "psgd_uvd_update_apply",
                "psgd_uvd_wide_update_apply", "psgd_uvd_param_update", "psgd_uvd_apply")


@pytest.mark.parametrize("placement,most", [(None, 5), ("packed", 6)])
def test_launch_count_of_an_updating_step(psgd, hip_lib, monkeypatch, placement, most):
    def refuse(*a, **k):
        raise AssertionError("the whitening route drew from a torch generator")
    params, opt, closure = _make(psgd, "fused", placement=placement)
    opt.step(closure)                                                  # (tables uploaded, buffers made)
    monkeypatch.setattr(psgd, "_randn_like", refuse)
    monkeypatch.setattr(torch, "randn", refuse)
    monkeypatch.setattr(torch, "randn_like", refuse)
    with _recorded(hip_lib) as calls:
        opt.step(closure)
    tail = [c for c in calls if c.startswith(TAIL_ENTRIES)]
    print(placement, tail)
    assert len(tail) <= most, calls
    assert tail.count("psgd_multi_randn_f32") == 1
    assert [c for c in tail if c.startswith("psgd_uvd_pack")] == ["psgd_uvd_pack_f32"] * (1 if placement is None else 2)
    assert "psgd_uvd_update_apply_f32" in tail and "psgd_uvd_param_update_multi" in tail


# ------------------------------------------------------------------------------------------------------------ one backward only
@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_a_once_differentiable_closure_trains_on_one_backward_and_no_global_draw(psgd, tail):
    calls = []
    params, opt, closure = _make(psgd, tail, once=True, calls=calls)
    losses = []
    for k in range(3):
        cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state(_dev())
        losses.append(float(opt.step(closure).detach()))
        assert len(calls) == k + 1                                     # exactly one closure call per step
        assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(_dev()), dev0)
    assert opt.probe_step == 3 and losses[-1] != losses[0] and all(bool(torch.isfinite(p).all()) for p in params)
    opt.exact_hessian_vector_product.assign(False)                     # ignored on this route: still one closure call
    opt.step(closure)
    assert len(calls) == 4 and opt.probe_step == 4
    params, opt, closure = _make(psgd, tail, once=True, fit="hessian")
    with pytest.raises(RuntimeError):                                  # (the text is autograd's and differs between versions)
        opt.step(closure)


# ------------------------------------------------------------------------------------------------------------------------ guard
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_a_skipped_step_keeps_every_bit_and_every_counter(psgd, hip_lib, tail, momentum):
    poison = {"x": 1.0}
    kw = dict(nonfinite="skip", momentum=momentum, dtype=torch.bfloat16, param_rounding="stochastic", param_rounding_seed=3)
    params, opt, closure = _make(psgd, tail, poison=poison, **kw)
    for _ in range(2):
        opt.step(closure)
    before = _state(params, opt)
    poison["x"] = float("inf")
    with _recorded(hip_lib) as calls:
        opt.step(closure)
    assert opt.last_step_skipped and opt.skipped_steps == 1 and "psgd_multi_randn_f32" not in calls
    after = _state(params, opt)
    after["counters"] = after["counters"][:-1] + (0,)                  # (skipped_steps itself counts)
    _assert_same(after, before, "a skipped whitening step")
    poison["x"] = 1.0
    opt.step(closure)
    want, _ = _run(psgd, tail, 3, **kw)                                # the run without the bad step: probe streams 0, 1, 2
    got = _state(params, opt)
    got["counters"] = got["counters"][:-1] + (0,)
    _assert_same(got, want, "the step after a skipped one")


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_a_loss_scale_does_not_move_a_bit_of_a_float32_run(psgd, tail):
    a, _ = _run(psgd, tail, 4, momentum=0.5)
    b, ob = _run(psgd, tail, 4, momentum=0.5, nonfinite="skip", loss_scale=2.0 ** 8)
    assert ob.skipped_steps == 0
    _assert_same(b, a, "float32 whitening run with loss_scale 2^8")
    c, oc = _run(psgd, tail, 4, momentum=0.5, nonfinite="skip", loss_scale="dynamic")
    assert float(oc.loss_scale) == 2.0 ** 16
    _assert_same(c, a, "float32 whitening run with a dynamic loss scale")


# ------------------------------------------------------------------------------------------------------------ narrow states
@pytest.mark.parametrize("r", [20, 32])
def test_native_bf16_state_one_step_against_the_oracle(psgd, r):
    """the bar of the bf16-state family (tests/test_uvd_bf16_gpu.py): every stored code is the floor or the ceiling of the oracle's
    value (check_bf16_state's element bound and share), the share no worse than twice the widened fp32 kernels' plus 1e-4"""
    shapes, coins = [(1021,)], (False, r == 20)
    params, opt, closure = _make(psgd, "fused", shapes=shapes, r=r, coins=coins, state_dtype=torch.bfloat16, state_route="native")
    assert opt._U.dtype == torch.bfloat16
    p = {k: _n64(t) for k, t in (("U", opt._U), ("V", opt._V), ("d", opt._d))}
    with torch.enable_grad():
        g = _flat64(torch.autograd.grad(closure(), params))
    v32 = psgd.counter_randn(psgd.uvd_step_rounding_seed(SEED0, 0), 0, 1021)
    w = {k: torch.from_numpy(x.astype(np.float32)).to(_dev()) for k, x in p.items()}
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(_dev())
    psgd.update_precond_UVd_math_(w["U"], w["V"], w["d"], dv(v32[:, None]), dv(g), LR_Q, TINY32, balance=coins[0], update_U=coins[1])
    q = {k: x.copy() for k, x in p.items()}
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], v32.astype(np.float64)[:, None], g, float(np.float32(LR_Q)), TINY32,
                                 balance=coins[0], update_U=coins[1])
    opt.step(closure)
    stored = {k: _n64(t) for k, t in (("U", opt._U), ("V", opt._V), ("d", opt._d))}
    pn, pw, worst = check_bf16_state("whitening native r=%d" % r, stored, q, {k: t.cpu().numpy() for k, t in w.items()},
                                     {"d", "U" if coins[1] else "V"}, "stochastic")
    print("native r=%d: share of codes off the oracle's pair %.3e (widened fp32 kernels off nearest: %.3e), worst err/bound %.2f"
          % (r, pn, pw, worst))
    assert pn <= 2 * pw + 1e-4
    assert opt.probe_step == 1 and opt._round_step == 1


@pytest.mark.parametrize("state_dtype", [torch.bfloat16, torch.float16])
def test_widen_route_equals_the_fp32_state_run_rounded_once(psgd, state_dtype):
    pa, oa, ca = _make(psgd, "fused", coins=(False, True))
    pb, ob, cb = _make(psgd, "fused", coins=(False, True), state_dtype=state_dtype)
    with torch.no_grad():                                              # the fp32 run starts from the narrow run's stored values
        for x, y in ((oa._U, ob._U), (oa._V, ob._V), (oa._d, ob._d)):
            x.copy_(y.float())
    oa.step(ca)
    ob.step(cb)
    for x, y in ((oa._U, ob._U), (oa._V, ob._V), (oa._d, ob._d)):
        assert y.dtype == state_dtype and _bits(x.to(state_dtype)).tobytes() == _bits(y).tobytes()
    assert _bits(oa._probe).tobytes() == _bits(ob._probe).tobytes()


# ------------------------------------------------------------------------------------------------------------------ row shards
@pytest.fixture(scope="module")
def one_rank_group():
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29591", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("native", [False, True])
def test_a_one_rank_group_is_the_unsharded_optimizer(psgd, one_rank_group, native):
    kw = dict(state_dtype=torch.bfloat16, state_route="native") if native else {}
    a, oa = _run(psgd, "fused", 3, r=20, momentum=0.5, **kw)
    b, ob = _run(psgd, "fused", 3, r=20, momentum=0.5, group=one_rank_group, **kw)
    _assert_same(b, a, "group of one rank against no group")
    assert _bits(oa._probe).tobytes() == _bits(ob._probe).tobytes()


SHARD_N, SHARD_R = 1021, 10


def _shard_setup(psgd, rank, world, group, dev):
    """rank's slice of ONE fixed problem: parameters, gradient weights and the initial state rows; rank None: all of it"""
    from psgd_tf_amd import sharded
    rng = np.random.default_rng(5)
    w0, a = (rng.standard_normal(SHARD_N).astype(np.float32) * 0.5), np.exp(rng.uniform(-1, 1, SHARD_N)).astype(np.float32)
    sc = np.float32((1.0 / (SHARD_N * SHARD_R)) ** 0.5)
    U0, V0 = (rng.standard_normal((SHARD_N, SHARD_R)).astype(np.float32) * sc for _ in range(2))
    lo, hi = (0, SHARD_N) if rank is None else sharded.shard_rows(SHARD_N, rank, world)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x[lo:hi])).to(dev)
    p = f(w0).requires_grad_(True)
    aw = f(a)
    kw = {} if rank is None else dict(group=group)
    opt = psgd.UVd([p], SHARD_R, 1.0, LR, LR_Q, None, 1.0, True, generator=torch.Generator().manual_seed(606 + 13 * (rank or 0)),
                   step_tail="fused", placement=None, preconditioner_fit="whitening", **kw)
    with torch.no_grad():
        opt._U.copy_(f(U0))
        opt._V.copy_(f(V0))
    opt._update_kw.update(balance=False, update_U=True)
    return p, opt, (lambda: 0.5 * torch.sum(aw * p * p) + 0.25 * torch.sum(aw * torch.tanh(p) ** 2)), lo


def _shard_worker(rank, port, outdir, two_devices):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    dev = torch.device("cuda", rank if two_devices else 0)
    torch.cuda.set_device(dev)
    if two_devices:
        dist.init_process_group("nccl", rank=rank, world_size=2, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=2)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import preconditioned_stochastic_gradient_descent as m
    p, opt, closure, lo = _shard_setup(m, rank, 2, dist.group.WORLD, dev)
    opt.step(closure)
    np.savez(os.path.join(outdir, "r%d.npz" % rank), v=opt._probe.cpu().numpy(), U=opt._U.cpu().numpy(), V=opt._V.cpu().numpy(),
             d=opt._d.cpu().numpy(), p=p.detach().cpu().numpy(), seed0=np.array(opt.probe_seed0, dtype=np.uint64),
             step=np.array(opt.probe_step), lo=np.array(lo), backend=np.array(dist.get_backend()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("transport", [
    "gloo-one-device",
    pytest.param("rccl-two-devices", marks=pytest.mark.skipif(torch.cuda.device_count() < 2,
                                                              reason="needs two GPUs (rank k on cuda:k over RCCL)"))])
def test_two_processes_draw_the_rows_of_the_one_process_probe(psgd, transport):
    import torch.multiprocessing as mp
    outdir = tempfile.mkdtemp()
    two = transport == "rccl-two-devices"
    mp.start_processes(_shard_worker, args=(29700 + os.getpid() % 250, outdir, two), nprocs=2, join=True, start_method="spawn")
    sh = [np.load(os.path.join(outdir, "r%d.npz" % k)) for k in range(2)]
    assert str(sh[0]["backend"]) == ("nccl" if two else "gloo")
    assert int(sh[0]["seed0"]) == int(sh[1]["seed0"]) and [int(s["step"]) for s in sh] == [1, 1]     # one probe_seed0 on both ranks
    assert int(sh[0]["lo"]) == 0 and 0 < int(sh[1]["lo"]) < SHARD_N
    p, opt, closure, _ = _shard_setup(psgd, None, 1, None, _dev())
    opt._probe_seed0 = int(sh[0]["seed0"])                               # the seed the ranks drew from their synchronised generator
    opt.step(closure)
    whole = opt._probe.cpu().numpy()
    assert np.concatenate([s["v"] for s in sh]).tobytes() == whole.tobytes()          # index0 = row0: the rows of the one probe
    for k, ref in (("U", opt._U), ("V", opt._V), ("d", opt._d), ("p", p.detach())):
        got = np.concatenate([s[k] for s in sh], 0)
        assert rel_err(got, ref.cpu().numpy()) < 1e-5, k                 # the bar of tests/test_sharded_2proc_gpu.py


# ------------------------------------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("tail", ["torch", "fused"])
@pytest.mark.parametrize("native", [False, True])
def test_resume_is_bit_identical(psgd, tail, native):
    kw = dict(r=20, prob=0.7, momentum=0.9)
    if native:
        kw.update(state_dtype=torch.bfloat16, state_route="native")
    want, _ = _run(psgd, tail, 6, **kw)
    params, opt, closure = _make(psgd, tail, **kw)
    for _ in range(3):
        opt.step(closure)
    sd = opt.state_dict()
    assert sd["probe_seed0"] == SEED0 and sd["probe_step"] == opt.probe_step and "preconditioner_fit" not in sd["hyper"]
    p2, o2, c2 = _make(psgd, tail, **dict(kw, seed=999, probe_seed=1))   # another generator state, another probe seed
    with torch.no_grad():
        for p, s in zip(p2, params):
            p.copy_(s)
    o2.load_state_dict(sd)
    assert o2.probe_seed0 == SEED0 and o2.probe_step == sd["probe_step"]
    for _ in range(3):
        o2.step(c2)
    _assert_same(_state(p2, o2), want, "3 + 3 steps against 6")


def test_an_fp32_checkpoint_continues_on_the_native_route(psgd):
    params, opt, closure = _make(psgd, "fused", r=20)
    for _ in range(2):
        opt.step(closure)
    sd = opt.state_dict()
    p2, o2, c2 = _make(psgd, "fused", r=20, state_dtype=torch.bfloat16, state_route="native", probe_seed=1)
    o2.load_state_dict(sd)
    assert (o2.probe_seed0, o2.probe_step) == (SEED0, 2) and o2._U.dtype == torch.bfloat16
    o2.step(c2)
    assert o2.probe_step == 3 and all(bool(torch.isfinite(t.float()).all()) for t in (o2._U, o2._V, o2._d, *p2))
    want = torch.empty(o2._probe.numel(), device=_dev())
    psgd.multi_randn([want], psgd.uvd_step_rounding_seed(SEED0, 2), 0)
    assert _bits(o2._probe).tobytes() == _bits(want).tobytes()


# ------------------------------------------------------------------------------------------------------------------ convergence
def test_the_class_follows_the_oracle_to_the_whitening_level(psgd):
    """tests/uvd_whitening_cases.py through class UVd, fused tail: the same probes (probe_seed), gradients, coins and initial state.
    At the checkpoints the state is held to the bars of tests/test_trajectory_gpu.py against the fp64 oracle -- drift <= 1e-5 and
    <= 3 max(drift of the fp32 oracle, 1e-7) -- and at the end the variance ratio of the HIP state meets the level the oracle met."""
    keep = (1, 10, 100, 500, 1000, 1500, wc.STEPS)
    (U64, V64, d64), k64 = wc.oracle_run(wc.STEPS, keep=keep)
    _, k32 = wc.oracle_run(wc.STEPS, dtype=np.float32, keep=keep)
    p = torch.zeros(wc.N, device=_dev(), requires_grad=True)
    opt = psgd.UVd([p], wc.R, 1.0, 0.0, wc.LR_PRECOND, None, 1.0, True, generator=torch.Generator().manual_seed(wc.COIN_SEED),
                   step_tail="fused", placement=None, preconditioner_fit="whitening", probe_seed=wc.PROBE_SEED)
    U0, V0, d0 = wc.initial_state(np.float32)
    with torch.no_grad():
        for dst, src in ((opt._U, U0), (opt._V, V0), (opt._d, d0)):
            dst.copy_(torch.from_numpy(src))
    gs = torch.from_numpy(np.stack([wc.gradient(t) for t in range(wc.STEPS)])).to(_dev())
    bad = []
    for t in range(wc.STEPS):
        g = gs[t]
        opt.step(lambda: torch.sum(p * g))
        if t + 1 in keep:
            for k, got, r64, r32 in zip("UVd", (opt._U, opt._V, opt._d), k64[t + 1], k32[t + 1]):
                e, e32 = rel_err(_n64(got), r64), rel_err(r32.astype(np.float64), r64)
                print("t=%d %s drift_hip=%.3e drift_fp32=%.3e" % (t + 1, k, e, e32))
                if not (e <= 1e-5 and e <= 3 * max(e32, 1e-7)):
                    bad.append((t + 1, k, e, e32))
    got = wc.variance_ratio(_n64(opt._U), _n64(opt._V), _n64(opt._d))
    want = wc.variance_ratio(U64, V64, d64)
    print("variance ratio after %d steps: HIP state %.4f, fp64 oracle %.4f" % (wc.STEPS, got, want))
    assert opt.probe_step == wc.STEPS and not bad, bad
    assert want <= wc.LEVEL and got <= wc.LEVEL


# ---------------------------------------------------------------------------------------------------------------------- example
def test_the_example_trains_where_the_hessian_route_raises():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "uvd_whitening.py")
    spec = importlib.util.spec_from_file_location("uvd_whitening_example", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    error, first, last = mod.main(60)
    assert error is not None
    assert np.isfinite(last) and last < first
