"""mixed_dtypes=True on the GPU: one optimizer over float32, bfloat16 and float16 parameter tensors, on both step tails.

The standard mixed list: sizes 1, 7, 4095, 4096, 4097, 8200, 3 (both sides of the 4096-element chunk, a multi-chunk tensor with a
ragged last chunk), dtypes interleaved fp32, bf16, fp16, bf16, fp32, fp16, bf16.  Every tensor is a view at element 1 of a buffer of
its own, so the 16-bit tensors start 2-byte aligned only (and the float32 ones 4-byte aligned only).

The rule under test: each tensor is treated exactly as it would be in a one-dtype optimizer of its own dtype, given the same
float32 preconditioned gradient.  Nothing here has a tolerance: every comparison is of bits."""
import numpy as np
import pytest
import torch

from psgd_tf_amd import _lib
from tests import guard_bands

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SIZES = [1, 7, 4095, 4096, 4097, 8200, 3]
DTYPES = [F32, BF16, F16, BF16, F32, F16, BF16]
DTYPES_SR = [F32, BF16, BF16, BF16, F32, F32, BF16]          # stochastic rounding takes no float16 tensor
STARTS = [int(s) for s in np.cumsum([0] + SIZES[:-1])]
N = sum(SIZES)
CODES = {F32: _lib.DTYPE_F32, BF16: _lib.DTYPE_BF16, F16: _lib.DTYPE_F16}
# a learning rate and a clip at which the 16-bit tensors move: a step of 2e-2 * 1e-2 would be below half a bfloat16 spacing
WD, LR, MAX_NORM = 0.01, 0.5, 50.0


@pytest.fixture(scope="module")
def psgd():
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().reshape(-1).view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(xs, ys):
    xs, ys = list(xs), list(ys)
    return len(xs) == len(ys) and all(x.dtype == y.dtype and torch.equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


def _differ(xs, ys):
    """[] when the two lists hold the same bits, else (position, number of elements that differ) of every entry that does not"""
    xs, ys = list(xs), list(ys)
    assert len(xs) == len(ys) and all(x.dtype == y.dtype and x.shape == y.shape for x, y in zip(xs, ys))
    return [(i, int((_bits(x) != _bits(y)).sum())) for i, (x, y) in enumerate(zip(xs, ys)) if not torch.equal(_bits(x), _bits(y))]


def _odd_view(values, T):
    """the values as a tensor of dtype T that starts at element 1 of a larger buffer: aligned to its element and no better"""
    buf = torch.zeros(values.numel() + 3, dtype=T, device=_dev())
    view = buf[1:1 + values.numel()]
    view.copy_(values)
    assert view.data_ptr() % (2 * view.element_size()) == view.element_size() and view.is_contiguous()
    return view


_data = {}


def _problem():
    """one diagonal-plus-rank-one quadratic over the N elements, made once and never changed"""
    if not _data:
        rng = np.random.default_rng(23)
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(_dev())
        _data.update(a=f(rng.uniform(0.5, 3.0, N)), c=f(rng.standard_normal(N) * 0.01), w0=f(rng.standard_normal(N)),
                     dyadic=f(rng.integers(-64, 65, N) / 16.0), v0=f(rng.standard_normal(N) * 2.0 ** -6))
    return _data


def _params(dtypes, source="w0"):
    w = _problem()[source]
    return [_odd_view(w[s:s + n], T).requires_grad_(True) for s, n, T in zip(STARTS, SIZES, dtypes)]


def _copies(ps):
    return [_odd_view(p.detach(), p.dtype).requires_grad_(p.requires_grad) for p in ps]


KINDS = {
    "UVd": lambda psgd, ps, **kw: psgd.UVd(ps, rank_of_modification=3, placement=None, **kw),
    "SPLU": lambda psgd, ps, **kw: psgd.SPLU(ps, rank_of_modification=3, **kw),
    "Dense": lambda psgd, ps, **kw: psgd.Dense(ps, **kw),
    "Kron": lambda psgd, ps, **kw: psgd.Kron(ps, any_rank=True, **kw),
}


def _groups(ps):
    """two named groups that cut across the dtypes ({0 fp32, 3 bf16, 5 fp16} and {2 fp16}); the rest is the implicit group"""
    return [{"params": [ps[3], ps[0], ps[5]], "lr_scale": 0.5, "weight_decay": 0.0},
            {"params": [ps[2]], "lr_scale": 2.0, "weight_decay": 0.0625}]


def _opt(psgd, kind, tail, params, seed=5, max_norm=MAX_NORM, inf_at=None, **kw):
    d = _problem()
    calls = [0]

    def closure():
        w = torch.cat([p.reshape(-1).float() for p in params])
        loss = 0.5 * torch.sum(d["a"] * w * w) + 0.5 * torch.sum(d["c"] * w) ** 2
        calls[0] += 1
        if inf_at is not None and calls[0] == inf_at:        # an Inf in the gradient of the float16 tensor 5, and of no other
            loss = loss + torch.sum(params[5].float() * float("inf"))
        return loss
    if kw.pop("groups", False):
        kw["param_groups"] = _groups(params)
    kw.setdefault("mixed_dtypes", True)
    opt = KINDS[kind](psgd, params, lr_params=LR, lr_preconditioner=0.05, grad_clip_max_norm=max_norm,
                      generator=torch.Generator().manual_seed(seed), step_tail=tail, weight_decay=WD, **kw)
    assert (opt._tail is not None) == (tail == "fused")
    return opt, closure


def _state(opt, params):
    names = ("_U", "_V", "_d", "_L12", "_l3", "_U12", "_u3")
    state = [getattr(opt, n).clone() for n in names if hasattr(opt, n)]
    if hasattr(opt, "_cur"):
        state.append(opt.Q.clone())
    if hasattr(opt, "factors") and not hasattr(opt, "_L12"):
        state += [q.clone() for pair in opt.factors for q in pair]
    return [p.detach().clone() for p in params] + state


_warmed = []


def _warm(psgd):
    """Throw-away UVd steps at this (N, r) before any run that is compared.  The first updating UVd steps of a process at a shape
    end with V and d (and through them a few float32 parameters) a few ulps from those of every later, identical run
    (tests/test_param_groups_gpu.py: _warm, which found it on the first step).  At this shape it is not only the first: of
    identical one-step runs at the start of a process the third or the fourth was the odd one (two fused runs of the same code,
    seeds and inputs differed in 4 elements of a parameter, 6959 of V and 6 of d; the fifty-odd runs after it all agreed, fused
    and torch alike).  That is the preconditioner's start-up, not the step tail, and not what these tests are about: identical
    one-step runs, the tails in turn, are repeated until three in a row agree bit for bit, and that must happen within ten."""
    if not _warmed:
        _warmed.append(True)
        runs = []
        for k in range(10):
            torch.manual_seed(1)
            params = _params(DTYPES)
            opt, closure = _opt(psgd, "UVd", ("torch", "fused")[k % 2], params)
            opt.step(closure)
            runs.append(_state(opt, params))
            if len(runs) >= 3 and _same(runs[-1], runs[-2]) and _same(runs[-2], runs[-3]):
                return
        raise AssertionError("identical UVd steps did not settle on one result within 10 runs")


def _run(psgd, kind, tail, dtypes=DTYPES, steps=5, **kw):
    _warm(psgd)
    torch.manual_seed(100)                                   # the probe vectors of the flat classes come from the global generator
    params = _params(dtypes)
    opt, closure = _opt(psgd, kind, tail, params, **kw)
    for _ in range(steps):
        opt.step(closure)
    return _state(opt, params), opt


# --------------------------------------------------------------------------- 1. each tensor against its own-dtype call
def _lr_eff(gs, lr, max_norm, tiny):
    """fl32(double(fl32(lr)) * min(max_norm / (sqrt(S) + tiny), 1)) for dyadic gradients, whose sum of squares is exact"""
    S = float(sum(torch.sum(g.double() ** 2) for g in gs))
    factor = min(float(np.float32(max_norm)) / (np.sqrt(S) + float(np.float32(tiny))), 1.0)
    return float(np.float32(np.float64(np.float32(lr)) * factor))


@pytest.mark.parametrize("rounding", ["nearest", "stochastic"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_each_tensor_is_updated_as_in_an_optimizer_of_its_own_dtype(psgd, kind, rounding):
    """the plan the class builds for the standard list, fed a fixed flat gradient with clipping, weight decay and the undo vector:
    tensor i ends with the bits of a ONE-dtype call on that tensor alone with the same lr_eff and, under stochastic rounding, the
    same seed and its flat offset as index0 (its float32 tensors: the nearest call)"""
    sr = rounding == "stochastic"
    dtypes = DTYPES_SR if sr else DTYPES
    d = _problem()
    params = _params(dtypes)
    opt, _ = _opt(psgd, kind, "fused", params, **(dict(param_rounding="stochastic") if sr else {}))
    plan = opt._tail
    assert plan.mixed and opt._mixed and len(plan.by_dtype) == len(set(dtypes))
    assert opt._tiny == max(torch.finfo(T).tiny for T in dtypes)
    gs = [d["dyadic"][s:s + n].clone() for s, n in zip(STARTS, SIZES)]
    vs = [_odd_view(d["v0"][s:s + n], T) for s, n, T in zip(STARTS, SIZES, dtypes)]
    max_norm, seed = 3.0, 0xC0FFEE
    lr_eff = _lr_eff(gs, LR, max_norm, opt._tiny)
    assert lr_eff < float(np.float32(LR))                                                # the clip is active
    alone = _copies(params)
    kw = dict(rounding="stochastic", rounding_seed=seed) if sr else {}
    with torch.no_grad():
        if kind == "Kron":
            sumsq = psgd.multi_sumsq(gs).clone()
            psgd.multi_param_update(params, gs, vs, LR, sumsq, max_norm, opt._tiny, plan=plan, weight_decay=WD, **kw)
        else:
            psgd.uvd_step_tail(params, torch.cat(gs), LR, max_norm, opt._tiny, vs, plan=plan, weight_decay=WD, **kw)
        for i, (p, g, v) in enumerate(zip(alone, gs, vs)):
            kw_i = dict(kw, index0=STARTS[i]) if sr and p.dtype == BF16 else {}
            if kind == "Kron":
                psgd.multi_param_update([p], [g], [v], lr_eff, weight_decay=WD, **kw_i)
            else:
                psgd.uvd_step_tail([p], g, lr_eff, None, None, [v], weight_decay=WD, **kw_i)
    for i, (p, q) in enumerate(zip(params, alone)):
        assert torch.equal(_bits(p), _bits(q)), "tensor %d (%s): %d elements differ" % (
            i, p.dtype, int((_bits(p) != _bits(q)).sum()))
    assert sum(not torch.equal(_bits(p), _bits(q)) for p, q in zip(params, _params(dtypes))) >= 6     # ... and they were updated


def test_the_functional_tail_refuses_a_mixed_list_without_a_plan_for_it(psgd):
    params = _params(DTYPES)
    with pytest.raises(ValueError, match="every tensor must be a contiguous"):
        psgd.uvd_step_tail(params, torch.zeros(N, device=_dev()), LR)
    with pytest.raises(TypeError):
        psgd.multi_param_update(params, [torch.zeros(n, device=_dev()) for n in SIZES], None, LR)


def test_the_shared_constants_do_not_depend_on_the_order(psgd):
    perm = [6, 2, 0, 5, 1, 4, 3]
    params = _params(DTYPES)
    a, _ = _opt(psgd, "UVd", "torch", params)
    b, _ = _opt(psgd, "UVd", "torch", [params[i] for i in perm])
    k, _ = _opt(psgd, "Kron", "torch", [params[i] for i in perm])
    want = (torch.finfo(F16).tiny, torch.finfo(BF16).eps ** 0.5)
    assert (a._tiny, a._delta_param_scale) == (b._tiny, b._delta_param_scale) == (k._tiny, k._delta) == want


# --------------------------------------------------------------------------- 2. both tails, whole steps
FEATURES = {
    "plain": {},
    "momentum": dict(momentum=0.9),
    "guard": dict(nonfinite="skip", loss_scale=2.0 ** 4, inf_at=3),
    "fd": dict(exact_hessian_vector_product=False),
    "whitening": dict(preconditioner_fit="whitening", probe_seed=7),
    "groups": dict(groups=True),
    "sr": dict(param_rounding="stochastic", param_rounding_seed=0x5EED, dtypes=DTYPES_SR),
}


@pytest.mark.parametrize("feature", list(FEATURES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_both_tails_agree_bit_for_bit(psgd, kind, feature):
    """5 whole steps on the standard list with clipping and weight decay on: parameters and preconditioner state"""
    t, topt = _run(psgd, kind, "torch", **FEATURES[feature])
    f, fopt = _run(psgd, kind, "fused", **FEATURES[feature])
    assert fopt._tail.mixed
    assert _differ(f, t) == []
    assert all(bool(torch.isfinite(x.float()).all()) for x in f)
    if feature == "guard":
        assert (topt.skipped_steps, fopt.skipped_steps) == (1, 1)


@pytest.mark.parametrize("tail", ["fused", "torch"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_skipped_step_keeps_every_tensor(psgd, kind, tail):
    """an Inf in the gradient of ONE float16 tensor at step 3: the step is skipped and every tensor of every dtype keeps its bits"""
    kw = dict(nonfinite="skip", loss_scale=2.0 ** 4, inf_at=3)
    before, opt2 = _run(psgd, kind, tail, steps=2, **kw)
    after, opt3 = _run(psgd, kind, tail, steps=3, **kw)
    assert (opt2.skipped_steps, opt3.skipped_steps, opt3.last_step_skipped) == (0, 1, True)
    assert _differ(before, after) == []


# --------------------------------------------------------------------------- 3. one-dtype lists
@pytest.mark.parametrize("T", [F32, BF16, F16], ids=lambda T: str(T)[6:])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_one_dtype_list_does_not_see_the_switch(psgd, kind, T):
    on, oopt = _run(psgd, kind, "fused", dtypes=[T] * len(SIZES), mixed_dtypes=True, exact_hessian_vector_product=False)
    off, fopt = _run(psgd, kind, "fused", dtypes=[T] * len(SIZES), mixed_dtypes=False, exact_hessian_vector_product=False)
    assert not oopt._mixed and not oopt._tail.mixed and len(oopt._tail.by_dtype) == 1
    assert (oopt._tiny, oopt._tail.code) == (fopt._tiny, fopt._tail.code)
    assert _differ(on, off) == []


# --------------------------------------------------------------------------- 4. guard bands
class Spy:
    """the loaded library behind a recording proxy: the names of the typed calls; only(j): of the *param_update* calls the j-th
    alone reaches the library, the others launch nothing and report success (tests/test_param_groups_gpu.py)"""

    def __init__(self, lib, only=None):
        self._lib, self._only, self.calls, self._updates = lib, only, [], 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("psgd_") and "workspace" not in name:
            self.calls.append(name)
        if self._only is not None and "param_update" in name:
            self._updates += 1
            if self._updates - 1 != self._only:
                return lambda *a: 0
        return fn

    def __enter__(self):
        self._real, _lib._lib = _lib._lib, self
        return self

    def __exit__(self, *exc):
        _lib._lib = self._real


def _arena_params(fill):
    A = guard_bands.Arena(sum(n * 4 for n in SIZES) + 2 * len(SIZES) * (4096 + 4096) + (1 << 16), fill, _dev(), guard=4096)
    w = _problem()["w0"]
    ps = []
    for i, (s, n, T) in enumerate(zip(STARTS, SIZES, DTYPES)):
        p = A.take((n,), T, align=16, skew=1, name="p%d" % i)                              # element 1 of a 16-byte line
        p.copy_(w[s:s + n])
        ps.append(p.requires_grad_(True))
    return A, ps


@pytest.mark.parametrize("fill", [0xFF, 0x7F], ids=["nan-ff", "nan-7f"])
@pytest.mark.parametrize("kind", ["UVd", "Kron"])
def test_a_full_fused_step_stays_inside_every_tensor(psgd, kind, fill):
    """the parameters carved out of an arena of NaN / 0xFF bytes with a guard band on either side of each: after a whole fused
    finite-difference step with momentum, the guard and groups, no byte outside any tensor's extent has moved"""
    _warm(psgd)
    A, ps = _arena_params(fill)
    torch.manual_seed(3)
    opt, closure = _opt(psgd, kind, "fused", ps, exact_hessian_vector_product=False, momentum=0.9, nonfinite="skip",
                        loss_scale=2.0 ** 4, groups=True)
    start = [p.detach().clone() for p in ps]
    opt.step(closure)
    torch.cuda.synchronize()
    A.check()
    assert opt.skipped_steps == 0 and sum(not torch.equal(_bits(p), _bits(s)) for p, s in zip(ps, start)) >= 6


@pytest.mark.parametrize("tail", ["uvd_step_tail", "multi_param_update"])
def test_a_launch_of_one_dtype_leaves_the_tensors_of_the_others_alone(psgd, tail):
    """each per-dtype launch of the update alone (the others are swallowed by the spy): the tensors of that dtype end as after the
    whole call, the tensors of the other dtypes keep their bits, and no guard byte moves"""
    from psgd_tf_amd.multi_tail import MultiTailPlan
    d = _problem()
    gs = [d["dyadic"][s:s + n].clone() for s, n in zip(STARTS, SIZES)]
    plan = psgd.UVdTailPlan(SIZES, DTYPES, _dev()) if tail == "uvd_step_tail" else MultiTailPlan(SIZES, _dev(), DTYPES)

    def call(ps):
        with torch.no_grad():
            if tail == "uvd_step_tail":
                psgd.uvd_step_tail(ps, torch.cat(gs), LR, plan=plan, weight_decay=WD)
            else:
                psgd.multi_param_update(ps, gs, None, LR, plan=plan, weight_decay=WD)
    A0, whole = _arena_params(0xFF)
    call(whole)
    for j, (code, _, _) in enumerate(plan.by_dtype):
        A, ps = _arena_params(0xFF)
        start = [p.detach().clone() for p in ps]
        with Spy(_lib.load(), only=j) as spy:
            call(ps)
        torch.cuda.synchronize()
        A.check()
        assert len([c for c in spy.calls if "param_update" in c]) == 3
        for i, T in enumerate(DTYPES):
            assert torch.equal(_bits(ps[i]), _bits(whole[i] if CODES[T] == code else start[i])), (j, i)
        assert sum(not torch.equal(_bits(w), _bits(s)) for w, s in zip(whole, start)) >= 6
    A0.check()


def test_the_launches_of_a_fused_step(psgd):
    """a clipped finite-difference UVd step with two named groups: every typed role once per dtype present, the sum of squares
    once, the update once per (group, dtype) pair -- (packs x D) + sums + pairs"""
    _warm(psgd)
    params = _params(DTYPES)
    opt, closure = _opt(psgd, "UVd", "fused", params, exact_hessian_vector_product=False, groups=True)
    opt.step(closure)
    with Spy(_lib.load()) as spy:
        opt.step(closure)
    tail = [c for c in spy.calls if "pack" in c or "param_update" in c or "sumsq" in c]
    pairs = sum(len(opt._tail.dtype_chunks(g.indices)) for g in opt.param_groups)
    assert pairs == 3 + 1 + 2
    assert len([c for c in tail if "pack" in c]) == 3 * 3                                 # v, h, g
    assert len([c for c in tail if "sumsq" in c]) == 1
    assert len([c for c in tail if "param_update" in c]) == 3 + pairs                      # the perturbation, then the update
    assert len(tail) == psgd.tail_launch_count(DTYPES, SIZES, [g.indices for g in opt.param_groups], packs=4, sums=1)


# --------------------------------------------------------------------------- 5. checkpoints
@pytest.mark.parametrize("kind", ["UVd", "Kron"])
def test_checkpoints_cross_the_switch_and_resume_bit_for_bit(psgd, kind):
    """a dict saved from an all-float32 optimizer loads into the mixed one of the same shapes (and back); a mixed run interrupted
    by state_dict() / load_state_dict() ends with the bits of the uninterrupted one"""
    _warm(psgd)
    kw = dict(momentum=0.9, exact_hessian_vector_product=False)
    torch.manual_seed(50)
    fparams = _params([F32] * len(SIZES))
    fopt, fclosure = _opt(psgd, kind, "fused", fparams, **kw)
    for _ in range(2):
        fopt.step(fclosure)
    sd = fopt.state_dict()
    assert "mixed_dtypes" not in sd and not any("dtype" in k and k != "state_dtype" for k in sd)

    def fresh(seed):
        params = _params(DTYPES)
        opt, closure = _opt(psgd, kind, "fused", params, seed=seed, **kw)
        return params, opt, closure
    torch.manual_seed(60)
    p1, o1, c1 = fresh(11)
    o1.load_state_dict(sd)
    for _ in range(3):
        o1.step(c1)
    torch.manual_seed(60)
    p2, o2, c2 = fresh(12)
    o2.load_state_dict(sd)
    o2.step(c2)
    sd2, rng = o2.state_dict(), torch.cuda.get_rng_state()
    assert "mixed_dtypes" not in sd2
    p3 = _copies(p2)
    o3, c3 = _opt(psgd, kind, "fused", p3, seed=13, **kw)
    o3.load_state_dict(sd2)
    torch.cuda.set_rng_state(rng)
    for _ in range(2):
        o3.step(c3)
    assert _differ(_state(o3, p3), _state(o1, p1)) == []
    fopt.load_state_dict(o1.state_dict())                                                 # ... and back
    fopt.step(fclosure)


# --------------------------------------------------------------------------- 6. a 1-rank group
@pytest.fixture(scope="module")
def pg():
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29593", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield dist.group.WORLD
    dist.destroy_process_group()


def test_one_rank_group_equals_the_unsharded_run(psgd, pg):
    kw = dict(momentum=0.9, exact_hessian_vector_product=False)
    sharded, sopt = _run(psgd, "UVd", "fused", steps=1, group=pg, **kw)
    alone, _ = _run(psgd, "UVd", "fused", steps=1, **kw)
    assert sopt._group is pg and sopt._tail.mixed
    assert _differ(sharded, alone) == []


# --------------------------------------------------------------------------- 7. the second trip of the grid-stride loops
def test_a_sub_plan_longer_than_the_grid(psgd):
    """4200 tensors of 1 .. 3 elements, float32 and bfloat16 in turn: each dtype's sub-plan has 2100 chunks, more than the 2048
    workgroups of a launch, so pack and update reach their last tensors on the second trip of the loop -- against per-tensor
    torch expressions, bit for bit (no clipping: lr_eff = fl32(lr))"""
    k = 4200
    sizes = [1 + i % 3 for i in range(k)]
    dtypes = [F32 if i % 2 == 0 else BF16 for i in range(k)]
    rng = np.random.default_rng(5)
    base = {T: torch.from_numpy(rng.standard_normal(sum(sizes) + 2).astype(np.float32)).to(_dev()).to(T) for T in (F32, BF16)}
    ps, at = [], 1
    for n, T in zip(sizes, dtypes):                          # consecutive views of two buffers, element-aligned only
        ps.append(base[T][at:at + n])
        at += n
    plan = psgd.UVdTailPlan(sizes, dtypes, _dev())
    assert [n for _, _, n in plan.by_dtype] == [2100, 2100] and 2100 > 2048
    out = torch.full((sum(sizes),), float("nan"), device=_dev())
    flat = psgd.uvd_pack(ps, out, 0.5, plan=plan)
    assert torch.equal(_bits(flat), _bits(torch.cat([p.float() * 0.5 for p in ps])))
    g = torch.from_numpy((rng.integers(-64, 65, sum(sizes)) / 16.0).astype(np.float32)).to(_dev())
    want, at = [], 0
    c = float(np.float32(np.float32(LR) * np.float32(WD)))
    for p in ps:
        n = p.numel()
        delta = (float(np.float32(LR)) * g[at:at + n]).to(p.dtype)
        delta = delta + (c * p.float()).to(p.dtype)
        want.append(p - delta)
        at += n
    psgd.uvd_step_tail(ps, g, LR, plan=plan, weight_decay=WD)
    assert _same(ps, want)
