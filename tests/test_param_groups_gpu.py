"""param_groups= (a learning-rate scale and a weight decay per group of parameter tensors) on the GPU: the functional tails against
a numpy restatement of the arithmetic, both tails of every class bit for bit, neutral groups, a frozen group, schedules, the
launch contract, extents, the row-sharded optimizer and resume.

Five parameter tensors of sizes [1, 5, PSGD_UVD_TAIL_CHUNK + 3, 64, 7]: the third crosses a chunk boundary and no tensor after the
first starts at a multiple of 16 bytes of the flat order in any dtype.  The groups are interleaved: {0, 3}, {2}, the rest implicit.
Class Kron: two small matrices and a vector (any_rank), once with bf16 operands (a mixed gradient list)."""
import numpy as np
import pytest
import torch

from psgd_tf_amd import _lib
from tests import guard_bands

pytestmark = pytest.mark.gpu

CHUNK = _lib.UVD_TAIL_CHUNK
SIZES = [1, 5, CHUNK + 3, 64, 7]
STARTS = [0, 1, 6, CHUNK + 9, CHUNK + 73]
N = sum(SIZES)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TENSOR_GROUPS = [((0, 3), 0.5, 0.0), ((2,), 2.0, 0.0625), ((1, 4), 1.0, 0.01)]
WD = 0.01                                              # the optimizer's own weight decay: what the implicit group follows


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


def _class_groups(ps, neutral=False, frozen=False):
    """the groups of the class tests: {0, 3} and {2} named, {1, 4} implicit"""
    if neutral:                                                        # every group: lr_scale 1.0 and the optimizer's weight decay
        return [{"params": [ps[3], ps[0]], "lr_scale": 1.0, "weight_decay": WD}, {"params": [ps[2]]}]
    first = {"lr_scale": 0.0, "weight_decay": 0.0} if frozen else {"lr_scale": 0.5, "weight_decay": 0.0}
    return [dict(first, params=[ps[3], ps[0]]), {"params": [ps[2]], "lr_scale": 2.0, "weight_decay": 0.0625}]


class Spy:
    """the loaded library behind a recording proxy: the names of the calls that match, in order; only(j): of the calls of the
    *param_update* family the j-th alone reaches the library, the others launch nothing and report success"""

    def __init__(self, lib, keep=lambda name: "param_update" in name or "sumsq" in name, only=None):
        self._lib, self._keep, self._only, self.calls, self._updates = lib, keep, only, [], 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if self._keep(name):
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


# ------------------------------------------------------------------------------------------------------ the restatement (numpy)
def _narrow(x, T):
    """T(x) for a float32 array, as a float32 array: round to nearest even; float32 is the identity"""
    x = np.asarray(x, dtype=np.float32)
    if T == F32:
        return x
    if T == F16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16) & 0xFFFFFFFF
    out = r.astype(np.uint32).view(np.float32).copy()
    out[np.isnan(x)] = np.nan
    return out


def _codes(x, T):
    """the stored bits of the float32 array x, every value a value of T"""
    if T == F32:
        return x.view(np.int32)
    if T == F16:
        return x.astype(np.float16).view(np.int16)
    return (x.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)


def _sr_codes(psgd, x, seed, index0):
    """the bfloat16 codes of SR(x) on the flat indices index0, index0 + 1, ...: (bits(x) + u) >> 16, u the top 16 bits of the
    counter hash of the parameters' rounding stream (tensor id 16)"""
    a, b = psgd.rounding_stream_key(seed, 16)
    M = np.uint64(0xFFFFFFFF)
    i = np.arange(x.size, dtype=np.uint64) + np.uint64(index0)
    z = ((i & M) * np.uint64(0x9E3779B1) + np.uint64(a) + ((i >> np.uint64(32)) & M) * np.uint64(0x85EBCA77)) & M
    z ^= z >> np.uint64(16)
    z = (z * np.uint64(0x7FEB352D)) & M
    z ^= np.uint64(b)
    z ^= z >> np.uint64(15)
    z = (z * np.uint64(0x846CA68B)) & M
    z ^= z >> np.uint64(16)
    u = z >> np.uint64(16)
    code = ((x.view(np.uint32).astype(np.uint64) + u) >> np.uint64(16)) & np.uint64(0xFFFF)
    code[np.isnan(x)] = 0x7FC0
    return code.astype(np.uint16).view(np.int16)


def _restate(psgd, ps, gs, vs, T, lr, groups, clip=None, sr=None):
    """The contract of both tails for float32 arrays ps, gs, vs (vs None or a list; the values of ps and vs are values of T):
    for group j  lr_j = fl32(lr * lr_scale_j)  [the product in double],  lr_eff_j = fl32(double(lr_j) * min(max_norm / (sqrt(S) +
    tiny), 1))  [S: the sum of the fl32 squares of ALL gradients, in double],  c_j = fl32(lr_eff_j * fl32(wd_j)) where wd_j != 0;
    then the chain of Nearest<T>, or of Stochastic for sr = (seed, index0).  Returns the stored bits per tensor."""
    factor = None
    if clip is not None:
        max_norm, tiny = clip
        S = sum(np.sum((g * g).astype(np.float64)) for g in gs)                   # exact for the dyadic gradients of these tests
        factor = min(np.float64(np.float32(max_norm)) / (np.sqrt(np.float64(S)) + np.float64(np.float32(tiny))), np.float64(1.0))
    out = [None] * len(ps)
    for indices, scale, wd in groups:
        lr_eff = np.float32(float(lr) * float(scale))
        if factor is not None:
            lr_eff = np.float32(np.float64(lr_eff) * factor)
        c = np.float32(lr_eff * np.float32(wd)) if np.float32(wd) != 0 else None
        for i in indices:
            p, g = ps[i], gs[i]
            with np.errstate(over="ignore", invalid="ignore"):
                if sr is None:
                    delta = _narrow(lr_eff * g, T)
                    if vs is not None:
                        delta = _narrow(delta + vs[i], T)
                    if c is not None:
                        delta = _narrow(delta + _narrow(c * p, T), T)
                    out[i] = _codes(_narrow(p - delta, T), T)
                else:
                    d = lr_eff * g
                    if vs is not None:
                        d = d + vs[i]
                    if c is not None:
                        d = d + c * p
                    out[i] = _sr_codes(psgd, (p - d).astype(np.float32), sr[0], sr[1] + STARTS[i])
    return out


def _inputs(T, seed=0):
    """numpy float32 arrays (p, g, v per tensor): p and v values of T with +-0, a subnormal and the largest finite value of T among
    them, g dyadic (j / 16, |j| <= 64: the sum of squares is exact in any order) with +-0 among them"""
    rng = np.random.default_rng(seed)
    fi = torch.finfo(T)
    special = np.array([0.0, -0.0, fi.smallest_normal / 4, -fi.smallest_normal / 4, fi.max, -fi.max], dtype=np.float32)
    ps, gs, vs = [], [], []
    for n in SIZES:
        p = _narrow(rng.standard_normal(n).astype(np.float32), T)
        v = _narrow((rng.standard_normal(n) * 2.0 ** -6).astype(np.float32), T)
        g = (rng.integers(-64, 65, n) / 16.0).astype(np.float32)
        if n >= 64:
            p[3:9], p[n - 6:] = special, special[::-1]
            v[1:5] = special[:4]                                                       # (a finite largest value plus v stays finite)
            g[5:7], g[n - 2:] = [0.0, -0.0], [-0.0, 0.0]
        ps.append(p), gs.append(g), vs.append(v)
    ps[0][:] = -0.0                                                                    # the one-element tensor: p = -0, g = 0
    gs[0][:] = 0.0
    return ps, gs, vs


def _to(xs, T):
    return [torch.from_numpy(x.copy()).to(_dev()).to(T) for x in xs]


CASES = [(T, clip, with_vs) for T in (F32, BF16, F16) for clip in (False, True) for with_vs in (False, True)]


@pytest.mark.parametrize("T,clip,with_vs", CASES, ids=lambda x: str(x).replace("torch.", ""))
@pytest.mark.parametrize("tail", ["uvd_step_tail", "multi_param_update"])
def test_functional_tails_equal_the_restatement(psgd, tail, T, clip, with_vs):
    """lr_scale <= 2 and lr = 2^-10 keep the largest finite value finite: |lr_eff g| <= 2^-7 and c |p| <= 2^-13 max(T)"""
    ps, gs, vs = _inputs(T)
    lr, max_norm, tiny = 2.0 ** -10 * 1.2001, 3.0, float(torch.finfo(T).tiny)
    want = _restate(psgd, ps, gs, vs if with_vs else None, T, lr, TENSOR_GROUPS, (max_norm, tiny) if clip else None)
    P, G, V = _to(ps, T), _to(gs, F32), _to(vs, T) if with_vs else None
    if tail == "uvd_step_tail":
        psgd.uvd_step_tail(P, torch.cat(G), lr, max_norm if clip else None, None, V, tensor_groups=TENSOR_GROUPS)
    else:
        sumsq = psgd.multi_sumsq(G).clone() if clip else None
        psgd.multi_param_update(P, G, V, lr, sumsq, max_norm if clip else None, tensor_groups=TENSOR_GROUPS)
    for i, (p, w) in enumerate(zip(P, want)):
        got = _bits(p).cpu().numpy()
        assert np.array_equal(got, w), "tensor %d: %d of %d elements differ, first at %d" % (
            i, int((got != w).sum()), w.size, int(np.flatnonzero(got != w)[0]))
    if clip:                                                                           # the clip is active: the case tests it
        assert np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in gs)) > max_norm


@pytest.mark.parametrize("clip,with_vs", [(False, False), (True, True)])
@pytest.mark.parametrize("tail", ["uvd_step_tail", "multi_param_update", "multi_param_update_mixed"])
def test_functional_tails_stochastic_equal_the_restatement(psgd, tail, clip, with_vs):
    ps, gs, vs = _inputs(BF16, seed=1)
    if tail.endswith("mixed"):                                        # tensors 2 and 4 bring a bfloat16 gradient: dyadic, so exact
        gs = [_narrow(g, BF16) for g in gs]
    lr, max_norm, seed, index0 = 2.0 ** -10 * 1.2001, 3.0, 0xC0FFEE, 2 ** 33 + 5
    want = _restate(psgd, ps, gs, vs if with_vs else None, BF16, lr, TENSOR_GROUPS,
                    (max_norm, float(torch.finfo(BF16).tiny)) if clip else None, sr=(seed, index0))
    P, G, V = _to(ps, BF16), _to(gs, F32), _to(vs, BF16) if with_vs else None
    kw = dict(rounding="stochastic", rounding_seed=seed, index0=index0, tensor_groups=TENSOR_GROUPS)
    if tail == "uvd_step_tail":
        psgd.uvd_step_tail(P, torch.cat(G), lr, max_norm if clip else None, None, V, **kw)
    else:
        if tail.endswith("mixed"):
            G = [g.to(BF16) if i in (2, 4) else g for i, g in enumerate(G)]
        sumsq = psgd.multi_sumsq(G).clone() if clip else None
        psgd.multi_param_update(P, G, V, lr, sumsq, max_norm if clip else None, **kw)
    for i, (p, w) in enumerate(zip(P, want)):
        assert np.array_equal(_bits(p).cpu().numpy(), w), "tensor %d" % i
    # the stored codes do not depend on the grouping: one group with the coefficients of group 1 against three such groups
    one, three = _to(ps, BF16), _to(ps, BF16)
    flat = torch.cat(_to(gs, F32))
    psgd.uvd_step_tail(one, flat, lr, rounding="stochastic", rounding_seed=seed, tensor_groups=[(range(5), 2.0, 0.0625)])
    psgd.uvd_step_tail(three, flat, lr, rounding="stochastic", rounding_seed=seed,
                       tensor_groups=[(g[0], 2.0, 0.0625) for g in TENSOR_GROUPS])
    assert _same(one, three)


# ------------------------------------------------------------------------------------------------------------- the flat classes
_flat_data = {}


def _flat_problem():
    if not _flat_data:
        rng = np.random.default_rng(11)
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(_dev())
        _flat_data.update(a=f(rng.uniform(0.5, 3.0, N)), c=f(rng.standard_normal(N) * 0.01), w0=f(rng.standard_normal(N)),
                          dyadic=f(rng.integers(-64, 65, N) / 16.0))
    return _flat_data


FLAT = {
    "UVd": lambda psgd, ps, **kw: psgd.UVd(ps, rank_of_modification=3, placement=None, **kw),
    "UVd-bf16-state": lambda psgd, ps, **kw: psgd.UVd(ps, rank_of_modification=4, placement=None, state_dtype=BF16, state_route="native", **kw),
    "SPLU": lambda psgd, ps, **kw: psgd.SPLU(ps, rank_of_modification=3, **kw),
    "Dense": lambda psgd, ps, **kw: psgd.Dense(ps, **kw),
}
FEATURES = {
    "plain": {},
    "momentum": dict(momentum=0.9),
    "guard": dict(nonfinite="skip", loss_scale=2.0 ** 8),
    "fd": dict(exact_hessian_vector_product=False),
    "sr": dict(param_rounding="stochastic", param_rounding_seed=0x5EED),
}


def _flat_state(opt, params):
    names = ("_U", "_V", "_d", "_L12", "_l3", "_U12", "_u3")
    state = [getattr(opt, n).clone() for n in names if hasattr(opt, n)]
    if hasattr(opt, "_Qs"):
        state.append(opt.Q.clone())
    if float(opt.momentum) > 0.0:
        state.append(opt._momentum_buffer().clone())
    return [p.detach().clone() for p in params] + state


def _flat_opt(psgd, kind, tail, groups="on", params=None, dyadic=False, seed=5, max_norm=None, **kw):
    d = _flat_problem()
    T = BF16 if kw.get("param_rounding") == "stochastic" else F32
    cuts = np.cumsum([0] + SIZES)
    if params is None:
        params = [d["w0"][cuts[k]:cuts[k + 1]].to(T).clone().requires_grad_(True) for k in range(len(SIZES))]

    def closure():
        w = torch.cat([p.reshape(-1) for p in params]).float()
        if dyadic:                                           # the gradient is a fixed dyadic vector
            return torch.sum(w * d["dyadic"])
        return 0.5 * torch.sum(d["a"] * w * w) + 0.5 * torch.sum(d["c"] * w) ** 2
    if groups is not None:
        kw["param_groups"] = groups if isinstance(groups, list) else _class_groups(params, neutral=groups == "neutral",
                                                                                  frozen=groups == "frozen")
    kw.setdefault("preconditioner_update_probability", 0.0 if dyadic else 1.0)
    opt = FLAT[kind](psgd, params, lr_params=0.02, lr_preconditioner=0.05, grad_clip_max_norm=max_norm,
                     generator=torch.Generator().manual_seed(seed), step_tail=tail, weight_decay=WD, **kw)
    assert (opt._tail is not None) == (tail == "fused")
    return params, opt, closure


_flat_runs = {}


def _warm(psgd):
    """One throw-away step of class UVd at this N before any run that is compared.  The FIRST updating UVd step of a process at
    (N, r) = (4176, 3) ends with V and d a few ulps away from those of every later, identical run -- with or without groups, on
    either tail (measured: 2100 elements of V, 44 of d, at most 1.9e-9 / 6e-8 apart; runs two, three and four agree bit for bit).
    That is the preconditioner's first call, not the step tail, and not what these tests are about."""
    if "warm" not in _flat_runs:
        _flat_runs["warm"] = True
        for kind in ("UVd", "UVd-bf16-state"):
            torch.manual_seed(1)
            _, opt, closure = _flat_opt(psgd, kind, "torch", groups=None)
            opt.step(closure)


def _flat_run(psgd, kind, tail, steps=3, **kw):
    _warm(psgd)
    key = (kind, tail, steps, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _flat_runs:
        torch.manual_seed(100)                               # the probe vectors of :713 / :721 come from the global generator
        params, opt, closure = _flat_opt(psgd, kind, tail, **kw)
        for _ in range(steps):
            opt.step(closure)
        _flat_runs[key] = (_flat_state(opt, params), opt, torch.cuda.get_rng_state())
    return _flat_runs[key]


@pytest.mark.parametrize("feature", list(FEATURES))
@pytest.mark.parametrize("kind", list(FLAT))
def test_flat_class_tails_agree(psgd, kind, feature):
    """3 steps with groups, no clipping (as in the both-tails tests of these classes); each feature switched on once"""
    t, topt, _ = _flat_run(psgd, kind, "torch", **FEATURES[feature])
    f, fopt, _ = _flat_run(psgd, kind, "fused", **FEATURES[feature])
    assert _same(f, t)
    assert all(bool(torch.isfinite(p.float()).all()) for p in f[:5]) and fopt.skipped_steps == 0
    none, _, _ = _flat_run(psgd, kind, "fused", groups=None, **FEATURES[feature])
    assert not _same(f[:5], none[:5])                                                  # the groups do something


@pytest.mark.parametrize("kind", ["UVd", "SPLU", "Dense"])
def test_flat_class_tails_agree_with_clipping_on_dyadic_gradients(psgd, kind):
    """no preconditioner update and a preconditioner that is a power of two times I (the initial factors at scale 1/2; UVd with
    U = 0): the preconditioned gradient is dyadic, its sum of squares exact in any order, the clip active"""
    out = {}
    for tail in ("torch", "fused"):
        torch.manual_seed(100)                               # (the initial U and V of class UVd come from the global generator)
        params, opt, closure = _flat_opt(psgd, kind, tail, dyadic=True, max_norm=0.25, momentum=0.5, preconditioner_init_scale=0.5)
        if kind == "UVd":
            opt._U.zero_()
        for _ in range(3):
            opt.step(closure)
        out[tail] = _flat_state(opt, params)
    assert _same(out["fused"], out["torch"])
    assert not torch.equal(out["fused"][2], _flat_problem()["w0"][6:CHUNK + 9])


@pytest.mark.parametrize("kind", list(FLAT))
def test_flat_class_neutral_groups_are_no_groups(psgd, kind):
    """every group lr_scale 1.0 and the optimizer's weight decay, clip and momentum on, the finite-difference route"""
    kw = dict(max_norm=0.5, momentum=0.9, exact_hessian_vector_product=False)
    a, aopt, _ = _flat_run(psgd, kind, "fused", groups="neutral", **kw)
    b, bopt, _ = _flat_run(psgd, kind, "fused", groups=None, **kw)
    assert [g.indices for g in aopt.param_groups] == [(0, 3), (2,), (1, 4)] and bopt.param_groups is None
    assert _same(a, b)
    assert "param_groups" in aopt.state_dict() and "param_groups" not in bopt.state_dict()


@pytest.mark.parametrize("tail", ["torch", "fused"])
def test_frozen_group(psgd, tail):
    """lr_scale = 0 and weight_decay = 0 on the exact route: tensors 0 and 3 keep their bits; the others are those of a tail call
    that was given only them, with the same preconditioned gradient"""
    torch.manual_seed(100)
    params, opt, closure = _flat_opt(psgd, "SPLU", tail, groups="frozen")
    start = [p.detach().clone() for p in params]
    opt.step(closure)
    assert _same([params[0], params[3]], [start[0], start[3]])
    others = [1, 2, 4]
    alone = [start[i].clone() for i in others]
    pre_grad = torch.cat([opt._out[STARTS[i]:STARTS[i] + SIZES[i]] for i in others])
    psgd.uvd_step_tail(alone, pre_grad, 0.02, tensor_groups=[((1,), 2.0, 0.0625), ((0, 2), 1.0, WD)])
    assert _same([params[i] for i in others], alone) and not _same(alone, [start[i] for i in others])
    opt.step(closure)
    opt.step(closure)
    assert _same([params[0], params[3]], [start[0], start[3]])


def test_schedules_take_effect_at_the_next_step_and_rebuild_nothing(psgd):
    torch.manual_seed(100)
    params, opt, closure = _flat_opt(psgd, "UVd", "fused", max_norm=0.5)
    plan = opt._tail
    opt.step(closure)
    tables = lambda: [plan.chunks.data_ptr(), plan._tables["params"].dev.data_ptr()] + \
        [plan._group_chunks[g.indices][0].data_ptr() for g in opt.param_groups]
    before, n_tables = tables(), (len(plan._group_chunks), len(plan._tables))
    held = params[2].detach().clone()
    opt.param_groups[1].lr_scale.assign(0.0)
    opt.param_groups[1].weight_decay.assign(0.0)
    opt.step(closure)
    assert torch.equal(_bits(params[2]), _bits(held))                                  # group 1 stood still in this step ...
    held1 = params[1].detach().clone()
    opt.param_groups[1].lr_scale.assign(psgd._Hyper(3.0))
    opt.param_groups[2].lr_scale.assign(0.0)
    opt.param_groups[2].weight_decay.assign(0.0)
    opt.step(closure)
    assert not torch.equal(_bits(params[2]), _bits(held)) and torch.equal(_bits(params[1]), _bits(held1))   # ... and moves again
    assert tables() == before and (len(plan._group_chunks), len(plan._tables)) == n_tables
    opt.param_groups[0].weight_decay.assign(-1.0)
    with pytest.raises(ValueError, match=r"UVd: param_groups\[0\]: weight_decay"):
        opt.step(closure)


def test_launch_contract_flat(psgd, hip_lib):
    """G groups: G calls of the *param_update* family after ONE sum of squares; without groups the calls of the commit before"""
    tail_family = lambda name: any(s in name for s in ("param_update", "sumsq", "uvd_pack", "update_apply"))
    for exact in (True, False):
        torch.manual_seed(100)
        params, opt, closure = _flat_opt(psgd, "UVd", "fused", max_norm=0.5, exact_hessian_vector_product=exact)
        opt.step(closure)
        with Spy(hip_lib, tail_family) as spy:
            opt.step(closure)
        perturb = [] if exact else ["psgd_uvd_param_update_multi"]                     # p + v: one launch over all tensors
        assert spy.calls == perturb + ["psgd_uvd_pack_f32"] * 3 + ["psgd_uvd_update_apply_f32", "psgd_uvd_sumsq_f32",
                                                                   "psgd_uvd_param_update_multi", "psgd_uvd_param_update_multi_wd",
                                                                   "psgd_uvd_param_update_multi_wd"]
        params, opt, closure = _flat_opt(psgd, "UVd", "fused", groups=None, max_norm=0.5, exact_hessian_vector_product=exact)
        opt.step(closure)
        with Spy(hip_lib, tail_family) as spy:
            opt.step(closure)
        assert spy.calls == perturb + ["psgd_uvd_pack_f32"] * 3 + ["psgd_uvd_update_apply_f32", "psgd_uvd_sumsq_f32",
                                                                   "psgd_uvd_param_update_multi_wd"]
    params, opt, closure = _flat_opt(psgd, "UVd", "fused", max_norm=0.5, **FEATURES["sr"])
    with Spy(hip_lib) as spy:
        opt.step(closure)
    assert spy.calls == ["psgd_uvd_sumsq_f32"] + ["psgd_uvd_param_update_multi_sr"] * 3


# -------------------------------------------------------------------------------------------------------------------- class Kron
KRON_SHAPES = [(8, 16), (16, 8), (7,)]
_kron_data = {}


def _kron_problem():
    if not _kron_data:
        rng = np.random.default_rng(3)
        f = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(_dev())

        def spd(n):
            a = rng.standard_normal((n, n)) * 0.3
            return a @ a.T / n + np.eye(n)
        _kron_data.update(W=[f(rng.standard_normal(s) * 0.5) for s in KRON_SHAPES], Hl=[f(spd(s[0])) for s in KRON_SHAPES[:2]],
                          Hr=[f(spd(s[1])) for s in KRON_SHAPES[:2]], a=f(rng.uniform(0.5, 2.0, 7)),
                          dyadic=[f(rng.integers(-64, 65, s) / 16.0) for s in KRON_SHAPES])
    return _kron_data


def _kron_groups(ps, neutral=False):
    if neutral:
        return [{"params": [ps[0]], "weight_decay": WD}, {"params": [ps[2]], "lr_scale": 1.0}]
    return [{"params": [ps[0]], "lr_scale": 0.5, "weight_decay": 0.0}, {"params": [ps[2]], "lr_scale": 2.0, "weight_decay": 0.0625}]


def _kron_opt(psgd, tail, groups="on", operands=False, dyadic=False, max_norm=None, **kw):
    d = _kron_problem()
    T = BF16 if kw.get("param_rounding") == "stochastic" else F32
    params = [w.to(T).clone().requires_grad_(True) for w in d["W"]]

    def closure():
        if dyadic:
            return sum(torch.sum(p.float() * g) for p, g in zip(params, d["dyadic"]))
        loss = sum(0.5 * torch.sum(W.float() * (hl @ W.float() @ hr)) for W, hl, hr in zip(params[:2], d["Hl"], d["Hr"]))
        return loss + 0.5 * torch.sum(d["a"] * params[2].float() ** 2)
    if groups is not None:
        kw["param_groups"] = _kron_groups(params, neutral=groups == "neutral")
    if operands:
        kw.update(operands="bfloat16", operand_min_dim=8)
    exact = kw.pop("exact_hessian_vector_product", True)
    opt = psgd.Kron(params, "dense", 1.0, 0.02, 0.05, max_norm, 0.0 if dyadic else 1.0, exact, step_tail=tail,
                    generator=torch.Generator(device=_dev()).manual_seed(9), any_rank=True, weight_decay=WD, **kw)
    assert opt.operand_layers == ([0, 1] if operands else [])
    return params, opt, closure


_kron_runs = {}


def _kron_run(psgd, tail, steps=3, **kw):
    key = (tail, steps, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _kron_runs:
        params, opt, closure = _kron_opt(psgd, tail, **kw)
        for _ in range(steps):
            opt.step(closure)
        state = [p.detach().clone() for p in params] + [q.clone() for pair in opt.factors for q in pair] + [m.clone() for m in opt._m or ()]
        _kron_runs[key] = (state, opt)
    return _kron_runs[key]


@pytest.mark.parametrize("feature", list(FEATURES))
@pytest.mark.parametrize("operands", [False, True], ids=["fp32", "bf16-operands"])
def test_kron_tails_agree(psgd, operands, feature):
    t, topt = _kron_run(psgd, "torch", operands=operands, **FEATURES[feature])
    f, fopt = _kron_run(psgd, "fused", operands=operands, **FEATURES[feature])
    assert [g.indices for g in fopt.param_groups] == [(0,), (2,), (1,)]
    assert _same(f, t)
    assert all(bool(torch.isfinite(p.float()).all()) for p in f[:3]) and fopt.skipped_steps == 0
    none, _ = _kron_run(psgd, "fused", operands=operands, groups=None, **FEATURES[feature])
    assert not _same(f[:3], none[:3])


def test_kron_tails_agree_with_clipping_on_dyadic_gradients(psgd):
    """identity factors, no factor update: the preconditioned gradient is the dyadic gradient and S is exact in any order"""
    kw = dict(dyadic=True, max_norm=2.0, momentum=0.5)
    t, _ = _kron_run(psgd, "torch", **kw)
    f, _ = _kron_run(psgd, "fused", **kw)
    assert _same(f, t) and not torch.equal(f[0], _kron_problem()["W"][0])


@pytest.mark.parametrize("operands", [False, True], ids=["fp32", "bf16-operands"])
def test_kron_neutral_groups_are_no_groups(psgd, operands):
    kw = dict(operands=operands, max_norm=0.5, momentum=0.9, exact_hessian_vector_product=False)
    a, aopt = _kron_run(psgd, "fused", groups="neutral", **kw)
    b, bopt = _kron_run(psgd, "fused", groups=None, **kw)
    assert len(aopt.param_groups) == 3 and bopt.param_groups is None and _same(a, b)
    assert "param_groups" in aopt.state_dict() and "param_groups" not in bopt.state_dict()


def test_launch_contract_kron(psgd, hip_lib):
    for operands, name in ((False, "psgd_multi_param_update%s_f32"), (True, "psgd_multi_param_update_mixed")):
        sumsq = "psgd_multi_sumsq_mixed" if operands else "psgd_multi_sumsq_f32"
        for exact in (True, False):
            params, opt, closure = _kron_opt(psgd, "fused", operands=operands, max_norm=0.5, exact_hessian_vector_product=exact)
            opt.step(closure)
            with Spy(hip_lib) as spy:
                opt.step(closure)
            perturb = [] if exact else ["psgd_multi_param_update_f32"]                 # p + v: one launch over all tensors
            plain = name % "" if "%" in name else name
            decayed = name % "_wd" if "%" in name else name
            assert spy.calls == perturb + [sumsq, plain, decayed, decayed]
            params, opt, closure = _kron_opt(psgd, "fused", groups=None, operands=operands, max_norm=0.5,
                                             exact_hessian_vector_product=exact)
            opt.step(closure)
            with Spy(hip_lib) as spy:
                opt.step(closure)
            assert spy.calls == perturb + [sumsq, decayed]                             # the calls of the commit before this one


def test_kron_resume_restores_the_groups(psgd):
    kw = dict(momentum=0.9, max_norm=0.5)
    whole, _ = _kron_run(psgd, "fused", steps=4, **kw)
    half, hopt = _kron_run(psgd, "fused", steps=2, **kw)
    sd = hopt.state_dict()
    params, opt, closure = _kron_opt(psgd, "fused", **kw)
    for g in opt.param_groups:
        g.lr_scale.assign(9.0)
    with torch.no_grad():
        for p, h in zip(params, half[:3]):
            p.copy_(h)
    opt.load_state_dict(sd)
    assert opt.state_dict()["param_groups"] == sd["param_groups"]
    for _ in range(2):
        opt.step(closure)
    state = [p.detach() for p in params] + [q for pair in opt.factors for q in pair] + list(opt._m)
    assert _same(state, whole)
    sd["param_groups"][0]["indices"] = [0, 1]
    with pytest.raises(ValueError, match="Kron.load_state_dict: 'param_groups'"):
        opt.load_state_dict(sd)


# ----------------------------------------------------------------------------------------------------------------------- extents
@pytest.mark.parametrize("T", [F32, BF16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("tail", ["uvd_step_tail", "multi_param_update"])
def test_extents_and_one_group_alone(psgd, hip_lib, tail, T):
    """parameters, gradient and vs carved out of one pattern-filled arena, each at an address that is a multiple of its element
    size only: nothing outside the parameters changes, the gradient and vs are only read, and the launch of one group writes none
    of the other groups' tensors"""
    ps, gs, vs = _inputs(T, seed=2)
    item = 2 if T == BF16 else 4
    A = guard_bands.Arena(3 * N * 4 + 64 * (2 * 4096 + 64) + (1 << 16), 0xA5, _dev(), guard=4096)
    P = [A.take(n, T, align=item, name="p%d" % i) for i, n in enumerate(SIZES)]
    V = [A.take(n, T, align=item, name="v%d" % i) for i, n in enumerate(SIZES)]
    if tail == "uvd_step_tail":
        G = A.take(N, F32, align=4, name="g")
        G.copy_(torch.from_numpy(np.concatenate(gs)))
        parts = [G[s:s + n] for s, n in zip(STARTS, SIZES)]
    else:
        G = parts = [A.take(n, F32, align=4, name="g%d" % i) for i, n in enumerate(SIZES)]
        for t, g in zip(G, gs):
            t.copy_(torch.from_numpy(g))
    for t, x in zip(V, vs):
        t.copy_(torch.from_numpy(x).to(T))

    def fill():
        for t, x in zip(P, ps):
            t.copy_(torch.from_numpy(x).to(T))

    def run():
        if tail == "uvd_step_tail":
            psgd.uvd_step_tail(P, G, 2.0 ** -10, 3.0, None, V, tensor_groups=TENSOR_GROUPS)
        else:
            psgd.multi_param_update(P, G, V, 2.0 ** -10, sumsq, 3.0, tensor_groups=TENSOR_GROUPS)
    for name in ["v%d" % i for i in range(5)] + (["g"] if tail == "uvd_step_tail" else ["g%d" % i for i in range(5)]):
        A.freeze(name)
    sumsq = psgd.multi_sumsq(parts).clone()
    fill()
    start = [p.clone() for p in P]
    run()
    torch.cuda.synchronize()
    A.check()
    whole = [p.clone() for p in P]
    assert all(not torch.equal(_bits(w), _bits(s)) for w, s in zip(whole[1:], start[1:]))       # (tensor 0: p = -0, g = 0)
    for j, (indices, _, _) in enumerate(TENSOR_GROUPS):
        fill()
        with Spy(hip_lib, only=j) as spy:
            run()
        torch.cuda.synchronize()
        A.check()
        assert len([c for c in spy.calls if "param_update" in c]) == len(TENSOR_GROUPS)
        for i in range(5):
            assert torch.equal(_bits(P[i]), _bits(whole[i] if i in indices else start[i])), (j, i)


# ------------------------------------------------------------------------------------------------------- row-sharded, resume
@pytest.fixture(scope="module")
def pg():
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29587", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("tail", ["fused", "torch"])
def test_one_rank_group_equals_the_unsharded_run(psgd, pg, tail):
    """a 1-rank RCCL group: the exchanges and the one all-reduce of the sum of squares are the identity"""
    kw = dict(max_norm=0.5, momentum=0.9, exact_hessian_vector_product=False)
    sharded, sopt, _ = _flat_run(psgd, "UVd", tail, group=pg, **kw)
    alone, _, _ = _flat_run(psgd, "UVd", tail, **kw)
    assert sopt._group is pg and len(sopt.param_groups) == 3
    assert _same(sharded, alone)


@pytest.mark.parametrize("kind,tail", [("UVd", "fused"), ("UVd-bf16-state", "fused"), ("SPLU", "torch"), ("Dense", "fused")])
def test_resume_is_the_uninterrupted_run(psgd, kind, tail):
    kw = dict(max_norm=0.5, momentum=0.9, exact_hessian_vector_product=False)
    whole, _, _ = _flat_run(psgd, kind, tail, steps=4, **kw)
    half, hopt, cuda_rng = _flat_run(psgd, kind, tail, steps=2, **kw)
    sd = hopt.state_dict()
    assert [g["indices"] for g in sd["param_groups"]] == [[0, 3], [2], [1, 4]]
    params = [p.clone().requires_grad_(True) for p in half[:5]]
    torch.manual_seed(999)
    other = [{"params": [params[0], params[3]], "lr_scale": 7.0}, {"params": [params[2]], "weight_decay": 1.0}]
    params, opt, closure = _flat_opt(psgd, kind, tail, groups=other, params=params, seed=77, **kw)
    opt.load_state_dict(sd)
    assert opt.state_dict()["param_groups"] == sd["param_groups"]
    torch.cuda.set_rng_state(cuda_rng)
    for _ in range(2):
        opt.step(closure)
    assert _same(_flat_state(opt, params), whole)
