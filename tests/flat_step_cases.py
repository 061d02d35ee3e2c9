"""What tests/test_flat_step_parity_gpu.py and tests/test_flat_step_model_cpu.py share: the switch grid of the flat-vector classes,
the inputs a class and the model of tests/flat_step_model.py are both fed, the comparison of one step, and the bars.

A case is (class, parameter set, tail, fit, dtype, features); it runs STEPS steps with preconditioner_update_probability 0.5.

  * The loss is sum a cosh(W), evaluated in FLOAT64 on both sides (the closure widens the parameters to
    float64; autograd rounds what it hands back to the parameters' dtype T once).  The class and the model then hold the same
    gradients and Hessian-vector products to the last bit: a float32 closure would part from the model's by one T-spacing wherever a
    value lies within 1e-7 of a rounding boundary of T, about thirty times over this grid, each time 1e-4 of a flat vector.
  * The parameters start at +-U(4, 6), the weights are a = 2^-13 exp(U(-1, 1)), the initial scale is 4 (sparse LU: 2), so that
    P = 16 I at the start, and lr_params = 0.05.  The reason is the reference's own arithmetic in T, which the nearest tails keep
    (psgd.py:757-762, uvd_step_tail: delta = T(lr_eff pre), fd: delta = T(delta + v), p <- T(p - delta)): every rounding of delta
    puts about spacing(delta) / (4 spacing(p)) of the elements on the far side of a rounding boundary of p, and on the
    finite-difference route delta carries v, whose size sqrt(eps of T) |N(0, 1)| (0.088 in bfloat16) does not follow the
    parameters (psgd.py:683, :721).  The 2 % cap on such elements can be met by that arithmetic only where spacing(v) is below
    8 % of spacing(p), that is |p| >= 16 |v|: parameters of magnitude 4 and more; and where p and delta cancel, no arithmetic in
    T lands within one spacing of the small difference.  With these inputs the documented arithmetic, restated on the CPU,
    leaves at most 1 % of a case's elements beyond half a spacing.  The weights are that small so that 2^17 a cosh(6) |v| stays
    below float16's 65504.  The price: the float32 rounding of a parameter of magnitude 5 is 1e-5 of its increment, which is
    what the yardstick, and so the increment's bar, shows.
  * The coins come from a CPU generator whose seed is the smallest from 1 on whose replayed coins, the skipped step aside, hold both
    outcomes (coin_seed); the draws of the Hessian fit are the case's own, fed through _randn_like; the whitening probe is
    counter_randn under the object's probe_seed0 and the MODEL's count of probes.
  * max_norm of a clipped case is the geometric mean of the smallest and the largest ||pre|| over the steps of an unclipped float64
    run of the model: the clip then binds in at least one step and not in at least one other, which run() asserts.
  * float32 parameters: the model carries its own and is never given the actor's.  Low-precision parameters: every step of the
    model starts from the actor's stored values, since a nearest tail may land one T-spacing from T(x64) and a stochastic one picks
    either neighbour; the preconditioner state and the momentum buffer are the model's own throughout and never resynchronised.

The bars of state, momentum buffer and float32 increment are not fixed in advance: bars() runs the model in float32 NumPy beside
the float64 run over the whole grid and takes, per model class and quantity, twice the larger of its worst distance and 1e-7; the
cap of 1e-4 is a condition.  profiles/flat_step_parity.txt has the figures.
"""
import collections
import functools
import itertools

import numpy as np
import torch

from tests import flat_step_model as fm
from tests.multi_randn_cases import reference as probe_reference
from tests.uvd_cases import rel_err

SETS = {"N117": [(7, 9), (33,), (2, 2, 2, 2), (5,)], "N132": [(16, 8), (4,)]}
STEPS, INF_STEP, P_UPDATE = 4, 2, 0.5
LR, LR_Q, MOMENTUM, WEIGHT_DECAY, STATIC_SCALE, GROWTH_INTERVAL = 0.05, 0.1, 0.9, 0.01, 2.0 ** 10, 2
# class -> (kind of the pair, rank, further constructor keywords, the model class it is compared with)
CLASSES = {"UVd-r3": ("uvd", 3, {}, "UVd-r3"), "UVd-r10": ("uvd", 10, {}, "UVd-r10"),
           "UVd-r3-packed": ("uvd", 3, {"placement": "packed"}, "UVd-r3"), "UVd-r10-packed": ("uvd", 10, {"placement": "packed"}, "UVd-r10"),
           "SPLU-r3": ("splu", 3, {}, "SPLU-r3"), "Dense": ("dense", 0, {}, "Dense")}
MODEL_CLASSES = ("UVd-r3", "UVd-r10", "SPLU-r3", "Dense")
INIT_SCALE = {"uvd": 4.0, "splu": 2.0, "dense": 4.0}
TAILS = ("torch", "fused")
FITS = ("exact", "fd", "whitening")
DTYPES = {"fp32": ("float32", False), "bf16": ("bfloat16", False), "bf16sr": ("bfloat16", True), "fp16": ("float16", False)}
FEATURES = ("off", "mwc", "static", "dynamic")       # mwc: momentum + weight decay + clip; static / dynamic: mwc + guard + loss scale
LEFT_OUT = ()                                        # combinations a constructor refuses: none on this grid
QUANTITIES = ("state", "momentum", "increment")
SHARE = "share beyond half a spacing"                # of a low-precision nearest case's elements: reported with the distances
BAR_FLOOR, BAR_CAP, BEYOND_HALF_CAP = 1e-7, 1e-4, 0.02
PROBE_SEED0 = 20261021                               # the probe seed of a run without an object (the yardstick)

Key = collections.namedtuple("Key", "model set fit dt feat")           # what the model's inputs depend on
Case = collections.namedtuple("Case", "cls set tail fit dt feat")


def cases():
    return [Case(*c) for c in itertools.product(CLASSES, SETS, TAILS, FITS, DTYPES, FEATURES) if c not in LEFT_OUT]


def key_of(case):
    return Key(CLASSES[case.cls][3], case.set, case.fit, case.dt, case.feat)


def keys():
    return [Key(*k) for k in itertools.product(MODEL_CLASSES, SETS, FITS, DTYPES, FEATURES)]


def kind_rank(model_cls):
    kind, rank = CLASSES[model_cls][:2]
    return kind, rank


def n_of(set_name):
    return sum(int(np.prod(s)) for s in SETS[set_name])


# ----------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def problem(set_name):
    """(W0, a, draws): initial parameters +-U(4, 6), the weights of the loss, and draws[k][i] ~ N(0, 1) in float32 for step k and
    parameter i -- float64 / float32 NumPy arrays; W0 is rounded to the parameters' format by whoever uses it"""
    rng = np.random.default_rng(sum(map(ord, set_name)))
    shapes = SETS[set_name]
    W0 = [rng.uniform(4.0, 6.0, s) * np.sign(rng.standard_normal(s)) for s in shapes]
    a = [2.0 ** -13 * np.exp(rng.uniform(-1.0, 1.0, s)) for s in shapes]
    draws = [[rng.standard_normal(s, dtype=np.float32) for s in shapes] for _ in range(STEPS)]
    return W0, a, draws


def loss_functions(set_name):
    """(grad, hess) of sum a cosh(W): a sinh(W) and the diagonal a cosh(W)"""
    a = problem(set_name)[1]
    return (lambda i, W: a[i] * np.sinh(W)), (lambda i, W: a[i] * np.cosh(W))


def initial_params(key):
    return [fm.round_to(w, DTYPES[key.dt][0]) for w in problem(key.set)[0]]


def poisoned(key, k):
    return key.feat in ("static", "dynamic") and k == INF_STEP


def replayed_coins(key, seed):
    """(coins, branches) of the STEPS steps from the CPU generator alone: first the constructor's draws (the seed of the
    parameters' rounding stream, then the probe seed), then per step the coin and, on a step of class UVd that updates and is not
    skipped, its two branches (balance p = 0.01, update_U p = 0.5): the order tools/class_step_digest.py documents"""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(int(DTYPES[key.dt][1]) + int(key.fit == "whitening")):
        torch.randint(0, 2 ** 62, (), generator=gen)
    coins, branches = [], []
    for k in range(STEPS):
        update = bool(torch.rand((), generator=gen).item() < P_UPDATE)
        coins.append(update)
        branches.append((False, True))
        if update and kind_rank(key.model)[0] == "uvd" and not poisoned(key, k):
            branches[-1] = (bool(torch.rand((), generator=gen).item() < 0.01), bool(torch.rand((), generator=gen).item() < 0.5))
    return coins, branches


@functools.lru_cache(maxsize=None)
def coin_seed(key):
    """the smallest seed from 1 on whose coins, the skipped step aside, hold both outcomes"""
    for seed in range(1, 100):
        coins = replayed_coins(key, seed)[0]
        if len({u for k, u in enumerate(coins) if not poisoned(key, k)}) == 2:
            return seed
    raise AssertionError("%s: no seed below 100 gives both outcomes" % (key,))


def feature_kwargs(key, max_norm):
    """the keywords of the model for the features of a case (the class's: class_kwargs of the GPU test, from the same constants)"""
    kw = dict(fit="whitening" if key.fit == "whitening" else "hessian", exact=key.fit != "fd", stochastic=DTYPES[key.dt][1])
    if key.feat != "off":
        kw.update(momentum=MOMENTUM, weight_decay=WEIGHT_DECAY, max_norm=max_norm)
    if key.feat in ("static", "dynamic"):
        kw.update(guard=True, loss_scale=STATIC_SCALE if key.feat == "static" else "dynamic", growth_interval=GROWTH_INTERVAL)
    return kw


def make_model(key, state, max_norm, dt=np.float64, cls=fm.FlatStepModel):
    grad, hess = loss_functions(key.set)
    return cls(kind_rank(key.model)[0], state, grad, hess, fmt=DTYPES[key.dt][0], lr=LR, lr_preconditioner=LR_Q, dt=dt,
               **feature_kwargs(key, max_norm))


def standin_state(key):
    """an initial state as the constructors' docstrings give it, for runs without an object: U, V ~ N(0, 1) (N r)^-1/2 and
    d = scale; L12 = s [I; 0], l3 = s, U12 = s [I, 0], u3 = s; Q = s I -- float32 values"""
    kind, r = kind_rank(key.model)
    N, s = n_of(key.set), INIT_SCALE[kind]
    if kind == "dense":
        return [(s * np.eye(N)).astype(np.float32)]
    if kind == "splu":
        L12 = np.zeros((N, r), dtype=np.float32)
        L12[:r] = s * np.eye(r)
        l3 = np.full((N - r, 1), s, dtype=np.float32)
        return [L12, l3, L12.T.copy(), l3.copy()]
    rng = np.random.default_rng(N * 100 + r)
    uv = (1.0 / (N * r)) ** 0.5
    return [(rng.standard_normal((N, r)) * uv).astype(np.float32), (rng.standard_normal((N, r)) * uv).astype(np.float32),
            np.full((N, 1), s, dtype=np.float32)]


def nearest_pick(lo, hi, x):
    return np.where(x - lo <= hi - x, lo, hi)


def step_model(model, key, k, params, coins, branches, probe_seed0, pick=nearest_pick):
    """step k of a case on `model` from the values `params`"""
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl
    N = n_of(key.set)
    probe = lambda j: probe_reference(impl, impl.uvd_step_rounding_seed(probe_seed0, j), 0, N)
    return model.step(params, coins[k], draws=problem(key.set)[2][k], probe=probe, branches=branches[k], poison=poisoned(key, k),
                      pick=pick)


def clip_norm(key, state, probe_seed0=PROBE_SEED0):
    """max_norm of a clipped case (None with the features off): the module docstring"""
    if key.feat == "off":
        return None
    coins, branches = replayed_coins(key, coin_seed(key))
    model, params, norms = make_model(key, state, None), initial_params(key), []
    for k in range(STEPS):
        out = step_model(model, key, k, params, coins, branches, probe_seed0)
        params = out["params"]
        if not out["skipped"]:
            norms.append(out["norm"])
    assert len(norms) >= 2 and max(norms) > 1.002 * min(norms), (key, norms)   # (a thousand times what float32 arithmetic moves a norm by)
    return float(np.float32(np.sqrt(min(norms) * max(norms))))


# -------------------------------------------------------------------------------------------------------------- actors
class ModelActor:
    """a FlatStepModel in the place of the class: it carries its own parameters, state and momentum buffer"""

    def __init__(self, key, model, coins, branches, probe_seed0, pick=nearest_pick):
        self.key, self.model, self.coins, self.branches, self.probe_seed0, self.pick = key, model, coins, branches, probe_seed0, pick
        self._params = initial_params(key)

    def params(self):
        return self._params

    def step(self, k):
        m = self.model
        before = ([s.copy() for s in m.state], None if m.m is None else m.m.copy(), self._params)
        out = step_model(m, self.key, k, self._params, self.coins, self.branches, self.probe_seed0, self.pick)
        self._params = out["params"]
        same = lambda xs, ys: all(np.array_equal(x, y) for x, y in zip(xs, ys))
        return dict(counters=m.counters(), state=m.state, m=m.m, params=self._params,
                    same_state=same(before[0], m.state), same_params=same(before[2], self._params),
                    same_m=(before[1] is None and m.m is None) or (before[1] is not None and np.array_equal(before[1], m.m)))


# ---------------------------------------------------------------------------------------------------------- comparison
def compare_step(key, k, fd_update, p_old, obs, rec, model, model_p_old, bars):
    """One step of an actor (obs, from the parameters p_old; fd_update: it perturbed them) against the float64 model (rec = what model.step returned from
    model_p_old).  Returns (violations, distances, (elements beyond half a spacing plus slack, elements judged)).  bars None:
    nothing that needs a bar is judged (the yardstick's first pass)."""
    fmt, stochastic = DTYPES[key.dt]
    bad, dist, beyond = [], {}, (0, 0)
    say = lambda text: bad.append("step %d: %s" % (k + 1, text))
    if tuple(obs["counters"]) != tuple(model.counters()):
        say("counters (skipped_steps, last_step_skipped, loss scale, m_step, probe_step, param_round_step) %r, model %r"
            % (tuple(obs["counters"]), tuple(model.counters())))
    if (not obs["same_state"]) != rec["updated"]:
        say("the state %s, the replayed coin says %s" % ("changed" if not obs["same_state"] else "did not change",
                                                         "skipped" if rec["skipped"] else rec["updated"]))
    if rec["skipped"]:
        if not obs["same_state"] or not obs["same_m"]:
            say("a skipped step changed the bits of the state or the momentum buffer")
        if fd_update:                 # T(T(p + v) - v): the rounding of p + v, at ITS magnitude, and that of the difference
            flat = lambda xs: np.concatenate([np.reshape(np.asarray(x, dtype=np.float64), -1) for x in xs])
            old, new, v = flat(p_old), flat(obs["params"]), flat(rec["v_T"])
            room = 0.5 * fm.spacing(old + v, fmt) + 0.5 * fm.spacing(new, fmt)
            if not np.all(np.abs(new - old) <= room):
                say("a skipped fd step moved %d parameter elements by more than one rounding of %s (worst %.2f of it)"
                    % (int(np.sum(~(np.abs(new - old) <= room))), fmt, float(np.max(np.abs(new - old) / room))))
        elif not obs["same_params"]:
            say("a skipped step changed the bits of the parameters")
        return bad, dist, beyond
    dist["state"] = max(rel_err(a, b) for a, b in zip(obs["state"], model.state))
    if model.m is not None:
        dist["momentum"] = rel_err(obs["m"], model.m)
    flat = lambda xs: np.concatenate([np.reshape(np.asarray(x, dtype=np.float64), -1) for x in xs])
    x64, inc64 = flat(rec["x"]), flat(rec["x"]) - flat(model_p_old)
    got = flat(obs["params"])
    if fmt == "float32":
        dist["increment"] = rel_err(got - flat(p_old), flat(rec["params"]) - flat(model_p_old))
    elif stochastic:
        lo, hi = fm.neighbours(x64, fmt)
        off = int(np.sum((got != lo) & (got != hi)))
        if off:
            say("%d elements are neither T-neighbour of x64" % off)
    else:
        u = np.maximum(fm.spacing(x64, fmt), fm.spacing(got, fmt))
        err = np.abs(got - x64)
        if not np.all(err <= u):
            say("%d elements lie more than one spacing of %s from x64 (worst %.3f)" % (int(np.sum(~(err <= u))), fmt, float(np.max(err / u))))
        if bars is not None:
            beyond = (int(np.sum(err > 0.5 * u + bars["increment"] * np.abs(inc64))), err.size)
    if bars is not None:
        for q, e in dist.items():
            if not e <= bars[q]:
                say("%s: distance %.3e from the model, bar %.3e" % (q, e, bars[q]))
    return bad, dist, beyond


def run(key, actor, model, coins, branches, probe_seed0, bars):
    """All steps of a case: `actor` (the class, or a model in its place) against the float64 `model`.  Returns (violations,
    {quantity: worst distance, and SHARE where elements were judged against half a spacing}).  Asserts what the case itself owes: both outcomes of the coin, the Inf step skipped and no other,
    a dynamic scale that halves and doubles, a clip that binds in one step and not in another."""
    fmt = DTYPES[key.dt][0]
    assert len({u for k, u in enumerate(coins) if not poisoned(key, k)}) == 2, (key, coins)
    bad, worst, beyond, judged, clips, scales = [], {}, 0, 0, [], [model.loss_scale]
    model_params = initial_params(key)
    for k in range(STEPS):
        p_old = actor.params()
        model_p_old = model_params if fmt == "float32" else p_old
        obs = actor.step(k)
        rec = step_model(model, key, k, model_p_old, coins, branches, probe_seed0)
        model_params = rec["params"]
        assert rec["skipped"] == poisoned(key, k), "%s step %d: the model %s" % (key, k + 1, "skipped" if rec["skipped"] else "ran")
        b, d, (nb, nj) = compare_step(key, k, coins[k] and key.fit == "fd", p_old, obs, rec, model, model_p_old, bars)
        bad += b
        beyond, judged = beyond + nb, judged + nj
        for q, e in d.items():
            worst[q] = max(worst.get(q, 0.0), e)
        scales.append(model.loss_scale)
        if not rec["skipped"]:
            clips.append(rec["clip"])
    if key.feat != "off":
        assert min(clips) < 1.0 and max(clips) == 1.0, "%s: clip factors %r" % (key, clips)
    if key.feat == "dynamic":
        ratios = {b / a for a, b in zip(scales, scales[1:])}
        assert ratios >= {0.5, 2.0}, "%s: loss scales %r" % (key, scales)
    if judged:
        worst[SHARE] = beyond / judged
    if judged and not beyond <= BEYOND_HALF_CAP * judged:
        bad.append("%d of %d elements lie further than half a spacing plus slack from x64 (cap %g)" % (beyond, judged, BEYOND_HALF_CAP))
    return bad, worst


# ----------------------------------------------------------------------------------------------------------- the yardstick
def sr_pick(seed):
    """the stochastic rounding of a model in the class's place: up with probability (x - lo) / (hi - lo), from a NumPy generator"""
    rng = np.random.default_rng(seed)

    def pick(lo, hi, x):
        width = np.where(hi > lo, hi - lo, 1.0)
        return np.where(rng.random(np.shape(x)) < (x - lo) / width, hi, lo)
    return pick


def yardstick_case(key, bars=None, actor_cls=fm.FlatStepModel, actor_dt=np.float32):
    """the model in float32 (or `actor_cls`, a mutant, in `actor_dt`) in the class's place against the float64 model, on the
    stand-in initial state: (violations, worst distances)"""
    state = standin_state(key)
    max_norm = clip_norm(key, state)
    coins, branches = replayed_coins(key, coin_seed(key))
    actor = ModelActor(key, make_model(key, state, max_norm, actor_dt, actor_cls), coins, branches, PROBE_SEED0, sr_pick(coin_seed(key)))
    return run(key, actor, make_model(key, state, max_norm), coins, branches, PROBE_SEED0, bars)


@functools.lru_cache(maxsize=None)
def yardstick():
    """{(model class, quantity): the worst distance of the float32 run of the model from its float64 run over the grid}"""
    worst = {(m, q): 0.0 for m in MODEL_CLASSES for q in QUANTITIES}
    for key in keys():
        bad, dist = yardstick_case(key)
        assert not bad, (key, bad)
        for q, e in dist.items():
            worst[(key.model, q)] = max(worst[(key.model, q)], e)
    return worst


def bars(model_cls):
    """{quantity: bar} of a model class: twice the larger of the yardstick's worst distance and BAR_FLOOR; the cap is a condition"""
    out = {q: 2.0 * max(yardstick()[(model_cls, q)], BAR_FLOOR) for q in QUANTITIES}
    assert all(b <= BAR_CAP for b in out.values()), (model_cls, out)
    return out
