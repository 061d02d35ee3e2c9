"""One step of a flat-vector PSGD optimizer (class UVd, class SPLU, class Dense) restated in NumPy: psgd.py:692-764 plus the
project's extensions (momentum, decoupled weight decay, the clip, nonfinite="skip", static and dynamic loss scale, the
gradient-whitening fit, low-precision parameters with nearest or stochastic rounding).  TEST INFRASTRUCTURE ONLY.

Written from the docstrings of _FlatStep.step, _StepFeatures, uvd_momentum_coefficients, uvd_loss_scale_next, uvd_step_tail and
INTEGRATION.md, not from step() itself; it imports nothing from psgd_tf_amd and uses no autograd.  The preconditioner is the pair of
oracle/psgd_oracle.py; the loss is given by its closed-form gradient and diagonal Hessian, evaluated here in float64 from the stored
parameter values.

    T            the parameters' number format ("float32", "float16", "bfloat16"); T(x) = x rounded to nearest-even in it
    dt           the arithmetic of the step itself: np.float64 (the reference) or np.float32 (the yardstick: what plain float32
                 arithmetic in the same order drifts by).  What autograd forms -- gradients, perturbed gradients, Hessian-vector
                 products -- is evaluated in float64 and rounded to T as torch narrows a float64 tensor (from_autograd) in both, so
                 the two runs see identical inputs.

One step, S the loss scale of this step (1 unguarded), delta = sqrt(eps of T) (psgd.py:683):

    g_T  = T(S grad(W))                                                                       per parameter
    update, hessian fit, exact:   v_T = the draw (in T);  Hv_T = T(S hess(W) v_T);            v = flat(v_T), h = flat(Hv_T) / S
    update, hessian fit, fd:      v_T = T(fl32(draw) fl32(delta));  W <- T(W + v_T);  Hv_T = T(T(S grad(W)) - g_T)
                                                                            v = flat(v_T) / delta, h = flat(Hv_T) / (S delta)
    update, whitening fit:        v = the probe, h = flat(g_T) / S (never the momentum buffer)
    g = flat(g_T) / S
    guard: v, h or g non-finite (a step that leaves the preconditioner alone: g only; the whitening fit: g only, before the probe
           is drawn) -> the step changes nothing but skipped_steps, last_step_skipped and the dynamic scale; fd: W <- T(W - v_T)
    momentum: m <- beta_k m + (1 - beta_k) g, beta_k = float32(min(k / (k + 1), momentum)), k the steps blended so far; m replaces g
    the preconditioner update (when the coin says so) on (v, h), then pre = P g
    lr_eff = lr min(1, max_norm / (||pre|| + tiny of T))
    x = W - lr_eff pre - lr_eff wd W - v_T (the last on the fd route);  W <- T(x), or one of the two T-neighbours of x (stochastic)
"""
import numpy as np

from oracle import psgd_oracle as orc

# significant bits, exponent of the smallest subnormal, largest finite value
FORMATS = {"float32": (24, -149, float(np.finfo(np.float32).max)), "float16": (11, -24, 65504.0),
           "bfloat16": (8, -133, float.fromhex("0x1.fep127"))}


def spacing(x, fmt):
    """the distance between neighbouring values of the format at |x| (float64 array): 2^(e - bits) with 2^(e-1) <= |x| < 2^e"""
    bits, emin, _ = FORMATS[fmt]
    _, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(1.0, np.maximum(e - bits, emin))


def _to_format(x, fmt, op):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = spacing(np.where(np.isfinite(x), x, 0.0), fmt)
        y = op(x / q) * q                                               # q is a power of two: both exact
        return np.where(np.abs(y) > FORMATS[fmt][2], np.sign(x) * np.inf, y)


def round_to(x, fmt):
    """T(x): x (float64) rounded once to the nearest value of the format, ties to even; the result as float64.  Beyond the
    largest finite value: +-Inf; subnormals are kept."""
    if fmt == "float32":
        with np.errstate(over="ignore"):
            return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)
    return _to_format(x, fmt, np.rint)


def neighbours(x, fmt):
    """(the largest value of the format <= x, the smallest >= x)"""
    return _to_format(x, fmt, np.floor), _to_format(x, fmt, np.ceil)


def delta_param_scale(fmt):
    """psgd.py:683 in the parameters' format: sqrt(eps)"""
    if fmt == "bfloat16":                                               # NumPy has no bfloat16: the same formula on eps = 2^-7
        return float(np.float32(2.0 ** -7) ** np.float32(0.5))
    return float(orc.delta_param_scale_of({"float32": np.float32, "float16": np.float16}[fmt]))


def tiny_of(fmt):
    """psgd.py:682: the smallest normal of the format (bfloat16 has float32's exponent range)"""
    return float(orc.tiny_of(np.float16 if fmt == "float16" else np.float32))


def momentum_coefficients(k, momentum):
    """(beta_k, 1 - beta_k) of the k-th blended step, k from 0: beta_k = float32(min(k / (k + 1), momentum)), the first step has
    beta = 0; 1 - beta_k is float32(1) - beta_k, rounded once"""
    beta = np.float32(min(k / (k + 1.0), float(momentum)))
    return float(beta), float(np.float32(1.0) - beta)


def loss_scale_next(scale, good_steps, skipped, growth_interval):
    """the dynamic loss scale after one more step: halved (not below 1) with the counter at 0 on a skipped step, doubled (not
    above 2^24) with the counter at 0 after growth_interval good steps in a row"""
    if skipped:
        return max(scale * 0.5, 1.0), 0
    good_steps += 1
    if good_steps >= growth_interval:
        return min(scale * 2.0, 2.0 ** 24), 0
    return scale, good_steps


# ---------------------------------------------------------------------------------------- the preconditioner pairs of the oracle
def _update(kind, state, v, h, step, tiny, branches):
    """the new state (a list of arrays) after one update on the columns (v, h); the old one is left alone"""
    if kind == "dense":
        return [orc.update_precond_dense(state[0], [v], [h], step)]
    if kind == "splu":
        return list(orc.update_precond_splu(*state, [v], [h], step))
    new = [s.copy() for s in state]
    orc.update_precond_UVd_math_(*new, v, h, step, tiny, balance=branches[0], update_U=branches[1])
    return new


def _apply(kind, state, g):
    if kind == "dense":
        return orc.precond_grad_dense(state[0], [g])[0]
    if kind == "splu":
        return orc.precond_grad_splu(*state, [g])[0]
    return orc.precond_grad_UVd_math(*state, g)


class FlatStepModel:
    """kind: "dense" (state [Q]), "splu" ([L12, l3, U12, u3]) or "uvd" ([U, V, d]); state: the initial state, copied and then
    carried by this object alone.  grad(i, W), hess(i, W): gradient and diagonal Hessian of the loss in parameter i at the values
    W (float64).  loss_scale: None, a power of two, or "dynamic" (starts at 2^16).  The preconditioner arithmetic of class UVd
    takes the tiny of T (psgd.py:733); the dense and sparse-LU pairs take that of their state's dtype."""

    def __init__(self, kind, state, grad, hess, *, fmt, lr, lr_preconditioner, max_norm=None, momentum=0.0, weight_decay=0.0,
                 guard=False, loss_scale=None, growth_interval=2000, fit="hessian", exact=True, stochastic=False, dt=np.float64):
        self.kind, self.fmt, self.dt = kind, fmt, np.dtype(dt)
        self.state = [np.array(s, dtype=dt) for s in state]
        self.grad, self.hess = grad, hess
        self.lr, self.lr_preconditioner, self.max_norm = lr, lr_preconditioner, max_norm
        self.momentum, self.weight_decay, self.guard = momentum, weight_decay, guard
        self.dynamic, self.growth_interval = loss_scale == "dynamic", growth_interval
        self.loss_scale = 2.0 ** 16 if self.dynamic else loss_scale
        self.whiten, self.exact, self.stochastic = fit == "whitening", exact, stochastic
        self.m, self.m_step, self.good_steps = None, 0, 0
        self.skipped_steps, self.last_step_skipped = 0, False
        self.probe_step, self.param_round_step = 0, 0

    # ------------------------------------------------------------------ the pieces a step is made of (each stated once)
    def beta(self, k):
        return momentum_coefficients(k, self.momentum)

    def h_scale(self, S, fd):
        """what the flat h is divided by"""
        return S * (delta_param_scale(self.fmt) if fd else 1.0)

    def v_scale(self, fd):
        """what the flat v is divided by"""
        return delta_param_scale(self.fmt) if fd else 1.0

    def clip_factor(self, pre):
        if self.max_norm is None:
            return 1.0
        dt = self.dt.type
        norm = np.sqrt(np.sum(pre * pre)) + dt(tiny_of(self.fmt))
        return float(min(dt(1.0), dt(self.max_norm) / norm))

    def decay_rate(self, lr_eff):
        """the factor of W in the decay term"""
        return lr_eff * self.weight_decay

    def guard_sees(self, update, v, h, g):
        """the flat vectors the guard judges"""
        return (v, h, g) if update and not self.whiten else (g,)

    def undo_skipped(self, W, v_T):
        """a skipped fd step takes the perturbation back: T(W - v_T)"""
        return [round_to(w - v, self.fmt) for w, v in zip(W, v_T)]

    def narrow(self, x):
        """T(x), nearest"""
        return round_to(x, self.fmt)

    # ------------------------------------------------------------------------------------------------------------ one step
    def from_autograd(self, x):
        """what autograd hands back for the float64 value x of a float64 loss: torch narrows float64 to float16 / bfloat16
        THROUGH float32 (its half types are constructed from float), so T(fl32(x)), two roundings"""
        return round_to(round_to(x, "float32"), self.fmt)

    def _T_grads(self, W, S, poison):
        out = [self.from_autograd(S * self.grad(i, w)) for i, w in enumerate(W)]
        if poison:                                    # a term Inf * sum(parameter 1) in the loss: its gradient is Inf everywhere
            out[1] = out[1] + np.inf
        return out

    def _flat(self, parts, scale):
        flat = np.concatenate([np.reshape(p, -1) for p in parts])
        return ((flat / scale) if scale != 1.0 else flat).astype(self.dt)[:, None]

    def step(self, params, update, *, draws=None, probe=None, branches=(False, True), poison=False, pick=None):
        """params: the values of the parameters before the step (float64 arrays that hold T values).  update: the coin.  draws:
        the standard-normal draws of psgd.py:713 / :721 per parameter (hessian fit, updating step).  probe: k -> the flat probe
        of the k-th step that draws one (whitening fit).  branches: (balance, update_U) of class UVd.  poison: the loss of this
        step carries Inf * sum(parameter 1).  pick: stochastic rounding -- (lo, hi, x) -> the neighbour to take.
        Returns a dict: skipped, updated (the state changed), x (the parameters before the last rounding, in dt), params (after
        it, float64), clip (the factor min(1, ...)) and norm (||pre||), both None on a skipped step, v_T (the perturbation
        or the probe vectors per parameter in T; None where the step drew none)."""
        fmt, dt = self.fmt, self.dt.type
        S = float(self.loss_scale) if self.guard and self.loss_scale is not None else 1.0
        W = [np.asarray(p, dtype=np.float64) for p in params]
        fd = update and not self.whiten and not self.exact
        g_T = self._T_grads(W, S, poison)
        v_T = v = h = None
        if update and self.whiten:
            h = self._flat(g_T, S)
        elif update and self.exact:
            v_T = [round_to(z, fmt) for z in draws]
            Hv_T = [self.from_autograd(S * self.hess(i, w) * z) for i, (w, z) in enumerate(zip(W, v_T))]
            v, h = self._flat(v_T, 1.0), self._flat(Hv_T, self.h_scale(S, False))
        elif update:
            scale = np.float32(delta_param_scale(fmt))
            v_T = [round_to((np.asarray(round_to(z, fmt), dtype=np.float32) * scale).astype(np.float64), fmt) for z in draws]
            W = [round_to(w + z, fmt) for w, z in zip(W, v_T)]                               # psgd.py:723, in T
            with np.errstate(invalid="ignore"):                                             # (Inf - Inf of a poisoned step)
                Hv_T = [round_to(pg - g, fmt) for pg, g in zip(self._T_grads(W, S, poison), g_T)]
            v, h = self._flat(v_T, self.v_scale(True)), self._flat(Hv_T, self.h_scale(S, True))
        g = self._flat(g_T, S)
        if self.guard:
            skipped = not all(np.all(np.isfinite(x)) for x in self.guard_sees(update, v, h, g))
            self.last_step_skipped = skipped
            self.skipped_steps += int(skipped)
            if self.dynamic:
                self.loss_scale, self.good_steps = loss_scale_next(self.loss_scale, self.good_steps, skipped, self.growth_interval)
            if skipped:
                if fd:
                    W = self.undo_skipped(W, v_T)
                return dict(skipped=True, updated=False, x=None, params=W, clip=None, norm=None, v_T=v_T)
        if update and self.whiten:
            v = np.asarray(probe(self.probe_step), dtype=self.dt).reshape(-1, 1)
            self.probe_step += 1
        if self.momentum != 0.0:
            beta, omb = self.beta(self.m_step)
            self.m_step += 1
            self.m = dt(omb) * g if beta == 0.0 or self.m is None else dt(beta) * self.m + dt(omb) * g
            g = self.m
        else:
            self.m_step = 0
        if update:
            tiny = tiny_of(fmt) if self.kind == "uvd" else None
            self.state = _update(self.kind, self.state, v, h, self.lr_preconditioner, tiny, branches)
        pre = _apply(self.kind, self.state, g)
        clip = self.clip_factor(pre)
        lr_eff = dt(self.lr) * dt(clip)
        decay = dt(self.decay_rate(lr_eff))
        x, i = [], 0
        for k, w in enumerate(W):
            w = w.astype(self.dt)
            xk = w - lr_eff * pre[i:i + w.size, 0].reshape(w.shape) - decay * w
            if fd:
                xk = xk - v_T[k].astype(self.dt)
            x.append(xk)
            i += w.size
        if self.stochastic:
            self.param_round_step += 1
            new = [pick(*neighbours(xk.astype(np.float64), fmt), xk.astype(np.float64)) for xk in x]
        else:
            new = [self.narrow(xk.astype(np.float64)) for xk in x]
        return dict(skipped=False, updated=bool(update), x=x, params=new, clip=clip, norm=float(np.sqrt(np.sum(pre * pre))), v_T=v_T,
                    pre=pre, lr_eff=float(lr_eff))

    def counters(self):
        """(skipped_steps, last_step_skipped, loss scale, steps blended into the momentum buffer, probes drawn, steps that
        rounded the parameters stochastically)"""
        return (self.skipped_steps, self.last_step_skipped, self.loss_scale, self.m_step, self.probe_step, self.param_round_step)
