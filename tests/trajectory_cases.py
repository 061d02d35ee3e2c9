"""Multi-step (trajectory) parity cases shared by tests/test_trajectory_cases_cpu.py and tests/test_trajectory_gpu.py.

Every single-call parity test of the suite holds a kernel to 1e-5 (state, apply) of the fp64 oracle after ONE call.  A preconditioner
is fitted over hundreds of calls, and an error of 1e-6 per call that always points the same way passes all of them and is 2e-4 off
after 200.  Here a preconditioner is run for T steps on a fixed stream of inputs, by three parties on identical fp32 inputs: the fp64
oracle (ground truth), the fp32 oracle (the yardstick: what plain fp32 arithmetic in the reference's op order drifts by) and the code
under test.  Nothing in this file needs a GPU.

  * Hessians with structure the preconditioner can learn.  Vector families (UVd, sparse LU, dense): H v = c .* v + W (W' v),
    c ~ LogUniform[1e-1, 1e1], W [N, k] ~ N(0,1) 3 / sqrt(N).  Kron: dG = Hl dX Hr, Hl = A A', A = O diag(exp(U(-1, 1))), O orthogonal.
  * Step t draws v (dx, dX) ~ N(0,1) in fp32; h = H v is formed in fp64 and rounded to fp32.
  * UVd's two coins come from a generator of their own (balance p = 0.01, update_U p = 0.5); if no step drew balance, step 37 does.
  * Checkpoints after 10, 50, 100, 200 steps: every state tensor and the apply on a fixed g of the case.

The bars of the GPU test (bars_failed), at every checkpoint, per state tensor and for the apply, drift = relative norm-wise distance
from the fp64 run:
  1. drift <= 1e-5 -- the suite's single-call bar, now held over the whole run;
  2. drift <= K max(drift_fp32_oracle, 1e-7), K per family (K_FAMILY), capped at 8 where the arithmetic is fp32 or better by design
     and at 32 for the Kron routes on f16 x 2 operand planes (about 22 bits: 4 times the rounding of fp32 per product);
  3. the fit measure |H P g - g| / |g| within 1e-3 (absolute) of the fp64 run's.
"""
import contextlib

import numpy as np

from oracle import psgd_oracle as orc
from tests.splu_cases import make_splu_problem
from tests.uvd_cases import TINY32, make_uvd_problem, rel_err

DRIFT_BAR = 1e-5
REF_FLOOR = 1e-7
FIT_BAR = 1e-3
BIAS = 2e-7                       # the teeth: one state tensor x (1 + BIAS) after every step
CHECKPOINTS = (10, 50, 100, 200)
FORCED_BALANCE_STEP = 37

# K of bar 2 per family: twice the largest drift / max(drift_fp32, 1e-7) measured on the MI355X (profiles/trajectory_parity.txt),
# rounded up to a whole number.  The caps are conditions, not measurements.
K_CAP = {"uvd": 8, "splu": 8, "dense": 8, "kron_small": 8, "kron_planes": 32}
# Largest measured ratios: UVd 1.46, sparse LU 1.41, dense 1.14, small-layer Kron 1.16, Kron planes and inverse route 1.02.
K_FAMILY = {"uvd": 3, "splu": 3, "dense": 3, "kron_small": 3, "kron_planes": 3}
assert all(K_FAMILY[f] <= K_CAP[f] for f in K_CAP)

STATE_KEYS = {"uvd": ("U", "V", "d"), "splu": ("L12", "l3", "U12", "u3"), "dense": ("Q",), "kron": ("Ql", "Qr")}
BIASED = {"uvd": "d", "splu": "l3", "dense": "Q", "kron": "Ql"}


class Case:
    """One trajectory: kind (uvd | splu | dense | kron), the family whose K applies, the shape (N, r) / (N,) / (M, N), the step,
    the number of steps and the checkpoints.  ref: "numpy" (oracle/psgd_oracle.py on the host) or "torch" (oracle/psgd_oracle_torch.py
    on the device, GPU test only).  The seed depends on nothing but the shape."""

    def __init__(self, kind, family, shape, step, T=200, checkpoints=CHECKPOINTS, ref="numpy", init=None):
        self.kind, self.family, self.shape, self.step, self.T, self.ref, self.init = kind, family, tuple(shape), step, T, ref, init
        self.checkpoints = tuple(c for c in checkpoints if c <= T)
        self.seed = sum(s * m for s, m in zip(self.shape, (1, 100003))) + 17
        self.id = "%s-%s-step%g%s" % (kind, "x".join(str(s) for s in self.shape), step, "-" + init if init else "")

    def __repr__(self):
        return self.id


def _uvd(N, r, steps=(0.01, 0.1)):
    return [Case("uvd", "uvd", (N, r), s) for s in steps]


UVD_CASES = (_uvd(2049, 10) + _uvd(1021, 32) + _uvd(4099, 4) + _uvd(63, 20)            # ranks to 32
             + _uvd(1021, 41, (0.01,)) + _uvd(2049, 64, (0.01,))                       # whole-matrix ranks 33 .. 64
             + _uvd(1021, 70, (0.01,)))                                                # column chunks
SPLU_CASES = [Case("splu", "splu", s, 0.01, init=i) for s in ((2049, 10), (1021, 41), (140, 70)) for i in ("demo", "generic")]
DENSE_CASES = [Case("dense", "dense", (n,), 0.01) for n in (64, 65, 257)]              # the 64 / 65 route switch, a 256-column edge
KRON_SMALL_CASES = [Case("kron", "kron_small", s, 0.01) for s in ((33, 129), (85, 10), (151, 16))]
# the plane routes and the solves through explicit inverses: references on the device, 30 steps
KRON_DEVICE_CASES = [Case("kron", "kron_planes", s, 0.01, T=30, checkpoints=(10, 30), ref="torch")
                     for s in ((600, 300), (513, 384), (1024, 2048))]
NUMPY_CASES = UVD_CASES + SPLU_CASES + DENSE_CASES + KRON_SMALL_CASES
ALL_CASES = NUMPY_CASES + KRON_DEVICE_CASES
# the demo-initialised sparse LU barely moves at step 0.01 (its fit measure stays at 1.000): a drift case only
FIT_MUST_IMPROVE = lambda case: not (case.kind == "splu" and case.init == "demo")


# ------------------------------------------------------------------------------------------------ problems
class Problem:
    """The fixed part of a case: the Hessian, the initial state and g (fp32 NumPy arrays), and the input stream."""

    def __init__(self, case):
        self.case = case
        rng = np.random.default_rng(case.seed)
        if case.kind == "kron":
            M, N = case.shape
            self.Hl, self.Hr = _spd(rng, M), _spd(rng, N)
            self.state0 = {"Ql": np.eye(M, dtype=np.float32), "Qr": np.eye(N, dtype=np.float32)}
            self.g = rng.standard_normal((M, N)).astype(np.float32)
            return
        N = case.shape[0]
        k = max(1, case.shape[1] // 2) if case.kind == "uvd" else 4
        self.c = np.exp(rng.uniform(np.log(1e-1), np.log(1e1), (N, 1)))
        self.W = rng.standard_normal((N, k)) * (3.0 / np.sqrt(N))
        if case.kind == "uvd":
            p = make_uvd_problem(N, case.shape[1], seed=case.seed)                     # U, V ~ (N r)^-1/2, d = 1: the class's start
            self.state0 = {key: p[key] for key in ("U", "V", "d")}
            self.g = p["g"]
            coins = np.random.default_rng(case.seed + 1).uniform(size=(case.T, 2))
            self.balance = coins[:, 0] < 0.01
            if not self.balance.any() and case.T > FORCED_BALANCE_STEP:
                self.balance[FORCED_BALANCE_STEP] = True
            self.update_U = coins[:, 1] < 0.5
        elif case.kind == "splu":
            p = make_splu_problem(N, case.shape[1], seed=case.seed, init_like_demo=(case.init == "demo"))
            self.state0 = {key: p[key] for key in ("L12", "l3", "U12", "u3")}
            self.g = p["g"]
        else:
            self.state0 = {"Q": (0.3 * np.eye(N)).astype(np.float32)}
            self.g = rng.standard_normal((N, 1)).astype(np.float32)

    def hess(self, x):
        """H x in fp64 (x: fp64, a column for the vector families, [M, N] for Kron)"""
        if self.case.kind == "kron":
            return self.Hl @ x @ self.Hr
        return self.c * x + self.W @ (self.W.T @ x)

    def draw(self, t):
        """v (dx, dX) of step t (0-based): N(0,1) in fp32"""
        rng = np.random.default_rng([self.case.seed, t])
        shape = self.case.shape if self.case.kind == "kron" else (self.case.shape[0], 1)
        return rng.standard_normal(shape, dtype=np.float32)

    def inputs(self, t):
        """(v, h) of step t: h = H v formed in fp64 and rounded to fp32"""
        v = self.draw(t)
        return v, self.hess(v.astype(np.float64)).astype(np.float32)

    def fit(self, pg):
        """|H pg - g| / |g| in fp64, pg = P g as some party computed it"""
        g = self.g.astype(np.float64)
        return float(np.linalg.norm(self.hess(np.asarray(pg, dtype=np.float64).reshape(g.shape)) - g) / np.linalg.norm(g))


def _spd(rng, n):
    """A A' with A = O diag(exp(U(-1, 1))), O the orthogonal factor of a Gaussian matrix (fp64)"""
    O = np.linalg.qr(rng.standard_normal((n, n)))[0]
    A = O * np.exp(rng.uniform(-1.0, 1.0, n))[None, :]
    return A @ A.T


# ------------------------------------------------------------------------------------------------ the NumPy oracle as a party
def _one_blas_thread():
    """The matrices here are small (a few hundred rows at the most) and every step is a chain of short BLAS calls: a BLAS thread pool
    sized for the whole machine spends 50 times the arithmetic on waking and joining its threads.  One thread, where threadpoolctl is
    there to say so; the results do not depend on it being there."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api="blas")


def oracle_step(case, prob, state, t, v, h):
    """One update of `state` (a dict of arrays of one dtype) in that dtype; returns the new state dict."""
    dt = state[STATE_KEYS[case.kind][0]].dtype
    v, h = v.astype(dt), h.astype(dt)
    if case.kind == "uvd":
        s = {k: a.copy() for k, a in state.items()}
        orc.update_precond_UVd_math_(s["U"], s["V"], s["d"], v, h, case.step, TINY32, balance=bool(prob.balance[t]),
                                     update_U=bool(prob.update_U[t]))
        return s
    if case.kind == "splu":
        return dict(zip(STATE_KEYS["splu"], orc.update_precond_splu(state["L12"], state["l3"], state["U12"], state["u3"], [v], [h], case.step)))
    if case.kind == "dense":
        return {"Q": orc.update_precond_dense(state["Q"], [v], [h], case.step)}
    return dict(zip(STATE_KEYS["kron"], orc.update_precond_kron(state["Ql"], state["Qr"], v, h, case.step)))


def oracle_apply(case, state, g):
    dt = state[STATE_KEYS[case.kind][0]].dtype
    g = g.astype(dt)
    if case.kind == "uvd":
        return orc.precond_grad_UVd_math(state["U"], state["V"], state["d"], g)
    if case.kind == "splu":
        return orc.precond_grad_splu(state["L12"], state["l3"], state["U12"], state["u3"], [g])[0]
    if case.kind == "dense":
        return orc.precond_grad_dense(state["Q"], [g])[0]
    return orc.precond_grad_kron(state["Ql"], state["Qr"], g)


def run_oracle(case, prob, dtype, bias=0.0, record=None, inputs=None):
    """The oracle in `dtype` for case.T steps.  Returns {t: {"state": {...}, "apply": array, "fit": float}} for t = 0 (apply and fit
    only) and every t of `record` (default: the checkpoints).  bias: BIASED[kind] is multiplied by (1 + bias) after every step.
    inputs: a list of the (v, h) of every step, to share one drawn stream between several runs."""
    with _one_blas_thread():
        return _run_oracle(case, prob, dtype, bias, case.checkpoints if record is None else record, inputs)


def _run_oracle(case, prob, dtype, bias, record, inputs):
    state = {k: a.astype(dtype) for k, a in prob.state0.items()}
    pg = oracle_apply(case, state, prob.g)
    out = {0: {"apply": pg, "fit": prob.fit(pg)}}
    for t in range(case.T):
        v, h = inputs[t] if inputs is not None else prob.inputs(t)
        state = oracle_step(case, prob, state, t, v, h)
        if bias:
            key = BIASED[case.kind]
            state[key] = state[key] * state[key].dtype.type(1.0 + bias)
        if t + 1 in record:
            pg = oracle_apply(case, state, prob.g)
            out[t + 1] = {"state": {k: a.copy() for k, a in state.items()}, "apply": pg, "fit": prob.fit(pg)}
    return out


# ------------------------------------------------------------------------------------------------ drift and the bars
def drifts(case, got, ref64):
    """{tensor name or "apply": relative norm-wise distance of `got` from the fp64 run} at one checkpoint"""
    d = {k: rel_err(got["state"][k], ref64["state"][k]) for k in STATE_KEYS[case.kind]}
    d["apply"] = rel_err(got["apply"], ref64["apply"])
    return d


def bars_failed(case, d_got, d_ref, fit_got, fit_64):
    """The bars of the module docstring at one checkpoint; returns the list of violations (empty: all bars hold)."""
    K = K_FAMILY[case.family]
    bad = []
    for k, e in d_got.items():
        if not e <= DRIFT_BAR:
            bad.append("%s: drift %.2e > %.0e" % (k, e, DRIFT_BAR))
        lim = K * max(d_ref[k], REF_FLOOR)
        if not e <= lim:
            bad.append("%s: drift %.2e > %d x max(fp32 oracle %.2e, %.0e)" % (k, e, K, d_ref[k], REF_FLOOR))
    if not abs(fit_got - fit_64) <= FIT_BAR:
        bad.append("fit %.6f against %.6f" % (fit_got, fit_64))
    return bad
