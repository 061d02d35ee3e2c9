"""Shared data of the vector-layer tests (tests/test_kron_any_rank_cpu.py, tests/test_multi_vec_gpu.py, tests/test_kron_any_rank_gpu.py):
the input families, the three-phase restatement of the kernel's specification in NumPy, and the error measures.

A vector of length n is the reference's layer of shape [1, n] in the (dense, scaling) format: Ql = [[ql]], qr = [1, n]
(psgd.py:276-322).  Everything here is made once per key and handed out as read-only arrays."""
import numpy as np

from oracle import psgd_oracle as orc

# the edges of a lane's 4-wide access, of the wave, of the workgroup, and several trips per thread
LENGTHS = (2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 70001)
STATES = ("random", "fresh", "chained")
STEP = float(np.float32(0.05))
TINY32 = float(np.finfo(np.float32).tiny)
BAR_FACTORS, BAR_INCREMENT, BAR_APPLY = 1e-5, 2e-3, 1e-5          # the project's bars for Kron (tests/test_kron_gpu.py)


def three_phase(ql, qr, dx, dg, step, tiny):
    """The specification of psgd_multi_vec_update_f32 in the dtype of its inputs: ql a scalar, qr / dx / dg arrays of n elements.
    Returns (new ql, new qr)."""
    dt = qr.dtype.type
    ql, step, tiny = dt(ql), dt(step), dt(tiny)
    rho = np.sqrt(ql / np.max(qr))                                  # phase 1
    qlp = ql / rho
    qrp = rho * qr
    A = (qlp * dg) * qrp                                            # phase 2
    Bt = (dx / qlp) * (dt(1.0) / qrp)
    a2, b2 = A * A, Bt * Bt
    grad1 = np.sum(a2) - np.sum(b2)
    grad2 = a2 - b2
    step1 = step / (np.abs(grad1) + tiny)                           # phase 3
    step2 = step / (np.max(np.abs(grad2)) + tiny)
    return qlp - (step1 * grad1) * qlp, qrp - (step2 * grad2) * qrp


def apply_formula(ql, qr, g):
    dt = qr.dtype.type
    ql = dt(ql)
    return ((ql * ql) * g) * (qr * qr)


def oracle_update(ql, qr, dx, dg, step, dtype=np.float64):
    """oracle.update_precond_kron on the [1, n] view in `dtype`: (new ql as a scalar, new qr of n elements)"""
    f = lambda a: np.asarray(a, dtype=dtype).reshape(1, -1)
    Ql, Qr = orc.update_precond_kron(np.full((1, 1), ql, dtype=dtype), f(qr), f(dx), f(dg), step)
    assert Ql.shape == (1, 1) and Qr.shape == (1, np.size(qr))
    return Ql[0, 0], Qr[0]


def oracle_apply(ql, qr, g, dtype=np.float64):
    f = lambda a: np.asarray(a, dtype=dtype).reshape(1, -1)
    return orc.precond_grad_kron(np.full((1, 1), ql, dtype=dtype), f(qr), f(g))[0]


_cases = {}


def case(n, state, seed=0):
    """(ql, qr, dx, dg, g): float32 values of one vector of length n in one of the factor states
        random    qr = exp(U(-1.6, 1.6)), ql in 0.1 .. 10
        fresh     ql = 1, qr = 1
        chained   the state after 20 chained fp64 oracle updates from fresh (then rounded to float32)
    dx is standard normal; dg = h * dx + 0.1 noise with a positive diagonal h = exp(U(-1, 1)), so that the pair looks like
    (v, Hv) of a well-posed problem and P = Q'Q has something to converge to."""
    key = (n, state, seed)
    if key not in _cases:
        rng = np.random.default_rng([n, STATES.index(state), seed])
        h = np.exp(rng.uniform(-1.0, 1.0, n))
        pair = lambda: (lambda dx: (dx, h * dx + 0.1 * rng.standard_normal(n)))(rng.standard_normal(n))
        if state == "random":
            ql, qr = float(np.exp(rng.uniform(np.log(0.1), np.log(10.0)))), np.exp(rng.uniform(-1.6, 1.6, n))
        else:
            ql, qr = 1.0, np.ones(n)
            if state == "chained":
                for _ in range(20):
                    dx, dg = pair()
                    ql, qr = oracle_update(ql, qr, dx, dg, STEP)
        dx, dg = pair()
        g = rng.standard_normal(n)
        out = tuple(np.asarray(a, dtype=np.float32) for a in (ql, qr, dx, dg, g))
        for a in out:
            a.setflags(write=False)
        _cases[key] = out
    return _cases[key]


def rel(a, b):
    """norm-wise relative error of a against the fp64 value b"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def update_errors(new_ql, new_qr, ql, qr, dx, dg, step=STEP):
    """(factor error, increment error) of an fp32 result against the fp64 oracle on the same float32 inputs, each the larger of the
    error of ql and that of qr (relative, norm-wise), as tests/test_kron_gpu.py takes them per factor"""
    ref_ql, ref_qr = oracle_update(ql, qr, dx, dg, step)
    new_qr, qr = np.asarray(new_qr, dtype=np.float64), np.asarray(qr, dtype=np.float64)
    new_ql, ql = np.float64(new_ql), np.float64(ql)
    return (max(rel(new_ql, ref_ql), rel(new_qr, ref_qr)),
            max(rel(new_ql - ql, ref_ql - ql), rel(new_qr - qr, ref_qr - qr)))
