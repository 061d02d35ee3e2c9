"""Shared data and the fp64 restatement of class Kron's step (tests/test_kron_class_cpu.py, tests/test_kron_class_gpu.py).

The restatement is NumPy fp64 on top of the oracle's update_precond_kron / precond_grad_kron: steps 1-7 of Kron.step with the coin
and the probe vectors handed in, so that a GPU run and the restatement can be fed the same draws."""
import numpy as np

from oracle import psgd_oracle as orc

LENET5 = [(26, 6), (151, 16), (257, 120), (121, 84), (85, 10)]          # W1 .. W5 of mnist_with_lenet5.py:12-16
SPARSE = [((16, 40), ("dense", "norm")), ((40, 16), ("dense", "scale")), ((16, 40), ("norm", "dense")),
          ((40, 16), ("norm", "scale")), ((16, 40), ("scale", "dense")), ((40, 16), ("scale", "norm"))]
TINY32 = float(np.finfo(np.float32).tiny)
DELTA32 = float(np.float32(np.sqrt(np.float32(np.finfo(np.float32).eps))))


def spd(n, rng, spread=1.0):
    """a symmetric positive definite n x n matrix whose entries are float32 values (held in fp64)"""
    d = np.exp(rng.uniform(-spread, spread, n))
    B = rng.standard_normal((n, n)) * (0.1 / n ** 0.5)
    H = np.diag(d) + B @ B.T
    H = 0.5 * (H + H.T)
    return H.astype(np.float32).astype(np.float64)


def quadratic_problem(shapes, seed, scale=0.5):
    """loss = sum_k tr(W_k' Hl_k W_k Hr_k) / 2: (Ws, Hls, Hrs), all fp64 arrays of float32 values"""
    rng = np.random.default_rng(seed)
    Ws = [(rng.standard_normal(s) * scale).astype(np.float32).astype(np.float64) for s in shapes]
    return Ws, [spd(s[0], rng) for s in shapes], [spd(s[1], rng) for s in shapes]


def quadratic_loss(Ws, Hls, Hrs):
    return float(sum(0.5 * np.sum(W * (Hl @ W @ Hr)) for W, Hl, Hr in zip(Ws, Hls, Hrs)))


def quadratic_grads(Ws, Hls, Hrs):
    return [Hl @ W @ Hr for W, Hl, Hr in zip(Ws, Hls, Hrs)]


def initial_factors(shape, pair, init_scale=1.0):
    """demo_usage_of_all_preconditioners.py:68-78 in fp64; the left factor times init_scale"""
    def one(side, n):
        if side == "dense":
            return np.eye(n)
        if side == "scale":
            return np.ones((1, n))
        return np.stack([np.ones(n), np.zeros(n)])
    return [one(pair[0], shape[0]) * init_scale, one(pair[1], shape[1])]


def kron_step_f64(Ws, Qs, grad_fn, hvp_fn, vs, *, lr_params, lr_preconditioner, max_norm=None, update=True, exact=True):
    """Steps 2-7 of Kron.step in fp64.  grad_fn(Ws) -> gradients; hvp_fn(vs) -> Hessian-vector products (exact route);
    vs: the probe vectors as drawn (on the finite-difference route already multiplied by delta).
    Returns (new Ws, new Qs, preconditioned gradients, lr_eff)."""
    grads = grad_fn(Ws)
    undo = None
    if update:
        if exact:
            dXs, dGs = vs, hvp_fn(vs)
        else:
            perturbed = grad_fn([W + v for W, v in zip(Ws, vs)])
            dGs = [(pg - g) / DELTA32 for pg, g in zip(perturbed, grads)]
            dXs = [v / DELTA32 for v in vs]
            undo = vs
        Qs = [list(orc.update_precond_kron(q[0], q[1], dX, dG, lr_preconditioner)) for q, dX, dG in zip(Qs, dXs, dGs)]
    pre = [orc.precond_grad_kron(q[0], q[1], g) for q, g in zip(Qs, grads)]
    lr_eff = lr_params
    if max_norm is not None:
        S = sum(float(np.sum(g * g)) for g in pre)
        lr_eff = lr_params * min(max_norm / (np.sqrt(S) + TINY32), 1.0)
    if undo is None:                      # (on the finite-difference route W here is the unperturbed parameter: W + v - (lr pg + v))
        new = [W - lr_eff * g for W, g in zip(Ws, pre)]
    else:
        new = [(W + v) - (lr_eff * g + v) for W, g, v in zip(Ws, pre, undo)]
    return new, Qs, pre, lr_eff


def rel(a, b):
    """norm-wise relative error of a against the fp64 value b"""
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300))
