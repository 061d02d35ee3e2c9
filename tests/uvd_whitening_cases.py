"""The convergence case of UVd(preconditioner_fit="whitening"), shared by tests/test_uvd_whitening_cpu.py (the oracle alone, which
sets the level) and tests/test_uvd_whitening_gpu.py (class UVd on the same inputs, held to that level and to the oracle's path).

N = 256, r = 4.  Step t feeds the gradient g_t = sigma .* z_t, sigma = 0.1 on the first half and 10 on the second, z_t the
counter_randn stream of Z_SEED at index0 = t N, and the probe v_t = counter_randn(uvd_step_rounding_seed(PROBE_SEED, t), 0, N): what
class UVd draws with probe_seed=PROBE_SEED.  The coins of psgd.py:703, :562, :588 are those of a CPU torch.Generator seeded with
COIN_SEED, drawn in the class's order.  The whitening level is the ratio of the mean of (P g)^2 over the second half to the mean
over the first half, on SAMPLES fresh gradients (the stream of EVAL_SEED): 1e4 for P = I, 1 for the whitening P = diag(1 / sigma).
"""
import numpy as np
import torch

from oracle import psgd_oracle as orc

N, R = 256, 4
# Chosen on the CPU with the fp64 and the fp32 oracle: at lr 0.2 the ratio is 1.930 after 2000 steps (the cap) and the fp32 oracle is
# still within 7.9e-6 of the fp64 one.  Larger rates get there sooner (0.4: 1.905 after 1200 steps, 0.5: 1.636) but the fp32 oracle
# has then left the fp64 path by more than 1e-5 (1.6e-5, 2.1e-4): no fp32 run could be held to the trajectory bars.
STEPS, LR_PRECOND = 2000, 0.2
LEVEL = 2.0                                # the ratio the oracle must reach, and then the kernels
SAMPLES = 64
PROBE_SEED, Z_SEED, EVAL_SEED, COIN_SEED, STATE_SEED = 0x5EED, 0xD47A, 0xE7A1, 77, 2026
TINY32 = float(np.finfo(np.float32).tiny)
SIGMA = np.concatenate([np.full(N // 2, 0.1), np.full(N // 2, 10.0)]).astype(np.float32)


def _psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def gradient(t):
    """g_t, float32 [N]: the product of two float32 values, rounded once"""
    return SIGMA * _psgd().counter_randn(Z_SEED, t * N, N)


def probe(t):
    m = _psgd()
    return m.counter_randn(m.uvd_step_rounding_seed(PROBE_SEED, t), 0, N)


def coins(steps):
    """[(balance, update_U)] of the first `steps` updating steps of UVd(..., preconditioner_update_probability=1,
    generator=torch.Generator().manual_seed(COIN_SEED)): per step the coin of :703, then :562 (p = 0.01), then :588 (p = 0.5)"""
    gen = torch.Generator().manual_seed(COIN_SEED)
    out = []
    for _ in range(steps):
        torch.rand((), generator=gen)
        out.append((bool(torch.rand((), generator=gen).item() < 0.01), bool(torch.rand((), generator=gen).item() < 0.5)))
    return out


def initial_state(dtype=np.float64):
    """psgd.py:687-690 with a numpy generator: U, V ~ N(0, 1) / sqrt(N r) as float32 values, d = 1"""
    rng = np.random.default_rng(STATE_SEED)
    sc = np.float32((1.0 / (N * R)) ** 0.5)
    U, V = (rng.standard_normal((N, R), dtype=np.float32) * sc for _ in range(2))
    return U.astype(dtype), V.astype(dtype), np.ones((N, 1), dtype=dtype)


def oracle_run(steps, lr=LR_PRECOND, dtype=np.float64, keep=()):
    """the oracle's trajectory in `dtype`: (U, V, d) after `steps` steps, and {t: (U, V, d) copies} for the t in keep"""
    U, V, d = initial_state(dtype)
    kept = {}
    for t, (bal, upd) in enumerate(coins(steps)):
        v, g = probe(t).astype(dtype)[:, None], gradient(t).astype(dtype)[:, None]
        orc.update_precond_UVd_math_(U, V, d, v, g, float(np.float32(lr)), TINY32, balance=bal, update_U=upd)
        if t + 1 in keep:
            kept[t + 1] = (U.copy(), V.copy(), d.copy())
    return (U, V, d), kept


def variance_ratio(U, V, d):
    """mean((P g)^2) over the second half / over the first half, on SAMPLES fresh gradients, in float64"""
    U, V, d = (np.asarray(x, dtype=np.float64) for x in (U, V, d))
    z = _psgd().counter_randn(EVAL_SEED, 0, SAMPLES * N).astype(np.float64).reshape(SAMPLES, N).T
    pg = orc.precond_grad_UVd_math(U, V, d.reshape(N, 1), SIGMA.astype(np.float64)[:, None] * z)
    return float(np.mean(pg[N // 2:] ** 2) / np.mean(pg[:N // 2] ** 2))
