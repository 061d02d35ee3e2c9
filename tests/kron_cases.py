"""Shared Kron test data: ill-conditioned triangular factors (tests/test_kron_gpu.py, tests/test_kron_routes_gpu.py)."""
import numpy as np


def illcond_factor(rng, n, cond=1e4):
    """An upper-triangular factor with cond(Q) ~ `cond`: its diagonal spread log-evenly over [1/cond, 1] in random order, a dense
    upper triangle scaled column by column with the diagonal (NumPy, fp64)."""
    d = np.exp(np.linspace(0.0, -np.log(cond), n))
    rng.shuffle(d)
    return np.triu(rng.standard_normal((n, n)) * (0.3 / n ** 0.5), 1) * d[None, :] + np.diag(d)
