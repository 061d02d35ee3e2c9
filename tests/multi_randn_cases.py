"""What the CPU and the GPU tests of the counter-based probe vectors share (tests/test_multi_randn_cpu.py,
tests/test_multi_randn_gpu.py): the fixed stream of the moment tests and its bounds; and reference(), the CPU restatement of a
stream computed once, which tests/flat_step_cases.py feeds to its model as the whitening probe."""
import numpy as np

MOMENT_SEED, MOMENT_N = 20261020, 2 ** 20              # the stream of the moment tests, here and on the GPU


def moment_figures(z):
    """{name: (value, bound)} of n draws; every bound is five standard errors of the statistic under N(0, 1), except the
    largest magnitude, which is sqrt(-2 ln 2^-32) = 6.66, the largest radius the construction can give"""
    z = np.asarray(z, dtype=np.float64)
    n = z.size
    return {"mean": (abs(z.mean()), 5.0 / np.sqrt(n)),
            "variance": (abs(z.var() - 1.0), 5.0 * np.sqrt(2.0 / n)),
            "pair correlation": (abs(np.corrcoef(z[0::2], z[1::2])[0, 1]), 5.0 / np.sqrt(n / 2)),
            "third moment": (abs((z ** 3).mean()), 5.0 * np.sqrt(15.0 / n)),
            "max |z|": (np.abs(z).max(), 6.67)}


_want = {}


def reference(psgd, seed, index0, n):
    """counter_randn at scale 1, computed once per stream and shared"""
    key = (seed, index0, n)
    if key not in _want:
        _want[key] = psgd.counter_randn(seed, index0, n)
    return _want[key]
