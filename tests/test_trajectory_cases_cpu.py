"""The trajectory cases of tests/trajectory_cases.py without a GPU: the yardstick is sound and the bars have teeth.

For every case whose references are the NumPy oracle, three runs on one input stream: fp64, fp32, and fp32 with one state tensor
multiplied by (1 + 2e-7) after every step.
  * Reference condition: the fp32 oracle stays within 1e-5 of the fp64 oracle at every checkpoint, on every state tensor and on the
    apply.  A condition on the inputs: a trajectory that plain fp32 cannot follow compares nothing.
  * Fit condition: the fp64 oracle's |H P g - g| / |g| at the last checkpoint is below its value before the first step (the
    preconditioner learns something), except from the demo state of the sparse LU, which barely moves at step 0.01.
  * Teeth: the biased run -- a relative error of 2e-7 per step, 50 times below every single-call bar of the suite -- fails the bars
    that tests/test_trajectory_gpu.py holds the kernels to, at the last checkpoint.
"""
import functools

import numpy as np
import pytest

from tests import trajectory_cases as tc

_BY_ID = {c.id: c for c in tc.NUMPY_CASES}
IDS = sorted(_BY_ID)


@functools.lru_cache(maxsize=None)
def _runs(case_id):
    case = _BY_ID[case_id]
    prob = tc.Problem(case)
    inputs = [prob.inputs(t) for t in range(case.T)]
    r64 = tc.run_oracle(case, prob, np.float64, inputs=inputs)
    r32 = tc.run_oracle(case, prob, np.float32, inputs=inputs)
    last = (case.checkpoints[-1],)
    biased = tc.run_oracle(case, prob, np.float32, bias=tc.BIAS, record=last, inputs=inputs)
    return case, r64, r32, biased


def test_case_table():
    """ids are unique, seeds depend on the shape alone, every UVd schedule has a balance step and both branches"""
    assert len(_BY_ID) == len(tc.NUMPY_CASES) and len({c.id for c in tc.ALL_CASES}) == len(tc.ALL_CASES)
    for c in tc.ALL_CASES:
        assert c.checkpoints and c.checkpoints[-1] == c.T
        assert all(o.seed == c.seed for o in tc.ALL_CASES if o.shape == c.shape)
        assert tc.K_FAMILY[c.family] <= tc.K_CAP[c.family]
    for c in tc.UVD_CASES:
        p = tc.Problem(c)
        assert p.balance.any() and p.update_U.any() and not p.update_U.all()
    assert tc.K_CAP == {"uvd": 8, "splu": 8, "dense": 8, "kron_small": 8, "kron_planes": 32}
    assert (tc.DRIFT_BAR, tc.REF_FLOOR, tc.FIT_BAR, tc.BIAS) == (1e-5, 1e-7, 1e-3, 2e-7)


def test_input_stream_is_deterministic():
    c = _BY_ID["uvd-63x20-step0.01"]
    a, b = tc.Problem(c), tc.Problem(c)
    for t in (0, 5):
        for x, y in zip(a.inputs(t), b.inputs(t)):
            assert x.dtype == np.float32 and np.array_equal(x, y)
    assert not np.array_equal(a.inputs(0)[0], a.inputs(1)[0])
    v, h = a.inputs(3)
    assert np.array_equal(h, a.hess(v.astype(np.float64)).astype(np.float32))


@pytest.mark.parametrize("case_id", IDS)
def test_fp32_oracle_follows_fp64(case_id):
    case, r64, r32, _ = _runs(case_id)
    for t in case.checkpoints:
        d = tc.drifts(case, r32[t], r64[t])
        print("%s t=%d fp32 drift %s fit %.4f" % (case.id, t, " ".join("%s=%.2e" % kv for kv in d.items()), r64[t]["fit"]))
        for k, e in d.items():
            assert np.isfinite(e) and e <= tc.DRIFT_BAR, (case.id, t, k, e)


@pytest.mark.parametrize("case_id", [i for i in IDS if tc.FIT_MUST_IMPROVE(_BY_ID[i])])
def test_fp64_fit_improves(case_id):
    case, r64, _, _ = _runs(case_id)
    first, last = r64[0]["fit"], r64[case.checkpoints[-1]]["fit"]
    print("%s fit %.4f -> %.4f" % (case.id, first, last))
    assert last < first, (case.id, first, last)


@pytest.mark.parametrize("case_id", IDS)
def test_a_bias_of_2e_7_per_step_fails_the_bars(case_id):
    case, r64, r32, biased = _runs(case_id)
    t = case.checkpoints[-1]
    d_ref = tc.drifts(case, r32[t], r64[t])
    d_bad = tc.drifts(case, biased[t], r64[t])
    bad = tc.bars_failed(case, d_bad, d_ref, biased[t]["fit"], r64[t]["fit"])
    print("%s biased drift %s" % (case.id, " ".join("%s=%.2e" % kv for kv in d_bad.items())))
    assert bad, (case.id, d_bad, d_ref)
    # ... and the unbiased fp32 run passes them: the bars separate the two
    assert not tc.bars_failed(case, d_ref, d_ref, r32[t]["fit"], r64[t]["fit"])
