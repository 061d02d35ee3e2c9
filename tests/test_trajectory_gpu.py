"""Trajectory parity on the GPU: every preconditioner family run for 200 steps (the large Kron layers: 30) through the public
functions, against the fp64 and the fp32 oracle on the identical stream of fp32 inputs (tests/trajectory_cases.py; what the cases
are, and that the fp32 oracle can follow them and a bias of 2e-7 per step cannot pass, is checked without a GPU by
tests/test_trajectory_cases_cpu.py).

At every checkpoint, for every state tensor and for the apply, drift = relative norm-wise distance from the fp64 run:
  1. drift_hip <= 1e-5;
  2. drift_hip <= K max(drift_fp32_oracle, 1e-7), K per family (trajectory_cases.K_FAMILY; the caps K <= 8 for UVd, sparse LU, dense
     and the small-layer Kron kernels and K <= 32 for the Kron routes on f16 x 2 operand planes are conditions);
  3. the fit measure |H P g - g| / |g| of the kernels' state within 1e-3 of the fp64 run's.
All violations of a case are collected and asserted at its end, so one run lists every figure.

Call patterns: UVd as update_precond_UVd_math_ + precond_grad_UVd_math at the checkpoints, and as the fused
update_precond_UVd_math_and_precond_grad on every step (the two states must end bit-identical); sparse LU and dense feed the pure
update's return value back in; Kron applies after every update, as an optimizer does, on the default apply route, and is also
compared after steps 1, 2 and 3 -- where a factor product cached from the previous step's factors would show.

Set PSGD_TRAJECTORY_PARITY_OUT to a file name to collect every measured drift and ratio (profiles/trajectory_parity.txt)."""
import os

import numpy as np
import pytest
import torch

from oracle import psgd_oracle_torch as oref
from tests import trajectory_cases as tc
from tests.uvd_cases import TINY32

pytestmark = pytest.mark.gpu

EARLY = (1, 2, 3)


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import preconditioned_stochastic_gradient_descent as m
    assert torch.cuda.is_available()
    return m


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Judge:
    """The bars at every checkpoint of one run of one case; prints and records every figure, collects the violations."""

    def __init__(self, case, route):
        self.case, self.route, self.bad = case, route, []

    def check(self, t, d_got, d_ref, fit_got, fit_64):
        for k, e in d_got.items():
            self._say("%s %s t=%d %s drift_hip=%.3e drift_fp32=%.3e ratio=%.2f"
                      % (self.case.id, self.route, t, k, e, d_ref[k], e / max(d_ref[k], tc.REF_FLOOR)))
        self._say("%s %s t=%d fit hip=%.6f fp64=%.6f" % (self.case.id, self.route, t, fit_got, fit_64))
        self.bad += ["%s t=%d %s" % (self.route, t, b) for b in tc.bars_failed(self.case, d_got, d_ref, fit_got, fit_64)]

    @staticmethod
    def _say(line):
        print(line)
        path = os.environ.get("PSGD_TRAJECTORY_PARITY_OUT")
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")


def _numpy_refs(case, record):
    """The problem, its input stream and the two oracle runs; the reference condition (fp32 oracle within 1e-5 of fp64) and, where
    the case claims it, the fit condition, before any kernel result is judged."""
    prob = tc.Problem(case)
    inputs = [prob.inputs(t) for t in range(case.T)]
    r64 = tc.run_oracle(case, prob, np.float64, record=record, inputs=inputs)
    r32 = tc.run_oracle(case, prob, np.float32, record=record, inputs=inputs)
    for t in record:
        for k, e in tc.drifts(case, r32[t], r64[t]).items():
            assert e <= tc.DRIFT_BAR, ("the fp32 oracle does not follow the fp64 oracle", case.id, t, k, e)
    if tc.FIT_MUST_IMPROVE(case):
        assert r64[case.T]["fit"] < r64[0]["fit"]
    return prob, inputs, r64, r32


def _judge_numpy(judge, prob, t, state, out, r64, r32):
    got = {"state": {k: x.cpu().numpy() for k, x in state.items()}, "apply": out.cpu().numpy()}
    judge.check(t, tc.drifts(judge.case, got, r64[t]), tc.drifts(judge.case, r32[t], r64[t]), prob.fit(got["apply"]), r64[t]["fit"])


# ------------------------------------------------------------------------------------------------ UVd
_uvd_final = {}        # case id -> {route: final state}: test_uvd leaves it for the bit-identity test


def _run_uvd(psgd, case, prob, inputs, route, on_checkpoint=None):
    g = _dev(prob.g)
    st = {k: _dev(a) for k, a in prob.state0.items()}
    for t in range(case.T):
        v, h = _dev(inputs[t][0]), _dev(inputs[t][1])
        kw = dict(balance=bool(prob.balance[t]), update_U=bool(prob.update_U[t]))
        if route == "fused":
            out = psgd.update_precond_UVd_math_and_precond_grad(st["U"], st["V"], st["d"], v, h, g, case.step, TINY32, **kw)
        else:
            assert psgd.update_precond_UVd_math_(st["U"], st["V"], st["d"], v, h, case.step, TINY32, **kw) is None
        if on_checkpoint is not None and t + 1 in case.checkpoints:
            if route == "two_calls":
                out = psgd.precond_grad_UVd_math(st["U"], st["V"], st["d"], g)
            on_checkpoint(t + 1, st, out)
    return st


@pytest.mark.parametrize("case", tc.UVD_CASES, ids=str)
def test_uvd(psgd, case):
    prob, inputs, r64, r32 = _numpy_refs(case, case.checkpoints)
    bad = []
    for route in ("two_calls", "fused"):
        judge = _Judge(case, route)
        final = _run_uvd(psgd, case, prob, inputs, route, lambda t, st, out: _judge_numpy(judge, prob, t, st, out, r64, r32))
        _uvd_final.setdefault(case.id, {})[route] = final
        bad += judge.bad
    assert not bad, (case.id, bad)


@pytest.mark.parametrize("case", tc.UVD_CASES, ids=str)
def test_uvd_fused_and_two_calls_end_bit_identical(psgd, case):
    """The state after case.T fused calls against the state after case.T update calls, bit for bit.  The fused call runs its own
    instantiations of the writing sweep and of the d step; the expressions that decide the stored state spell out their fused
    multiply-adds (uvd_kernels.h: uvd_qh, uvd_nabla, uvd_rank2, uvd_d_step), so every instantiation rounds alike.  Left to the
    compiler's contraction the two routes ended 9e-9 .. 1.2e-7 apart in U and V and 6e-8 .. 1.3e-6 in d at every rank to 64."""
    final = _uvd_final.get(case.id)
    if final is None:
        prob = tc.Problem(case)
        inputs = [prob.inputs(t) for t in range(case.T)]
        final = {route: _run_uvd(psgd, case, prob, inputs, route) for route in ("two_calls", "fused")}
    diff = {k: float((final["two_calls"][k] - final["fused"][k]).abs().max()) for k in tc.STATE_KEYS["uvd"]}
    print("%s two calls vs fused, max abs diff: %s" % (case.id, " ".join("%s=%.3e" % kv for kv in diff.items())))
    for k in tc.STATE_KEYS["uvd"]:
        assert torch.equal(final["two_calls"][k], final["fused"][k]), (case.id, k, diff)


# ------------------------------------------------------------------------------------------------ sparse LU, dense
@pytest.mark.parametrize("case", tc.SPLU_CASES, ids=str)
def test_splu(psgd, case):
    prob, inputs, r64, r32 = _numpy_refs(case, case.checkpoints)
    keys = tc.STATE_KEYS["splu"]
    g = _dev(prob.g)
    st = tuple(_dev(prob.state0[k]) for k in keys)
    judge = _Judge(case, "update")
    for t in range(case.T):
        st = psgd.update_precond_splu(*st, [_dev(inputs[t][0])], [_dev(inputs[t][1])], case.step)
        if t + 1 in case.checkpoints:
            out = psgd.precond_grad_splu(*st, [g])[0]
            _judge_numpy(judge, prob, t + 1, dict(zip(keys, st)), out, r64, r32)
    assert not judge.bad, (case.id, judge.bad)


@pytest.mark.parametrize("case", tc.DENSE_CASES, ids=str)
def test_dense(psgd, case):
    prob, inputs, r64, r32 = _numpy_refs(case, case.checkpoints)
    psgd.set_dense_route("native")
    g = _dev(prob.g)
    Q = _dev(prob.state0["Q"])
    judge = _Judge(case, "update")
    for t in range(case.T):
        Q = psgd.update_precond_dense(Q, [_dev(inputs[t][0])], [_dev(inputs[t][1])], step=case.step)
        if t + 1 in case.checkpoints:
            out = psgd.precond_grad_dense(Q, [g])[0]
            _judge_numpy(judge, prob, t + 1, {"Q": Q}, out, r64, r32)
    assert not judge.bad, (case.id, judge.bad)


# ------------------------------------------------------------------------------------------------ Kron, small-layer kernels
@pytest.mark.parametrize("case", tc.KRON_SMALL_CASES, ids=str)
def test_kron_small_layers(psgd, case):
    from psgd_tf_amd import kron
    assert kron._apply_route == "reference"
    record = EARLY + case.checkpoints
    prob, inputs, r64, r32 = _numpy_refs(case, record)
    g = _dev(prob.g)
    Ql, Qr = _dev(prob.state0["Ql"]), _dev(prob.state0["Qr"])
    judge = _Judge(case, "update+apply")
    for t in range(case.T):
        Ql, Qr = psgd.update_precond_kron(Ql, Qr, _dev(inputs[t][0]), _dev(inputs[t][1]), case.step)
        out = psgd.precond_grad_kron(Ql, Qr, g)                    # after every update, as an optimizer does
        if t + 1 in record:
            _judge_numpy(judge, prob, t + 1, {"Ql": Ql, "Qr": Qr}, out, r64, r32)
    assert not judge.bad, (case.id, judge.bad)


# ------------------------------------------------------------------------------------------------ Kron, plane and inverse routes
def _rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    d = torch.linalg.vector_norm(b)
    return float(torch.linalg.vector_norm(a - b) / (d if d > 0 else 1.0))


def _torch_refs(case, device):
    """The fp64 and fp32 runs of oracle/psgd_oracle_torch.py on `device` on one input stream: h = Hl dX Hr formed there in fp64 and
    rounded to fp32.  Returns the stream, g, the fit measure and {dtype: {t: (Ql, Qr, apply)}} for t = 0 (apply only) and the steps
    of EARLY and the checkpoints."""
    prob = tc.Problem(case)
    Hl, Hr = (torch.from_numpy(H).to(device) for H in (prob.Hl, prob.Hr))
    g = torch.from_numpy(prob.g).to(device)
    gnorm = torch.linalg.vector_norm(g.double())
    fit = lambda pg: float(torch.linalg.vector_norm(Hl @ pg.double() @ Hr - g.double()) / gnorm)
    stream = []
    for t in range(case.T):
        dX = torch.from_numpy(prob.draw(t)).to(device)
        stream.append((dX, (Hl @ dX.double() @ Hr).float()))
    record = EARLY + case.checkpoints
    runs = {}
    for dt in (torch.float64, torch.float32):
        Ql, Qr = (torch.from_numpy(prob.state0[k]).to(device, dt) for k in ("Ql", "Qr"))
        runs[dt] = {0: (None, None, oref.precond_grad_dense_dense(Ql, Qr, g.to(dt)))}
        for t, (dX, dG) in enumerate(stream):
            Ql, Qr = oref.update_precond_dense_dense(Ql, Qr, dX.to(dt), dG.to(dt), case.step, TINY32)
            if t + 1 in record:
                runs[dt][t + 1] = (Ql, Qr, oref.precond_grad_dense_dense(Ql, Qr, g.to(dt)))
    return stream, g, fit, record, runs


def _torch_drifts(got, ref64):
    return {"Ql": _rel(got[0], ref64[0]), "Qr": _rel(got[1], ref64[1]), "apply": _rel(got[2], ref64[2])}


def _assert_torch_reference_conditions(case, fit, record, runs):
    r64, r32 = runs[torch.float64], runs[torch.float32]
    for t in record:
        for k, e in _torch_drifts(r32[t], r64[t]).items():
            assert e <= tc.DRIFT_BAR, ("the fp32 reference does not follow the fp64 reference", case.id, t, k, e)
    first, last = fit(r64[0][2]), fit(r64[case.T][2])
    print("%s fp64 fit %.4f -> %.4f" % (case.id, first, last))
    assert last < first, (case.id, first, last)


@pytest.mark.parametrize("case", tc.KRON_DEVICE_CASES, ids=str)
def test_kron_plane_and_inverse_routes(psgd, case):
    from psgd_tf_amd import kron
    assert kron._apply_route == "reference"
    stream, g, fit, record, runs = _torch_refs(case, torch.device("cuda:0"))
    _assert_torch_reference_conditions(case, fit, record, runs)
    r64, r32 = runs[torch.float64], runs[torch.float32]
    M, N = case.shape
    Ql, Qr = torch.eye(M, device="cuda"), torch.eye(N, device="cuda")       # Problem.state0 of a Kron case
    judge = _Judge(case, "update+apply")
    for t, (dX, dG) in enumerate(stream):
        Ql, Qr = psgd.update_precond_kron(Ql, Qr, dX, dG, case.step)
        out = psgd.precond_grad_kron(Ql, Qr, g)
        if t + 1 in record:
            judge.check(t + 1, _torch_drifts((Ql, Qr, out), r64[t + 1]), _torch_drifts(r32[t + 1], r64[t + 1]),
                        fit(out), fit(r64[t + 1][2]))
    assert not judge.bad, (case.id, judge.bad)
    del stream, runs
    torch.cuda.empty_cache()
