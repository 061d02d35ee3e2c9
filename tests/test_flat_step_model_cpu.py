"""The float64 step model of tests/flat_step_model.py without a GPU: it agrees with what the suite already has (orc.uvd_step, the
momentum and loss-scale schedules of the package), the bars that tests/flat_step_cases.py derives have teeth (eight mutants of the
model, each put in the class's place under the GPU test's own comparison and bars, fail), and the conditions on low-precision
parameters can be met (the float32 run of the model meets them on every low-precision case of the grid)."""
import numpy as np
import pytest

from oracle import psgd_oracle as orc
from tests import flat_step_cases as fc
from tests import flat_step_model as fm


# ------------------------------------------------------------------------------------------ agreement with what exists
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fd"])
@pytest.mark.parametrize("update", [True, False], ids=["update", "no-update"])
def test_features_off_reproduces_the_uvd_step_oracle(exact, update):
    key = fc.Key("UVd-r3", "N117", "exact" if exact else "fd", "fp32", "off")
    state = fc.standin_state(key)
    model = fc.make_model(key, state, None)
    params, draws = fc.initial_params(key), fc.problem(key.set)[2][0]
    out = model.step(params, update, draws=draws, branches=(False, True))
    grad, hess = fc.loss_functions(key.set)
    r32 = lambda x: fm.round_to(x, "float32")
    grads = [r32(grad(i, w)) for i, w in enumerate(params)]
    U, V, d = (s.astype(np.float64) for s in state)
    tiny, delta = fm.tiny_of("float32"), float(orc.delta_param_scale_of(np.float32))
    if not update:
        want = orc.uvd_step(params, grads, None, None, U, V, d, fc.LR, fc.LR_Q, np.inf, tiny, update_Q=False)
    elif exact:
        vs = [r32(z) for z in draws]
        Hvs = [r32(hess(i, w) * v) for i, (w, v) in enumerate(zip(params, vs))]
        want = orc.uvd_step(params, grads, Hvs, vs, U, V, d, fc.LR, fc.LR_Q, np.inf, tiny)
    else:
        vs = [r32(np.float32(z) * np.float32(delta)) for z in draws]
        moved = [r32(w + v) for w, v in zip(params, vs)]
        Hvs = [r32(r32(grad(i, w)) - g) for i, (w, g) in enumerate(zip(moved, grads))]
        want = orc.uvd_step(moved, grads, Hvs, vs, U, V, d, fc.LR, fc.LR_Q, np.inf, tiny, exact=False, delta_param_scale=delta)
    for got, ref in zip(out["x"], want):
        assert fc.rel_err(got, ref) <= 1e-12
    for got, ref in zip(model.state, (U, V, d)):
        assert fc.rel_err(got, ref) <= 1e-12


def test_schedules_agree_with_the_package():
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl
    for k in range(0, 40):
        for momentum in (0.0, 0.3, 0.5, 0.9, 0.99, 0.999):
            assert fm.momentum_coefficients(k, momentum) == impl.uvd_momentum_coefficients(k, momentum), (k, momentum)
    for scale in (1.0, 2.0, 2.0 ** 10, 2.0 ** 16, 2.0 ** 23, 2.0 ** 24):
        for good in range(0, 4):
            for skipped in (False, True):
                for interval in (1, 2, 3, 2000):
                    assert fm.loss_scale_next(scale, good, skipped, interval) == impl.uvd_loss_scale_next(
                        scale, good, skipped, growth_interval=interval), (scale, good, skipped, interval)


def test_rounding_to_the_formats():
    import torch
    x = np.concatenate([np.random.default_rng(3).standard_normal(4000) * s for s in (1e-42, 1e-7, 1.0, 300.0, 7e4, 3.3e38)])
    x = np.concatenate([x, [0.0, 1.0, 1.00390625, 1.01171875, 65519.9, 65520.0, np.inf, -np.inf]])       # ties, the float16 edge
    with np.errstate(over="ignore"):                  # float32 values: torch narrows float64 through float32, twice rounded
        x = x.astype(np.float32).astype(np.float64)
    for fmt in ("float16", "bfloat16", "float32"):
        want = torch.from_numpy(x).to(getattr(torch, fmt)).double().numpy()
        assert np.array_equal(fm.round_to(x, fmt), want), fmt
        inside = x[np.abs(x) <= fm.FORMATS[fmt][2]]                                        # (neighbours: finite values of the format's range)
        lo, hi, x_ = *fm.neighbours(inside, fmt), x
        x = inside
        assert np.all(lo <= x) and np.all(x <= hi) and np.all((fm.round_to(x, fmt) == lo) | (fm.round_to(x, fmt) == hi))
        fin = np.isfinite(hi) & np.isfinite(lo) & (hi > lo)
        assert np.all((hi - lo)[fin] == fm.spacing(x, fmt)[fin])
        x = x_


# ------------------------------------------------------------------------------------------------------- the mutants
class DecayWithLr(fm.FlatStepModel):
    """decay taken with lr instead of lr_eff"""
    def decay_rate(self, lr_eff):
        return self.lr * self.weight_decay


class NoClipWithMomentum(fm.FlatStepModel):
    """clip factor left out when momentum is on"""
    def clip_factor(self, pre):
        return 1.0 if self.momentum != 0.0 else super().clip_factor(pre)


class HNotDividedByS(fm.FlatStepModel):
    """h not divided by S"""
    def h_scale(self, S, fd):
        return super().h_scale(1.0, fd)


class VNotDividedByDelta(fm.FlatStepModel):
    """v not divided by delta_param_scale on the fd route"""
    def v_scale(self, fd):
        return 1.0


class BetaOneStepOff(fm.FlatStepModel):
    """beta_k taken at k + 1"""
    def beta(self, k):
        return super().beta(k + 1)


class NoUndoOnSkippedFd(fm.FlatStepModel):
    """the undo left out on a skipped fd step"""
    def undo_skipped(self, W, v_T):
        return W


class GuardSeesStaleVH(fm.FlatStepModel):
    """the guard looking at v and h on a non-updating step (what the last updating step left in them)"""
    def guard_sees(self, update, v, h, g):
        if update and not self.whiten:
            self._stale = (v, h)
            return (v, h, g)
        return getattr(self, "_stale", ()) + (g,)


class TruncatesToBf16(fm.FlatStepModel):
    """truncation instead of nearest rounding to bfloat16"""
    def narrow(self, x):
        return fm._to_format(x, self.fmt, np.trunc) if self.fmt == "bfloat16" else super().narrow(x)


MUTANTS = [DecayWithLr, NoClipWithMomentum, HNotDividedByS, VNotDividedByDelta, BetaOneStepOff, NoUndoOnSkippedFd, GuardSeesStaleVH,
           TruncatesToBf16]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m.__name__ for m in MUTANTS])
def test_a_mutant_of_the_model_fails_the_gpu_comparison(mutant):
    """the mutant, in float64, in the class's place: the comparison and the bars of the GPU test must refuse it on some case"""
    caught = []
    for key in fc.keys():
        try:
            bad, _ = fc.yardstick_case(key, fc.bars(key.model), mutant, np.float64)
        except AssertionError as e:                   # the mutant broke what a case owes (which step is skipped): caught as well
            bad = [str(e)]
        if bad:
            caught.append((key, bad[0]))
            break
    assert caught, "%s (%s) passes every case of the grid" % (mutant.__name__, mutant.__doc__)
    print("%s fails %s: %s" % (mutant.__name__, "-".join(caught[0][0]), caught[0][1]))


def test_the_true_model_passes_its_own_comparison():
    """float64 against float64 on a slice of the grid: no violation, every distance 0 (the comparison itself is not what fails the
    mutants)"""
    for key in fc.keys()[::7]:
        bad, worst = fc.yardstick_case(key, fc.bars(key.model), fm.FlatStepModel, np.float64)
        assert not bad and all(e == 0.0 for e in worst.values()), (key, bad, worst)


# --------------------------------------------------------------------------------- the conditions can be met, and the bars
def test_the_float32_model_meets_the_low_precision_conditions():
    """The 1-spacing and 2 % conditions against the float64 run, and the bars, on EVERY case of the grid with the float32 run of
    the model in the class's place.  The seeds that this depends on are those of fc.problem (the sets' initial parameters, weights
    and draws), fc.coin_seed and fc.sr_pick: with them no float32 / float64 pair of this grid straddles a rounding boundary of T."""
    for key in fc.keys():
        bad, _ = fc.yardstick_case(key, fc.bars(key.model))
        assert not bad, (key, bad)


def test_bars_are_derived_and_capped():
    for m in fc.MODEL_CLASSES:
        b = fc.bars(m)
        for q in fc.QUANTITIES:
            assert b[q] == 2.0 * max(fc.yardstick()[(m, q)], fc.BAR_FLOOR) and b[q] <= fc.BAR_CAP
            print("%-8s %-10s yardstick %.3e  bar %.3e" % (m, q, fc.yardstick()[(m, q)], b[q]))


def test_the_grid():
    assert len(fc.cases()) == 6 * 2 * 2 * 3 * 4 * 4 - len(fc.LEFT_OUT) and len(fc.keys()) == 4 * 2 * 3 * 4 * 4
    assert {fc.n_of(s) for s in fc.SETS} == {117, 132}
