"""Whole steps of class UVd, class SPLU and class Dense against the float64 model of tests/flat_step_model.py over the switch grid
of _FlatStep.step: what a step leaves in the PARAMETERS, the preconditioner state, the momentum buffer and the counters, with the
switches on together.  tests/flat_step_cases.py has the inputs both sides share, the comparison and how the bars are derived.

The grid, 1152 cases of 4 steps each (every combination; no constructor refuses one, so none is left out):

    class      UVd rank 3 and rank 10 on the float32 state, each with the default placement and with placement="packed";
               SPLU rank 3 on the float32 state; Dense
    set        N117 = (7, 9), (33,), (2, 2, 2, 2), (5,)        N132 = (16, 8), (4,)
    tail       torch, fused                  fit     exact, fd, whitening
    dtype      float32, bfloat16 nearest, bfloat16 stochastic, float16
    features   off | momentum 0.9 + weight_decay 0.01 + an active clip | those + nonfinite="skip" + loss_scale=2**10 with an Inf
               gradient in step 3 | those with loss_scale="dynamic" and loss_scale_growth_interval=2 (the scale doubles after step
               2 and halves in step 3)

One test is one (class, set, tail, fit, dtype) and walks the 4 feature settings of it.  Asserted after every step: the counters and
flags exactly; that the state changed exactly when the replayed coin says so; a skipped step leaves every bit (fd: the parameters
within one rounding of T); state, momentum buffer and float32 increment within the bars; low-precision parameters within one
spacing of x64, at most 2 % of a case's elements further than half a spacing plus slack; stochastic ones on a T-neighbour of x64.

PSGD_FLAT_STEP_PARITY_OUT=<file> writes the yardstick's distances, the measured ones and the bars (profiles/flat_step_parity.txt).
"""
import os
import time

import pytest
import torch

from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl
from tests import flat_step_cases as fc

pytestmark = pytest.mark.gpu

GROUPS = [(c, s, t, f, d) for c in fc.CLASSES for s in fc.SETS for t in fc.TAILS for f in fc.FITS for d in fc.DTYPES]
MEASURED = {}                                       # (class, quantity) -> the worst distance any of its cases measured
_T0 = [None]


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    m.set_dense_route("native")
    return m


@pytest.fixture(scope="module")
def bars():
    """the bars of every model class, and at the end of the module the record of what was measured"""
    _T0[0] = time.time()
    out = {m: fc.bars(m) for m in fc.MODEL_CLASSES}
    yield out
    path = os.environ.get("PSGD_FLAT_STEP_PARITY_OUT")
    if path:
        lines = ["# class quantity: worst distance of the float32 NumPy model from the float64 model over the grid (the yardstick),",
                 "# worst distance of the class on the GPU from the float64 model, the bar = 2 max(yardstick, %g); cap %g" % (fc.BAR_FLOOR, fc.BAR_CAP)]
        for cls in fc.CLASSES:
            model_cls = fc.CLASSES[cls][3]
            for q in fc.QUANTITIES:
                lines.append("%-16s %-10s yardstick %.3e  measured %.3e  bar %.3e" % (
                    cls, q, fc.yardstick()[(model_cls, q)], MEASURED.get((cls, q), float("nan")), out[model_cls][q]))
        for cls in fc.CLASSES:
            lines.append("%-16s largest share of a low-precision nearest case's elements beyond half a spacing plus slack: %.4f (cap %g)"
                         % (cls, MEASURED.get((cls, fc.SHARE), float("nan")), fc.BEYOND_HALF_CAP))
        lines.append("# %d cases, %.1f s from the first fixture to the last test" % (len(fc.cases()), time.time() - _T0[0]))
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _dev():
    return torch.device("cuda:0")


def _raw(t):
    return t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()


def _f64(t):
    return t.detach().double().cpu().numpy()


def _state(opt):
    if isinstance(opt, impl.Dense):
        return [opt.Q]
    if isinstance(opt, impl.SPLU):
        return list(opt.factors)
    return [opt._U, opt._V, opt._d]


class ClassActor:
    """the optimizer class in a case: built on the case's parameters, coins and draws; step(k) runs one step and reports what
    the comparison reads"""

    def __init__(self, psgd, monkeypatch, case):
        key = self.key = fc.key_of(case)
        kind, rank, extra, _ = fc.CLASSES[case.cls]
        fmt, stochastic = fc.DTYPES[key.dt]
        dtype = getattr(torch, fmt)
        _, a, draws = fc.problem(key.set)
        self.tensors = [torch.from_numpy(w).to(_dev(), dtype).requires_grad_(True) for w in fc.initial_params(key)]
        a_dev = [torch.from_numpy(x).to(_dev()) for x in a]
        self.flags = flags = {"poison": False, "draws": iter(())}
        monkeypatch.setattr(impl, "_randn_like", lambda p: torch.from_numpy(next(flags["draws"])).to(p.device, p.dtype))
        self.draws = draws
        params = self.tensors

        def closure():                                # float64 throughout: autograd rounds to the parameters' dtype once
            loss = sum(torch.sum(x * torch.cosh(p.double())) for p, x in zip(params, a_dev))
            if flags["poison"]:
                loss = loss + params[1].double().sum() * float("inf")
            return loss
        self.closure = closure
        kw = dict(preconditioner_init_scale=fc.INIT_SCALE[kind], lr_params=fc.LR, lr_preconditioner=fc.LR_Q, grad_clip_max_norm=None,
                  preconditioner_update_probability=fc.P_UPDATE, exact_hessian_vector_product=key.fit != "fd",
                  generator=torch.Generator().manual_seed(fc.coin_seed(key)), step_tail=case.tail,
                  param_rounding="stochastic" if stochastic else "nearest",
                  preconditioner_fit="whitening" if key.fit == "whitening" else "hessian", **extra)
        if key.feat != "off":
            kw.update(momentum=fc.MOMENTUM, weight_decay=fc.WEIGHT_DECAY)
        if key.feat in ("static", "dynamic"):
            kw.update(nonfinite="skip", loss_scale=fc.STATIC_SCALE if key.feat == "static" else "dynamic",
                      loss_scale_growth_interval=fc.GROWTH_INTERVAL)
        if kind != "dense":
            kw["rank_of_modification"] = rank
        torch.manual_seed(1234)                       # the device generator behind UVd's initial U and V
        self.opt = opt = getattr(psgd, case.cls.split("-")[0])(self.tensors, **kw)
        assert (opt._tail is not None) == (case.tail == "fused")
        assert ("placement" in extra) == (getattr(opt, "_arena", None) is not None)
        self.state0 = [_f64(t) for t in _state(opt)]               # read once; the model carries its own from here
        self.probe_seed0 = opt.probe_seed0
        self._bits = self._snapshot()

    def set_max_norm(self, max_norm):
        if max_norm is not None:
            self.opt.grad_clip_max_norm.assign(max_norm)

    def _momentum(self):
        return self.opt._momentum_buffer() if self.key.feat != "off" else None

    def _snapshot(self):
        m = self._momentum()
        return ([_raw(t) for t in _state(self.opt)], None if m is None else _raw(m), [_raw(p) for p in self.tensors])

    def params(self):
        return [_f64(p) for p in self.tensors]

    def step(self, k):
        opt = self.opt
        self.flags["poison"], self.flags["draws"] = fc.poisoned(self.key, k), iter(self.draws[k])
        opt.step(self.closure)
        before, after = self._bits, self._snapshot()
        self._bits = after
        m = self._momentum()
        return dict(counters=(opt.skipped_steps, opt.last_step_skipped, opt.loss_scale.value, opt._m_step, opt.probe_step,
                              opt._param_round_step),
                    state=[_f64(t) for t in _state(opt)], m=None if m is None else _f64(m).reshape(-1, 1), params=self.params(),
                    same_state=before[0] == after[0], same_m=before[1] == after[1], same_params=before[2] == after[2])


@pytest.mark.parametrize("cls,set_name,tail,fit,dt", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_steps_match_the_fp64_model(psgd, monkeypatch, bars, cls, set_name, tail, fit, dt):
    bad = []
    if True:
        for feat in fc.FEATURES:
            case = fc.Case(cls, set_name, tail, fit, dt, feat)
            if case in fc.LEFT_OUT:
                continue
            actor = ClassActor(psgd, monkeypatch, case)
            key = actor.key
            max_norm = fc.clip_norm(key, actor.state0, actor.probe_seed0)
            actor.set_max_norm(max_norm)
            coins, branches = fc.replayed_coins(key, fc.coin_seed(key))
            model = fc.make_model(key, actor.state0, max_norm)
            violations, worst = fc.run(key, actor, model, coins, branches, actor.probe_seed0, bars[key.model])
            for q, e in worst.items():
                MEASURED[(cls, q)] = max(MEASURED.get((cls, q), 0.0), e)
            print("%s: %s" % ("-".join(case), "  ".join("%s %.3e" % (q, e) for q, e in sorted(worst.items()))))
            bad += ["%s-%s: %s" % (dt, feat, v) for v in violations]
    assert not bad, "\n".join(bad)

