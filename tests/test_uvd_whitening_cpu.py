"""UVd(preconditioner_fit="whitening") without a GPU: the constructor's checks, the checkpoint keys of the probe stream (class and
reshard_uvd_state), and the convergence case on the fp64 oracle alone -- the level the GPU test then holds the kernels to."""
import numpy as np
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import sharded
from tests import uvd_whitening_cases as wc


def _params(n=192):
    return [torch.zeros(n, requires_grad=True)]


# ------------------------------------------------------------------------------------------------------------- validation
def test_a_bad_preconditioner_fit_is_refused_before_any_device_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a tensor was made before the argument was judged")
    monkeypatch.setattr(torch, "randn", boom)
    monkeypatch.setattr(torch, "ones", boom)
    for bad in ("whiten", "Hessian", None, 1):
        with pytest.raises(ValueError, match="UVd: preconditioner_fit"):
            psgd.UVd(_params(), 2, preconditioner_fit=bad)
    with pytest.raises(TypeError):                                       # both arguments are keyword-only
        psgd.UVd(_params(), 2, 1.0, 0.01, 0.01, None, 1.0, True, None, None, None, None, "auto", "widen", None, "torch", 0.0, 0.0,
                 "propagate", None, 2000, "hessian")


def test_hessian_draws_no_seed_and_whitening_draws_exactly_one(monkeypatch):
    drawn = []
    real = psgd.UVd._draw_seed
    monkeypatch.setattr(psgd.UVd, "_draw_seed", lambda self, explicit: drawn.append(explicit) or real(self, explicit))
    gen = torch.Generator().manual_seed(3)
    before = gen.get_state().clone()
    for kw in ({}, {"preconditioner_fit": "hessian"}, {"preconditioner_fit": "hessian", "probe_seed": 9}):
        opt = psgd.UVd(_params(), 2, generator=gen, **kw)
        assert opt.probe_seed0 is None and opt.probe_step == 0 and opt.preconditioner_fit == "hessian"
    assert drawn == [] and torch.equal(gen.get_state(), before)          # nothing drawn, the generator untouched
    opt = psgd.UVd(_params(), 2, generator=gen, preconditioner_fit="whitening")
    twin = torch.Generator().manual_seed(3)
    assert drawn == [None] and opt.probe_seed0 == int(torch.randint(0, 2 ** 62, (), generator=twin).item())
    opt = psgd.UVd(_params(), 2, generator=gen, preconditioner_fit="whitening", probe_seed=2 ** 64 + 5)
    assert opt.probe_seed0 == 5 and opt._probe is None                   # an explicit seed: its low 64 bits, no draw, no buffer yet


# -------------------------------------------------------------------------------------------------------- checkpoint keys
def test_state_dict_round_trips_the_probe_stream():
    a = psgd.UVd(_params(), 2, preconditioner_fit="whitening", probe_seed=41)
    a._probe_step = 7
    sd = a.state_dict()
    assert (sd["probe_seed0"], sd["probe_step"]) == (41, 7) and "preconditioner_fit" not in sd["hyper"]
    b = psgd.UVd(_params(), 2, preconditioner_fit="whitening", probe_seed=1)
    b.load_state_dict(sd)
    assert (b.probe_seed0, b.probe_step) == (41, 7)
    h = psgd.UVd(_params(), 2)
    sdh = h.state_dict()
    assert "probe_seed0" not in sdh and "probe_step" not in sdh          # a hessian-fit optimizer adds nothing
    b.load_state_dict(sdh)                                               # a dict without the keys: this object's seed, counter 0
    assert (b.probe_seed0, b.probe_step) == (41, 0)
    h.load_state_dict(sd)                                                # ... and a hessian-fit optimizer ignores the keys
    assert (h.probe_seed0, h.probe_step) == (None, 0)
    with pytest.raises(ValueError, match="probe_step"):
        b.load_state_dict({k: v for k, v in sd.items() if k != "probe_step"})


def test_reshard_carries_the_probe_keys_unchanged():
    n, sds = 192, []
    for row0, rows in ((0, 128), (128, 64)):
        o = psgd.UVd(_params(rows), 2, preconditioner_fit="whitening", probe_seed=2 ** 63 + 11, generator=torch.Generator().manual_seed(1))
        o._probe_step = 5
        sd = o.state_dict()
        sd["row0"], sd["num_params_global"] = row0, n
        sds.append(sd)
    for counts in ([64, 64, 64], [n]):
        out = sharded.reshard_uvd_state(sds, counts)
        assert [(s["probe_seed0"], s["probe_step"]) for s in out] == [(2 ** 63 + 11, 5)] * len(counts)
        o = psgd.UVd(_params(counts[0]), 2, preconditioner_fit="whitening", probe_seed=0)
        o.load_state_dict(out[0], strict=False)
        assert (o.probe_seed0, o.probe_step) == (2 ** 63 + 11, 5)
    sds[1]["probe_step"] = 6                                             # the keys are global: ranks that disagree are refused
    with pytest.raises(ValueError, match="probe_step"):
        sharded.reshard_uvd_state(sds, [n])


# ------------------------------------------------------------------------------------------- convergence on the oracle alone
def test_the_oracle_whitens_the_two_scale_gradient():
    """N = 256, r = 4, g = sigma .* z with sigma = 0.1 | 10, probes from counter_randn, update_precond_UVd_math_ of the oracle in fp64
    at lr_preconditioner = 0.2 for 2000 steps (tests/uvd_whitening_cases.py has why these two).  The variance ratio of P g between
    the halves, on 64 fresh samples: 1e4 for P = I, 792.3 with the reference's initial U and V (the large half leaks through U V'
    into the small one), and 1.930 after the 2000 steps -- the level of 2 is met, and is what the kernels are held to."""
    start = wc.variance_ratio(*wc.initial_state())
    ident = wc.variance_ratio(np.zeros((wc.N, wc.R)), np.zeros((wc.N, wc.R)), np.ones((wc.N, 1)))
    (U, V, d), _ = wc.oracle_run(wc.STEPS)
    end = wc.variance_ratio(U, V, d)
    print("variance ratio: P = I %.4g, initial state %.4g, after %d steps at lr %g: %.4f" % (ident, start, wc.STEPS, wc.LR_PRECOND, end))
    assert 0.7e4 < ident < 1.4e4 and wc.STEPS <= 2000
    assert end <= wc.LEVEL
