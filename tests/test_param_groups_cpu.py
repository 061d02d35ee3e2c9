"""param_groups= of UVd, SPLU, Dense and Kron without a GPU: every construction error (raised before a device is looked at, so
class Kron, which has no CPU route, shows them here too), the contents of opt.param_groups, the re-check of assigned values at
the next step, the checkpoint key (present only with groups; round trip; a dict with another partition is refused and leaves the
object as it was), the refusal of reshard_uvd_state, and the argument checks of the functional tails' tensor_groups.

Five parameter tensors of sizes [1, 5, PSGD_UVD_TAIL_CHUNK + 3, 64, 7]; the groups are interleaved: {0, 3}, {2}, the rest implicit."""
import copy
import math

import pytest
import torch

from psgd_tf_amd import _lib
from psgd_tf_amd import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import sharded

SIZES = [1, 5, _lib.UVD_TAIL_CHUNK + 3, 64, 7]
FLAT = {"UVd": lambda ps, **kw: psgd.UVd(ps, 2, **kw), "SPLU": lambda ps, **kw: psgd.SPLU(ps, 2, **kw),
        "Dense": lambda ps, **kw: psgd.Dense(ps, **kw)}
ALL = dict(FLAT, Kron=lambda ps, **kw: psgd.Kron(ps, any_rank=True, **kw))


def _params(sizes=SIZES):
    return [torch.zeros(n, requires_grad=True) for n in sizes]


def _small():
    return _params([1, 5, 9, 4, 7])           # class Dense holds N^2 numbers: the construction checks need no chunk boundary


def _groups(ps):
    return [{"params": [ps[3], ps[0]], "lr_scale": 0.5, "weight_decay": 0.0}, {"params": [ps[2]], "weight_decay": 0.25}]


BAD = {
    "listed twice": (lambda ps: [{"params": [ps[1], ps[1]]}], "parameter 1 .*listed twice"),
    "in two groups": (lambda ps: [{"params": [ps[1]]}, {"params": [ps[4], ps[1]]}], r"parameter 1 .*listed twice.*group 1"),
    "not a parameter": (lambda ps: [{"params": [torch.zeros(5, requires_grad=True)]}], "not one of this optimizer's parameters"),
    "no requires_grad": (lambda ps: [{"params": [ps[0].detach()]}], "not one of this optimizer's parameters"),
    "empty params": (lambda ps: [{"params": []}], r"param_groups\[0\] has no 'params'"),
    "missing params": (lambda ps: [{"params": [ps[0]]}, {"lr_scale": 2.0}], r"param_groups\[1\] has no 'params'"),
    "negative lr_scale": (lambda ps: [{"params": [ps[0]], "lr_scale": -0.5}], "lr_scale must be finite and >= 0"),
    "NaN lr_scale": (lambda ps: [{"params": [ps[0]], "lr_scale": math.nan}], "lr_scale must be finite and >= 0"),
    "infinite lr_scale": (lambda ps: [{"params": [ps[0]], "lr_scale": math.inf}], "lr_scale must be finite and >= 0"),
    "negative weight_decay": (lambda ps: [{"params": [ps[0]], "weight_decay": -1e-3}], "weight_decay must be >= 0"),
    "NaN weight_decay": (lambda ps: [{"params": [ps[0]], "weight_decay": math.nan}], "weight_decay must be >= 0"),
    "unknown key": (lambda ps: [{"params": [ps[0]], "lr": 0.1}], r"param_groups\[0\] has unknown key 'lr'"),
}


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("cls", list(ALL))
def test_construction_errors_name_the_class_and_touch_no_device(monkeypatch, cls, bad):
    """(on the commit before this one every case is a TypeError: the constructors do not know the keyword)"""
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    make, match = BAD[bad]
    ps = _small()
    with pytest.raises(ValueError, match="^%s: .*%s" % (cls, match)):
        ALL[cls](ps, param_groups=make(ps))


@pytest.mark.parametrize("cls", list(FLAT))
def test_param_groups_attribute(cls):
    ps = _small()
    assert FLAT[cls](ps).param_groups is None and FLAT[cls](ps, param_groups=None).param_groups is None
    opt = FLAT[cls](ps, weight_decay=0.125, param_groups=_groups(ps))
    gs = opt.param_groups
    assert [g.indices for g in gs] == [(0, 3), (2,), (1, 4)]                       # positions, ascending; the implicit group last
    assert all(isinstance(g.lr_scale, psgd._Hyper) and isinstance(g.weight_decay, psgd._Hyper) for g in gs)
    assert [(float(g.lr_scale), g.weight_decay.value) for g in gs] == [(0.5, 0.0), (1.0, 0.25), (1.0, None)]
    # what a step uses: None follows opt.weight_decay at every step
    assert opt._step_groups(float(opt.weight_decay)) == [((0, 3), 0.5, 0.0), ((2,), 1.0, 0.25), ((1, 4), 1.0, 0.125)]
    opt.weight_decay.assign(0.5)
    assert opt._step_groups(float(opt.weight_decay))[2] == ((1, 4), 1.0, 0.5)
    # groups that name every parameter leave no implicit group; a single tensor may stand for a list of one
    full = FLAT[cls](ps, param_groups=[{"params": ps[:2]}, {"params": ps[2:]}])
    assert [g.indices for g in full.param_groups] == [(0, 1), (2, 3, 4)]
    assert [g.indices for g in FLAT[cls](ps, param_groups=[{"params": ps[4]}]).param_groups] == [(4,), (0, 1, 2, 3)]


def test_kron_param_groups_attribute():
    """class Kron has no CPU route: the stage of its constructor that judges the groups, on its own"""
    ps = _small()
    opt = psgd.Kron.__new__(psgd.Kron)
    opt._params = ps
    assert opt.param_groups is None
    opt._init_groups(_groups(ps))
    assert [(g.indices, float(g.lr_scale), g.weight_decay.value) for g in opt.param_groups] == \
        [((0, 3), 0.5, 0.0), ((2,), 1.0, 0.25), ((1, 4), 1.0, None)]
    with pytest.raises(ValueError, match="one HIP device"):                          # valid groups: the constructor goes on to the device
        psgd.Kron(ps, any_rank=True, param_groups=_groups(ps))


@pytest.mark.parametrize("cls", list(FLAT))
@pytest.mark.parametrize("which,value", [("lr_scale", -1.0), ("lr_scale", math.nan), ("lr_scale", math.inf), ("weight_decay", -0.5),
                                         ("weight_decay", math.nan)])
def test_an_assigned_bad_value_is_refused_by_the_next_step(cls, which, value):
    ps = _small()
    opt = FLAT[cls](ps, param_groups=_groups(ps))
    getattr(opt.param_groups[1], which).assign(value)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(ValueError, match=r"^%s: param_groups\[1\]: %s" % (cls, which)):
        opt.step(lambda: pytest.fail("the closure was called"))
    assert all(torch.equal(p, b) for p, b in zip(ps, before))
    getattr(opt.param_groups[1], which).assign(0.75)                                 # a schedule assigns with .assign(), as everywhere
    assert opt._step_groups(0.0)[1][1 if which == "lr_scale" else 2] == 0.75


@pytest.mark.parametrize("cls", list(FLAT))
def test_state_dict_round_trip_and_partition_mismatch(cls):
    ps = _small()
    plain = FLAT[cls](ps, generator=torch.Generator().manual_seed(1))
    assert "param_groups" not in plain.state_dict()
    opt = FLAT[cls](ps, generator=torch.Generator().manual_seed(1), param_groups=_groups(ps))
    sd = opt.state_dict()
    assert sd["param_groups"] == [{"indices": [0, 3], "lr_scale": 0.5, "weight_decay": 0.0},
                                  {"indices": [2], "lr_scale": 1.0, "weight_decay": 0.25},
                                  {"indices": [1, 4], "lr_scale": 1.0, "weight_decay": None}]
    assert {k: v for k, v in sd.items() if k != "param_groups"}.keys() == plain.state_dict().keys()
    # the values are assigned into an object with the same partition, whatever it was built with
    other = FLAT[cls](ps, param_groups=[{"params": [ps[0], ps[3]], "lr_scale": 3.0, "weight_decay": 1.0}, {"params": [ps[2]], "lr_scale": 0.0}])
    other.load_state_dict(sd)
    assert other.state_dict()["param_groups"] == sd["param_groups"]
    # a dict without the key: the object keeps its own values
    other.param_groups[0].lr_scale.assign(7.0)
    other.load_state_dict({k: v for k, v in sd.items() if k != "param_groups"})
    assert float(other.param_groups[0].lr_scale) == 7.0
    # another partition, a bad value, or groups into an object without groups: ValueError, and the object is left as it was
    moved = copy.deepcopy(sd)
    moved["param_groups"][0]["indices"], moved["param_groups"][2]["indices"] = [0], [1, 3, 4]
    moved["hyper"]["lr_params"] = 123.0
    bad_value = copy.deepcopy(sd)
    bad_value["param_groups"][1]["lr_scale"] = -1.0
    bad_value["hyper"]["lr_params"] = 123.0
    for target, dict_ in ((other, moved), (other, bad_value), (plain, sd)):
        before = target.state_dict()
        with pytest.raises(ValueError, match="%s.load_state_dict: .*param_groups" % cls):
            target.load_state_dict(dict_)
        after = target.state_dict()
        assert after.keys() == before.keys()
        for k in before:
            same = torch.equal(before[k], after[k]) if isinstance(before[k], torch.Tensor) else before[k] == after[k]
            assert same, k


def test_kron_checkpoint_helpers():
    """class Kron has no CPU route: the three helpers its state_dict / load_state_dict call, on an object with groups only"""
    ps = _small()
    opt = psgd.Kron.__new__(psgd.Kron)
    opt._params = ps
    assert opt._groups_encode({}) == {}
    opt._init_groups(_groups(ps))
    sd = opt._groups_encode({})
    assert [g["indices"] for g in sd["param_groups"]] == [[0, 3], [2], [1, 4]]
    assert opt._groups_judge({}, "Kron.load_state_dict") is None
    sd["param_groups"][0]["lr_scale"] = 0.125
    opt._groups_commit(opt._groups_judge(sd, "Kron.load_state_dict"))
    assert float(opt.param_groups[0].lr_scale) == 0.125
    sd["param_groups"][1]["indices"] = [1]
    with pytest.raises(ValueError, match="Kron.load_state_dict: 'param_groups' partitions"):
        opt._groups_judge(sd, "Kron.load_state_dict")


def test_reshard_refuses_dicts_with_groups():
    ps = _params([64, 64])
    opt = psgd.UVd(ps, 2, param_groups=[{"params": [ps[0]], "lr_scale": 0.0}])
    sd = opt.state_dict()
    with pytest.raises(ValueError, match="reshard_uvd_state: .*param_groups"):
        sharded.reshard_uvd_state([sd], [64, 64])
    del sd["param_groups"]
    assert len(sharded.reshard_uvd_state([sd], [64, 64])) == 2


@pytest.mark.parametrize("groups,match", [
    ([((0, 1), 1.0, 0.0)], r"partition range\(3\).*\[2\] are in no group"),
    ([((0, 1), 1.0, 0.0), ((1, 2), 1.0, 0.0)], "index 1 of tensor_groups.1. is listed twice"),
    ([((0, 1, 3), 1.0, 0.0), ((2,), 1.0, 0.0)], "index 3 of tensor_groups.0. is out of range"),
    ([((0, 1, 2), -1.0, 0.0)], "lr_scale must be finite"),
    ([((0, 1, 2), math.inf, 0.0)], "lr_scale must be finite"),
    ([((0, 1, 2), 1.0, math.nan)], "weight_decay must be >= 0"),
    ([((0, 1, 2), 1.0)], r"must be \(indices, lr_scale, weight_decay\)"),
    ([((), 1.0, 0.0), ((0, 1, 2), 1.0, 0.0)], "has no indices"),
])
def test_tensor_groups_argument_checks(groups, match):
    with pytest.raises(ValueError, match="uvd_step_tail: .*" + match):
        psgd._tensor_groups("uvd_step_tail", groups, 3, 0.0, True)
    assert psgd._tensor_groups("uvd_step_tail", None, 3, 0.5, True) is None
    with pytest.raises(ValueError, match="leave the weight_decay argument at 0"):
        psgd._tensor_groups("uvd_step_tail", [((0, 1, 2), 1.0, 0.0)], 3, 0.5, True)
    with pytest.raises(ValueError, match="perturbation"):
        psgd._tensor_groups("multi_param_update", [((0, 1, 2), 1.0, 0.0)], 3, 0.0, False)
    assert psgd._tensor_groups("x", [([2, 0], 2, 0.5), ((1,), 0, 0)], 3, 0.0, True) == [((0, 2), 2.0, 0.5), ((1,), 0.0, 0.0)]
