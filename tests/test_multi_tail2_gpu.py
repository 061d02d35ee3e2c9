"""The list kernels that momentum, the guard and weight decay of class Kron add to psgd_multi_tail.hip, through their wrappers
(kron_optimizer.multi_blend / multi_scale_check / multi_param_update(weight_decay=)): bit for bit against the torch expressions they
replace, on the shape lists of tests/test_multi_tail_gpu.py (chunk of 4096 elements, grid cap of 2048 workgroups).  The non-finite
values here are data that the kernels must report, not faults."""
import math

import numpy as np
import pytest
import torch

from tests import test_multi_tail_gpu as mt

pytestmark = pytest.mark.gpu

CHUNK, MAX_GRID, TINY = mt.CHUNK, mt.MAX_GRID, mt.TINY
WHICH = mt.WHICH
_dev, _assert_bits, _f64 = mt._dev, mt._assert_bits, mt._f64


@pytest.fixture(scope="module")
def ko():
    from psgd_tf_amd import _lib, kron_optimizer
    assert _lib.UVD_TAIL_CHUNK == CHUNK and _lib.UVD_TAIL_MAX_GRID == MAX_GRID
    return kron_optimizer


def _make_dyadic(which, seed, roles):
    """as mt._make, values j / 16 with |j| <= 64"""
    sizes, offsets = mt._lists_of(which)
    gen = torch.Generator(device=_dev()).manual_seed(seed)
    return {role: mt._carve(sizes, [(o + (r if which == "unaligned" else 0)) % 4 for o in offsets], gen, mt._dyadic)
            for r, role in enumerate(roles)}


def _flag(value):
    return torch.tensor([value], dtype=torch.int32, device=_dev())


# -------------------------------------------------------------------------------------------------------------------- blend
BETAS = [0.0, 0.5, float(np.float32(0.9))]


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("data", ["random", "dyadic"])
@pytest.mark.parametrize("which", WHICH)
def test_blend(ko, which, data, beta):
    """m = fl32(fl32(beta m) + fl32(omb g)); beta == 0 stores fl32(omb g) whatever m held"""
    d = mt._make(which, 11, ("m", "g")) if data == "random" else _make_dyadic(which, 12, ("m", "g"))
    omb = float(np.float32(1.0) - np.float32(beta))
    if beta == 0.0:
        for m in d["m"]:
            m.fill_(float("nan"))
        want = [g * omb for g in d["g"]]
    else:
        want = [m * beta + g * omb for m, g in zip(d["m"], d["g"])]
    untouched = [g.clone() for g in d["g"]]
    ko.multi_blend(d["m"], d["g"], beta, omb)
    _assert_bits(d["m"], want, "blend")
    _assert_bits(d["g"], untouched, "gradients")
    if beta == 0.0 and data == "dyadic":
        assert all(bool(torch.isfinite(m).all()) for m in d["m"])                   # no NaN of the old buffer came through


def test_blend_takes_beta_and_omb_as_given(ko):
    """omb is an argument of its own: the kernel does not form 1 - beta"""
    d = _make_dyadic("edges", 13, ("m", "g"))
    want = [m * 0.5 + g * 0.25 for m, g in zip(d["m"], d["g"])]
    ko.multi_blend(d["m"], d["g"], 0.5, 0.25)
    _assert_bits(d["m"], want, "blend with omb != 1 - beta")


# -------------------------------------------------------------------------------------------------------------- scale-check
S16 = 2.0 ** -16                                 # ("fd" below: float32(_FD_INV) of the module under test)


@pytest.mark.parametrize("scales", [("s16",), (1.0,), ("fd", 1.0), ("s16", "fd", 1.0), (1.0, 1.0, 1.0)])
@pytest.mark.parametrize("which", WHICH)
def test_scale_check_on_clean_data(ko, which, scales):
    """finite data: scaled lists equal x * s, lists with scale 1 keep their bits, the flag word keeps an old stamp"""
    scales = [S16 if s == "s16" else float(np.float32(ko._FD_INV)) if s == "fd" else s for s in scales]
    roles = ("a", "b", "c")[:len(scales)]
    d = mt._make(which, 21, roles, plant=False)
    want = [[x * s for x in d[r]] if s != 1.0 else [x.clone() for x in d[r]] for r, s in zip(roles, scales)]
    flag = _flag(41)
    ko.multi_scale_check([d[r] for r in roles], scales, flag=flag, stamp=42)
    assert int(flag.item()) == 41, "clean data stored to the flag"
    for r, w in zip(roles, want):
        _assert_bits(d[r], w, "list %s" % r)


@pytest.mark.parametrize("which", WHICH)
def test_scale_check_without_a_flag_only_rescales(ko, which):
    d = mt._make(which, 22, ("a", "b"))                                             # specials planted: they scale like the rest
    want_a, want_b = [x * S16 for x in d["a"]], [x.clone() for x in d["b"]]
    ko.multi_scale_check([d["a"], d["b"]], [S16, 1.0])
    _assert_bits(d["a"], want_a, "scaled")
    _assert_bits(d["b"], want_b, "scale 1")


@pytest.fixture(scope="module")
def placed():
    """three lists with a head, a tail, a second chunk and a tensor that only the second trip of the grid-stride loop reaches"""
    sizes = [CHUNK + 3, 37, 2 * CHUNK + 8] + [6] * 2100 + [5000]
    offsets = [1, 2, 3] + [(2 * i) % 4 for i in range(2101)]
    assert sum(-(-n // CHUNK) for n in sizes[:3]) + 2050 >= MAX_GRID
    gen = torch.Generator(device=_dev()).manual_seed(23)
    lists = [mt._carve(sizes, [(o + r) % 4 for o in offsets], gen, mt._randn) for r in range(3)]
    return lists


def _place(ts, where):
    """(tensor index, element index) of a placement in the list ts"""
    if where == "first":
        return 0, 0
    if where == "last":
        return len(ts) - 1, ts[-1].numel() - 1
    if where == "head":                          # in front of the first 16-byte boundary of its chunk
        i = next(i for i in range(3) if ts[i].data_ptr() % 16)
        return i, 0
    if where == "tail":                          # behind the last 16-byte boundary of its chunk
        i = next(i for i in range(3) if (ts[i].data_ptr() + 4 * ts[i].numel()) % 16)
        return i, ts[i].numel() - 1
    if where == "element_4096":
        return 2, CHUNK
    if where == "second_trip":                   # chunk 6 + 2050 >= 2048: the second trip of the loop
        return 3 + 2050, 3
    raise KeyError(where)


@pytest.mark.parametrize("value", [float("inf"), -float("inf"), float("nan")])
@pytest.mark.parametrize("where", ["first", "last", "head", "tail", "element_4096", "second_trip"])
@pytest.mark.parametrize("which_list", [0, 1, 2])
def test_scale_check_finds_one_non_finite_value(ko, placed, which_list, where, value):
    scales = [1.0, 0.5, 1.0]                     # one list is stored (its values halve from test to test and stay finite)
    flag = _flag(6)
    ko.multi_scale_check(placed, scales, flag=flag, stamp=7)
    assert int(flag.item()) == 6, "the data of this test is not clean"
    i, j = _place(placed[which_list], where)
    t = placed[which_list][i]
    old = t[j].clone()
    t[j] = value
    try:
        ko.multi_scale_check(placed, scales, flag=flag, stamp=8)
        assert int(flag.item()) == 8, "%r at %s of list %d was not reported" % (value, where, which_list)
        got = t[j].clone()
        assert (math.isnan(value) and bool(torch.isnan(got))) or float(got) == value
    finally:
        t[j] = old if which_list != 1 else old * 0.5


@pytest.mark.parametrize("nlists", [1, 2, 3])
def test_scale_check_counts_an_overflow_under_the_scale(ko, nlists):
    """a finite 3e38 times 2 is +Inf: bad, in whichever list it sits; the same value under scale 1 is not"""
    for bad_list in range(nlists):
        d = mt._make("edges", 24, ("a", "b", "c")[:nlists], plant=False)
        lists = [d[r] for r in ("a", "b", "c")[:nlists]]
        lists[bad_list][4].view(-1)[CHUNK - 1] = 3e38
        flag = _flag(0)
        ko.multi_scale_check(lists, [1.0] * nlists, flag=flag, stamp=1)
        assert int(flag.item()) == 0
        scales = [1.0] * nlists
        scales[bad_list] = 2.0
        ko.multi_scale_check(lists, scales, flag=flag, stamp=2)
        assert int(flag.item()) == 2
        assert float(lists[bad_list][4].view(-1)[CHUNK - 1]) == float("inf")


# ------------------------------------------------------------------------------------------------------- update with decay
def _want_update(d, lr_t, wd, with_vs):
    c = lr_t * torch.tensor(wd, dtype=torch.float32, device=_dev())                 # fl32(lr_eff * wd)
    if with_vs:
        return [p - ((g * lr_t + v) + p * c) for p, g, v in zip(d["p"], d["g"], d["v"])]
    return [p - (g * lr_t + p * c) for p, g in zip(d["p"], d["g"])]


@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("which", WHICH)
def test_update_with_decay_without_clipping(ko, which, with_vs):
    """specials planted: +-0, +-Inf, NaN, +-max, +-tiny and subnormals meet one another in p, g and v"""
    d = mt._make(which, 31, ("p", "g", "v"))
    lr, wd = 0.0371, 0.0123
    lr_t = torch.tensor(lr, dtype=torch.float32, device=_dev())
    want = _want_update(d, lr_t, wd, with_vs)
    untouched = [t.clone() for t in d["g"] + d["v"]]
    ko.multi_param_update(d["p"], d["g"], d["v"] if with_vs else None, lr, weight_decay=wd)
    _assert_bits(d["p"], want, "update with decay")
    _assert_bits(d["g"] + d["v"], untouched, "operands")


@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("S", [0.0, 4.0, 1e12, float("nan")])
@pytest.mark.parametrize("which", ["edges", "unaligned"])
def test_update_with_decay_and_clipping_from_a_host_written_sum(ko, which, S, with_vs):
    d = mt._make(which, 32, ("p", "g", "v"), plant=not math.isnan(S))
    lr, max_norm, wd = 0.05, 1.5, 0.01
    St = torch.tensor([S], dtype=torch.float64, device=_dev())
    lr_t = (_f64(lr) * torch.minimum(_f64(max_norm) / (torch.sqrt(St[0]) + _f64(TINY)), _f64(1.0))).float()
    want = _want_update(d, lr_t, wd, with_vs)
    ko.multi_param_update(d["p"], d["g"], d["v"] if with_vs else None, lr, St, max_norm, TINY, weight_decay=wd)
    _assert_bits(d["p"], want, "clipped update with decay")
    if math.isnan(S):                              # a NaN norm makes every parameter NaN, as without decay
        assert all(bool(torch.isnan(p).all()) for p in d["p"])


@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("which", ["edges", "unaligned"])
def test_zero_decay_gives_the_bits_of_the_plain_update(ko, which, with_vs):
    """psgd_multi_param_update_wd_f32 with wd == 0, called directly, against the wrapper's psgd_multi_param_update_f32"""
    from psgd_tf_amd import _lib
    a, b = mt._make(which, 33, ("p", "g", "v")), mt._make(which, 33, ("p", "g", "v"))
    vs_a, vs_b = (a["v"], b["v"]) if with_vs else (None, None)
    ko.multi_param_update(a["p"], a["g"], vs_a, 0.0371)
    (ps, gs, vs), plan = ko._lists("test", ("p", b["p"]), ("g", b["g"]), ("v", vs_b))
    rc = _lib.load().psgd_multi_param_update_wd_f32(
        plan.table("params", ps, "test"), plan.table("grads", gs, "test"), None if vs is None else plan.table("vs", vs, "test"),
        len(ps), plan.chunks.data_ptr(), plan.nchunks, 0.0371, None, 0.0, TINY, 0.0, ko._psgd._stream_ptr(plan.device))
    assert rc == _lib.PSGD_OK
    _assert_bits(b["p"], a["p"], "wd == 0")


def test_update_refuses_decay_on_the_perturbation(ko):
    d = mt._make("empty_middle", 34, ("p", "v"), plant=False)
    with pytest.raises(ValueError, match="no weight_decay"):
        ko.multi_param_update(d["p"], None, d["v"], weight_decay=0.1)


# --------------------------------------------------------------------------------------------------------------- first call
def test_first_calls_on_poisoned_buffers(ko):
    """the momentum buffers and the plan's flag word hold 0xFF bytes before the first call: the first blend (beta_0 = 0) does not
    read the buffers, the check neither reads nor clears the word; the same calls run a second time behave alike"""
    d = _make_dyadic("unaligned", 41, ("m", "g", "h"))
    plan = ko.MultiTailPlan([int(m.numel()) for m in d["m"]], _dev())                # a plan of its own: its stamps start at 1
    plan.flag.fill_(-1)
    for m in d["m"]:
        m.view(torch.int32).fill_(-1)
    g0 = [g.clone() for g in d["g"]]
    for round_ in range(2):
        beta = 0.0 if round_ == 0 else 0.5
        want = [g * 1.0 for g in d["g"]] if round_ == 0 else [m * 0.5 + g * 0.5 for m, g in zip(d["m"], d["g"])]
        ko.multi_blend(d["m"], d["g"], beta, 1.0 - beta, plan=plan)
        _assert_bits(d["m"], want, "blend, call %d" % round_)
        held = int(plan.flag.item())
        stamp = plan.next_stamp()
        assert stamp == round_ * 2 + 1 and held != stamp
        ko.multi_scale_check([d["g"], d["h"]], [1.0, 1.0], flag=plan.flag, stamp=stamp, plan=plan)
        assert int(plan.flag.item()) == held                                        # clean: the word keeps what it held (-1 at first)
        d["h"][1].view(-1)[5] = float("nan")
        stamp = plan.next_stamp()
        ko.multi_scale_check([d["g"], d["h"]], [1.0, 1.0], flag=plan.flag, stamp=stamp, plan=plan)
        assert int(plan.flag.item()) == stamp
        d["h"][1].view(-1)[5] = 0.0
    _assert_bits(d["g"], g0, "gradients")


def test_the_stamp_counter_wraps_to_one(ko):
    (_,), plan = ko._lists("test", ("x", [torch.zeros(3, device=_dev())]))
    plan.stamp = 2 ** 31 - 2
    assert plan.next_stamp() == 2 ** 31 - 1 and plan.next_stamp() == 1 and plan.next_stamp() == 2
