"""mixed_dtypes= (one optimizer over float32, bfloat16 and float16 parameters) without a device: the keyword checks, which all come
before a device is touched (the parameters here are CPU tensors, which no constructor accepts once it looks), the per-dtype
sub-plans of the chunk table, the shared constants and the launch-count formula.

The standard mixed list: sizes 1, 7, 4095, 4096, 4097, 8200, 3 (both sides of the 4096-element chunk, a multi-chunk tensor with a
ragged last chunk), dtypes interleaved fp32, bf16, fp16, bf16, fp32, fp16, bf16."""
import itertools

import numpy as np
import pytest
import torch

from psgd_tf_amd import _lib
from psgd_tf_amd import preconditioned_stochastic_gradient_descent as psgd

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
SIZES = [1, 7, 4095, 4096, 4097, 8200, 3]
DTYPES = [F32, BF16, F16, BF16, F32, F16, BF16]
CODES = {F32: _lib.DTYPE_F32, BF16: _lib.DTYPE_BF16, F16: _lib.DTYPE_F16}
CLASSES = {
    "UVd": lambda ps, **kw: psgd.UVd(ps, rank_of_modification=2, placement=None, **kw),
    "SPLU": lambda ps, **kw: psgd.SPLU(ps, rank_of_modification=2, **kw),
    "Dense": lambda ps, **kw: psgd.Dense(ps, **kw),
    "Kron": lambda ps, **kw: psgd.Kron(ps, any_rank=True, **kw),
}


def _params(dtypes, sizes=None):
    """CPU tensors: a constructor that reaches a device check refuses them, so whatever is raised before is raised before a device
    is touched"""
    sizes = [4] * len(dtypes) if sizes is None else sizes
    return [torch.zeros(n, dtype=dt, requires_grad=True) for n, dt in zip(sizes, dtypes)]


# ------------------------------------------------------------------------------------------------------------- keyword checks
@pytest.mark.parametrize("kind", list(CLASSES))
@pytest.mark.parametrize("bad", [1, 0, "yes", None, np.bool_(True)], ids=repr)
def test_a_switch_that_is_not_a_bool_is_refused(kind, bad):
    with pytest.raises(ValueError, match="mixed_dtypes must be True or False"):
        CLASSES[kind](_params([F32, BF16]), mixed_dtypes=bad)


def test_the_switch_is_keyword_only_and_off_by_default():
    import inspect
    for cls in (psgd.UVd, psgd.SPLU, psgd.Dense, psgd.Kron):
        p = inspect.signature(cls.__init__).parameters["mixed_dtypes"]
        assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default is False, cls


def test_kron_with_the_switch_off_refuses_a_mixed_list_as_before():
    with pytest.raises(TypeError, match="like parameter 0"):
        psgd.Kron(_params([F32, BF16]), any_rank=True)
    with pytest.raises(TypeError, match="like parameter 0"):
        psgd.Kron(_params([F32, BF16]), any_rank=True, mixed_dtypes=False)


@pytest.mark.parametrize("kind", list(CLASSES))
def test_a_dtype_outside_the_three_is_refused(kind):
    with pytest.raises(TypeError, match="float32"):
        CLASSES[kind](_params([F32, torch.float64]), mixed_dtypes=True)


@pytest.mark.parametrize("kind", list(CLASSES))
@pytest.mark.parametrize("dtypes", [[BF16, F16], [F32, F16], [F16, F32, BF16]], ids=lambda d: "-".join(str(x)[6:] for x in d))
def test_stochastic_rounding_refuses_float16_and_a_list_without_bfloat16(kind, dtypes):
    with pytest.raises(ValueError, match="param_rounding='stochastic'"):
        CLASSES[kind](_params(dtypes), mixed_dtypes=True, param_rounding="stochastic")


@pytest.mark.parametrize("kind", ["UVd", "SPLU"])
def test_state_dtype_param_is_ambiguous_with_two_dtypes(kind):
    with pytest.raises(ValueError, match="state_dtype='param' is ambiguous"):
        CLASSES[kind](_params([BF16, F32]), mixed_dtypes=True, state_dtype="param")


def test_uvd_tail_plan_refuses_a_wrong_dtype_list():
    with pytest.raises(ValueError, match="dtypes for"):
        psgd.UVdTailPlan([3, 4], [F32], "cpu")
    with pytest.raises(TypeError, match="float32, bfloat16 or float16"):
        psgd.UVdTailPlan([3, 4], [F32, torch.float64], "cpu")


# --------------------------------------------------------------------------------------------------------------- the sub-plans
def _rows(chunks):
    return [] if chunks is None else [tuple(r) for r in chunks.cpu().numpy().tolist()]


def test_the_dtype_sub_plans_partition_the_chunk_table():
    plan = psgd.UVdTailPlan(SIZES, DTYPES, "cpu")
    whole = [tuple(r) for r in psgd.uvd_tail_chunks(SIZES).tolist()]
    assert plan.mixed and plan.dtype is None and plan.code is None and _rows(plan.chunks) == whole
    assert [c for c, _, _ in plan.by_dtype] == [CODES[F32], CODES[BF16], CODES[F16]]
    seen = []
    for code, chunks, n in plan.by_dtype:
        rows = _rows(chunks)
        assert n == len(rows) > 0
        assert all(CODES[DTYPES[seg]] == code for seg, _ in rows)                        # a launch meets its own dtype only
        assert rows == [r for r in whole if CODES[DTYPES[r[0]]] == code]                # the plan's rows, in the plan's order
        seen += rows
    assert sorted(seen) == sorted(whole) and len(set(seen)) == len(whole)                # every chunk in exactly one
    assert plan.starts == list(np.cumsum([0] + SIZES[:-1])) and plan.sizes == tuple(SIZES)   # the segments are untouched
    assert plan.dtype_chunks(None) is plan.by_dtype                                      # built at construction, kept


def test_the_group_dtype_sub_plans_partition_each_group():
    plan = psgd.UVdTailPlan(SIZES, DTYPES, "cpu")
    whole = [tuple(r) for r in psgd.uvd_tail_chunks(SIZES).tolist()]
    groups = [(0, 3, 5), (2,), (1, 4, 6)]                                               # they cut across the dtypes
    for g in groups:
        mine = _rows(plan.group_chunks(g)[0])
        assert mine == [r for r in whole if r[0] in g]
        subs = plan.dtype_chunks(g)
        assert plan.dtype_chunks(g) is subs                                              # cached like group_chunks
        assert [c for c, _, _ in subs] == sorted({CODES[DTYPES[i]] for i in g})
        got = []
        for code, chunks, n in subs:
            rows = _rows(chunks)
            assert n == len(rows) and rows == [r for r in mine if CODES[DTYPES[r[0]]] == code]
            got += rows
        assert sorted(got) == sorted(mine)


def test_a_pair_without_a_chunk_is_not_launched():
    plan = psgd.UVdTailPlan([0, 5, 0], [F16, BF16, F32], "cpu")
    assert plan.mixed and [c for c, _, _ in plan.by_dtype] == [CODES[BF16]]
    assert plan.dtype_chunks((0, 2)) == []


def test_a_one_dtype_plan_is_the_plan_it_was():
    for spec in (BF16, [BF16] * len(SIZES)):
        plan = psgd.UVdTailPlan(SIZES, spec, "cpu")
        assert not plan.mixed and plan.dtype == BF16 and plan.code == CODES[BF16]
        (code, chunks, n), = plan.by_dtype
        assert code == CODES[BF16] and chunks is plan.chunks and n == plan.nchunks
        (code, chunks, n), = plan.dtype_chunks((1, 2))
        assert chunks is plan.group_chunks((1, 2))[0] and len(plan._group_chunks) == 1   # the group's own table, nothing new
    assert psgd.UVdTailPlan(SIZES, BF16, "cpu").tiny == torch.finfo(BF16).tiny


# ---------------------------------------------------------------------------------------------------------- shared constants
def test_tiny_and_delta_are_the_maxima_whatever_the_order():
    want = (torch.finfo(F16).tiny, torch.finfo(BF16).eps ** 0.5)
    for perm in itertools.permutations([F32, BF16, F16]):
        assert psgd.mixed_dtype_constants(perm) == want
        assert psgd.UVdTailPlan([2, 2, 2], list(perm), "cpu").tiny == want[0]
    assert psgd.mixed_dtype_constants([F32, BF16]) == (torch.finfo(F32).tiny, torch.finfo(BF16).eps ** 0.5)
    assert psgd.mixed_dtype_constants([BF16, F32]) == psgd.mixed_dtype_constants([F32, BF16])
    assert psgd.mixed_dtype_constants([F32, F16]) == (torch.finfo(F16).tiny, torch.finfo(F16).eps ** 0.5)
    for dt in (F32, BF16, F16):                                                          # one dtype: today's values
        assert psgd.mixed_dtype_constants([dt, dt]) == (torch.finfo(dt).tiny, torch.finfo(dt).eps ** 0.5)


# ------------------------------------------------------------------------------------------------------------ launch counts
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("G", [1, 3])
def test_the_launch_count_formula(D, G):
    """(packs x D) + sums + the (group, dtype) pairs that hold an element, counted against the sub-plans themselves"""
    dtypes = [[F32, BF16, F16][i % D] for i in range(len(SIZES))]
    groups = None if G == 1 else [(0, 3, 5), (2,), (1, 4, 6)]
    plan = psgd.UVdTailPlan(SIZES, dtypes, "cpu")
    pairs = sum(len(plan.dtype_chunks(g)) for g in (groups or [None]))
    assert len(plan.by_dtype) == D
    for packs, sums in ((3, 1), (1, 2), (0, 0)):
        assert psgd.tail_launch_count(dtypes, SIZES, groups, packs=packs, sums=sums) == packs * D + sums + pairs
    if G == 1:
        assert pairs == D
    else:
        assert pairs == {1: 3, 2: 5, 3: 5}[D]                # D >= 2: {0,3,5} and {1,4,6} hold two dtypes each, {2} one
    # an empty tensor brings no launch
    assert psgd.tail_launch_count([F32, F16], [5, 0], packs=1, sums=1) == 1 + 1 + 1
