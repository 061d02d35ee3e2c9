"""What the host layer of the three UVd operations (apply, update, fused update -> apply) decides before any kernel runs, pinned
on the CPU: how many numbers a call draws from the branch generator and in which order, and which exception a bad call raises.

Shapes: N = 130, r = 3 -- shard_rows(130, k, 3) gives two 64-row shards and a 2-row remainder, so the calls run on row counts
64, 64 and 2 with row0 = 0, 64 and 128.  One gloo process group of one rank, in this process; the stage backends are the NumPy
doubles of tests/cpu_stages.py and tests/cpu_stages_bf16.py.

The single-GPU entry points judge the rounding arguments before they look at a tensor, so a bad rounding and a rounding_seed
on an fp32 state are in the bad-call table although every tensor here is on the CPU.  Not in it, because no machine without a
GPU can tell them apart from a CPU-tensor error (such a call is wrong twice, and which of the two errors wins is not pinned):
the single-GPU entry points with r = 33 and a strided g on the product backend of the sharded path.  An fp32 `out` is not
forwarded to the fp32 NumPy double at all, so a wrongly shaped one is refused on the bf16 route only."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist

from psgd_tf_amd import _lib, sharded
from psgd_tf_amd import preconditioned_stochastic_gradient_descent as psgd
from tests.cpu_stages import NumpyStages
from tests.cpu_stages_bf16 import NumpyBf16Stages
from tests.uvd_cases import make_uvd_problem

N, R, WORLD = 130, 3, 3
TINY = float(np.finfo(np.float32).tiny)
STEP = 0.01
KINDS = {"fp32": (torch.float64, {}),                                   # (state dtype of the double, rounding keywords)
         "bf16-nearest": (torch.bfloat16, {"rounding": "nearest"}),
         "bf16-stochastic": (torch.bfloat16, {"rounding": "stochastic"})}


@pytest.fixture(scope="module")
def group():
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group("gloo", store=dist.FileStore(os.path.join(tmp, "store"), 1), rank=0, world_size=1)
        try:
            yield dist.group.WORLD
        finally:
            dist.destroy_process_group()


@pytest.fixture(scope="module")
def problem():
    return make_uvd_problem(N, R, seed=5, uv_gain=2.0, d_spread=0.3)


def _shard(p, k, state_dtype, vec_dtype=None):
    lo, hi = sharded.shard_rows(N, k, WORLD)
    vec_dtype = vec_dtype or (torch.float64 if state_dtype == torch.float64 else torch.float32)
    t = {key: torch.from_numpy(p[key][lo:hi].copy()).to(state_dtype if key in ("U", "V", "d") else vec_dtype) for key in p}
    return lo, t


def test_shards_are_two_of_64_rows_and_a_remainder():
    assert [sharded.shard_rows(N, k, WORLD) for k in range(WORLD)] == [(0, 64), (64, 128), (128, 130)]


@pytest.mark.parametrize("explicit", [(), ("balance",), ("update_U",), ("balance", "update_U")], ids=lambda e: "+".join(e) or "drawn")
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_draw_order(group, problem, kind, explicit):
    """the synchronised generator after every sharded update and fused call == a second generator from which the expected
    sequence is drawn by hand: rand (balance, p = 0.01), rand (update_U, p = 0.5), then randint(0, 2**62) for the seed of a
    stochastic rounding that got none; a value passed explicitly is not drawn.  What was drawn is what the stages were handed."""
    state_dtype, rounding_kw = KINDS[kind]
    bf16 = state_dtype == torch.bfloat16
    for k in range(WORLD):
        for fused in (False, True):
            for fixed in (False, True):
                lo, t = _shard(problem, k, state_dtype)
                be = NumpyBf16Stages(R) if bf16 else NumpyStages(R)
                gen, hand = torch.Generator().manual_seed(1000 + k), torch.Generator().manual_seed(1000 + k)
                kw = dict(rounding_kw, generator=gen, group=group, backend=be)
                kw.update({name: fixed for name in explicit})
                if bf16:
                    kw["row0"] = lo
                want_bal = fixed if "balance" in explicit else bool(torch.rand((), generator=hand).item() < 0.01)
                want_upd = fixed if "update_U" in explicit else bool(torch.rand((), generator=hand).item() < 0.5)
                want_seed = int(torch.randint(0, 2 ** 62, (), generator=hand).item()) if kind == "bf16-stochastic" else 0
                before = {key: t[key].clone() for key in ("U", "V")}
                x0 = sharded.EXCHANGES["count"]
                if fused:
                    out = sharded.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP,
                                                                           TINY, **kw)
                    assert out.shape == t["g"].shape
                else:
                    assert sharded.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY, **kw) is None
                tag = (kind, explicit, k, fused, fixed)
                synced = sharded.branch_rng_for(gen, group, None).gen if len(explicit) < 2 or kind == "bf16-stochastic" else gen
                assert torch.equal(synced.get_state(), hand.get_state()), tag
                assert sharded.EXCHANGES["count"] - x0 == (4 if bf16 and fused else 2) + int(want_bal), tag
                if not want_bal:                                              # the factor of the branch taken is the one rewritten
                    assert torch.equal(t["V" if want_upd else "U"], before["V" if want_upd else "U"]), tag
                    assert not torch.equal(t["U" if want_upd else "V"], before["U" if want_upd else "V"]), tag
                if bf16:
                    mode = psgd._ROUNDINGS[rounding_kw["rounding"]]
                    assert be.narrow_args == [("rewrite", mode, want_seed, lo), ("d", mode, want_seed, lo)], tag
                    assert (10 in be.log) == want_bal, tag


def test_row0_defaults_to_the_rows_before_this_rank(group, problem):
    _, t = _shard(problem, 2, torch.bfloat16)
    be = NumpyBf16Stages(R)
    sharded.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY, balance=False, update_U=True,
                                     group=group, backend=be, rounding="stochastic", rounding_seed=2 ** 64 + 77)
    assert be.narrow_args == [("rewrite", 1, 77, 0), ("d", 1, 77, 0)]      # one rank: nothing before it; the seed is taken mod 2**64


# ------------------------------------------------------------------------------------------------ bad calls
def _apply(mod):
    return lambda t, **kw: mod.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"], **kw)


def _update(mod):
    return lambda t, **kw: mod.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY, balance=False,
                                                        update_U=True, **kw)


def _fused(mod):
    return lambda t, **kw: mod.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP,
                                                                        TINY, balance=False, update_U=True, **kw)


ENTRY = {"apply": _apply, "update": _update, "fused": _fused}


def _mixed(t):
    return dict(t, V=t["V"].float())


def _fp16(t):
    return dict(t, U=t["U"].half(), V=t["V"].half(), d=t["d"].half())


def _rank33(t):
    n = t["U"].shape[0]
    return dict(t, U=torch.zeros(n, 33, dtype=torch.bfloat16), V=torch.zeros(n, 33, dtype=torch.bfloat16))


def _bad_out(t):
    return torch.empty(t["g"].shape[0] + 1, 1)


# (who, entry point, state, change of the tensors, keywords, exception); who: "cpu-backend" = sharded with the NumPy double,
# "product" = sharded with backend=None, "single" = the single-GPU function
BAD = [(who, op, state, None, {}, _lib.PsgdHipError)                                            # CPU tensor
       for who in ("product", "single") for op in ENTRY for state in ("fp32", "bf16")]
BAD += [(who, op, "bf16", _mixed, {}, TypeError) for who in ("cpu-backend", "product", "single") for op in ENTRY]
BAD += [(who, op, "bf16", _fp16, {}, TypeError) for who in ("product", "single") for op in ENTRY]
BAD += [("cpu-backend", op, "bf16", _rank33, {}, ValueError) for op in ENTRY]
BAD += [("cpu-backend", op, state, None, {"rounding": "up"}, ValueError) for op in ("update", "fused") for state in ("fp32", "bf16")]
BAD += [("cpu-backend", op, "fp32", None, kw, ValueError) for op in ("update", "fused")
        for kw in ({"rounding_seed": 3}, {"rounding": "stochastic"}, {"row0": 3}, {"row0": -1})]
BAD += [("cpu-backend", op, "bf16", None, {"row0": -1}, ValueError) for op in ("update", "fused")]
BAD += [("single", op, state, None, {"rounding": "up"}, ValueError) for op in ("update", "fused") for state in ("fp32", "bf16")]
BAD += [("single", op, "fp32", None, kw, ValueError) for op in ("update", "fused")
        for kw in ({"rounding_seed": 3}, {"rounding": "stochastic"})]
BAD += [("cpu-backend", "fused", "bf16", None, {"out": _bad_out}, ValueError)]


@pytest.mark.parametrize("who,op,state,change,kw,exc", BAD,
                         ids=["%s-%s-%s-%s" % (w, o, s, getattr(c, "__name__", None) or "-".join(sorted(k)) or "cpu")
                              for w, o, s, c, k, _ in BAD])
def test_bad_call(group, problem, who, op, state, change, kw, exc):
    double = who == "cpu-backend"
    _, t = _shard(problem, 1, torch.bfloat16 if state == "bf16" else torch.float64 if double else torch.float32,
                  None if double else torch.float32)
    if change is not None:
        t = change(t)
    kw = {k: (v(t) if callable(v) else v) for k, v in kw.items()}
    if who != "single":
        kw["group"] = group
    if double:
        kw["backend"] = NumpyBf16Stages(R) if state == "bf16" else NumpyStages(R)
    before = {k: v.clone() for k, v in t.items()}
    with pytest.raises(exc):
        ENTRY[op](psgd if who == "single" else sharded)(t, **kw)
    assert all(torch.equal(t[k], before[k]) for k in t)                       # refused before anything was written


def test_bad_narrow():
    dst, src = torch.zeros(N, dtype=torch.bfloat16), torch.zeros(N)
    with pytest.raises(_lib.PsgdHipError):
        psgd.uvd_bf16_narrow_(dst, src, tensor="d")                           # CPU tensors
    with pytest.raises(ValueError):
        psgd.uvd_bf16_narrow_(dst, src, tensor="Q")
    with pytest.raises(ValueError):
        psgd.uvd_bf16_narrow_(dst, src, tensor="d", rounding="up")
    with pytest.raises(TypeError):
        psgd.uvd_bf16_narrow_([0.0] * N, src, tensor="d")
