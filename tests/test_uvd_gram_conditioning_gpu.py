"""GPU: the r x r solves of the UVd update (psgd.py:574-578, K = I + V'U, one adjoint and one plain solve) on Grams that force row
exchanges and on ill-conditioned ones, through every solver the project has: lu_solve_rows (one row per lane; ranks <= 32 and the
whole-matrix kernels of ranks 33 .. 64), lu_solve_block (psgd_set_tuning(2, 1)), the Gauss-Jordan of the bf16-state kernels and the
device solve of the column-chunk / row-sharded wide route.  The problems of tests/uvd_cases.py (gram_case, exact_case) have the K they
claim: tests/test_uvd_gram_cases_cpu.py asserts their exchange counts and condition numbers without a GPU.

Reference: oracle.psgd_oracle.update_precond_UVd_math_ in fp64 on the same fp32 inputs.  Bars: those of tests/test_uvd_gpu.py, hard --
state 1e-5 (ranks above 32: 2e-5), increment of the rewritten factor and of d 2e-3, apply 1e-5 -- for every kind but cond1e3 and
cond1e4.  For these two the state bars stay; the increment bar is err <= 2 err_fp32_oracle + 2e-3, err_fp32_oracle = the distance of
the same NumPy oracle run on float32 arrays from the fp64 one (what fp32 storage of the inputs and intermediates alone costs; the
factor 2 allows another, equally valid summation order in the Gram).  No sensitivity relaxation of any kind.
bf16 state: the bars of tests/test_uvd_bf16_gpu.py through check_bf16_state, kinds GRAM_KINDS_BF16.
Set PSGD_UVD_GRAM_OUT to a file name to collect one line per (route, shape, kind, branch): cond(K), exchanges, errors."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from tests import uvd_cases as uc
from tests.test_sharded_gpu import _gather_fold_emulated
from tests.uvd_cases import TINY32, check_bf16_state, rel_err, to_bf16_np

pytestmark = pytest.mark.gpu

APPLY_TOL = 1e-5
STATE_TOL = 1e-5
INCR_TOL = 2e-3
STEP = 0.01
RELATIVE_KINDS = ("cond1e3", "cond1e4")

LE32 = [(1021, 1)] + uc.GRAM_SHAPES_LE32
WIDE = uc.GRAM_SHAPES_WIDE + [uc.GRAM_SHAPE_FEW_ROWS]
CHUNK = uc.GRAM_SHAPES_CHUNK


def _cases(shapes, kinds=uc.GRAM_KINDS):
    return [pytest.param(N, r, k, id="%d-%d-%s" % (N, r, k)) for N, r in shapes for k in kinds if r > 1 or k.startswith("cond")]


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import preconditioned_stochastic_gradient_descent as m
    assert torch.cuda.is_available()
    return m


def _t(a):
    return torch.tensor(np.asarray(a)).cuda()          # (a copy: the shared problems are read-only arrays)


def _to_dev(p):
    return {k: _t(v) for k, v in p.items()}


def _record(line):
    path = os.environ.get("PSGD_UVD_GRAM_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@functools.lru_cache(maxsize=None)
def _problem(N, r, kind):
    p = uc.exact_case(N, r, kind) if kind in uc.exact_gram_kinds(r) else uc.gram_case(N, r, kind)
    for a in p.values():
        a.setflags(write=False)
    return p


def _errors(got, q, p, update_U):
    """(largest state error over U, V, d; {tensor: increment error} of the rewritten factor and d)"""
    st = max(rel_err(got[k], q[k]) for k in ("U", "V", "d"))
    inc = {k: rel_err(got[k].astype(np.float64) - p[k], q[k] - p[k].astype(np.float64)) for k in (("U" if update_U else "V"), "d")}
    return st, inc


@functools.lru_cache(maxsize=None)
def _ref(N, r, kind, update_U):
    """Computed once per case and shared: the fp64 oracle's state and apply, the fp32 oracle's errors against it, cond(K), exchanges."""
    p = _problem(N, r, kind)
    q = {k: v.astype(np.float64) for k, v in p.items()}
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=False, update_U=update_U)
    f = {k: v.copy() for k, v in p.items()}
    orc.update_precond_UVd_math_(f["U"], f["V"], f["d"], f["v"], f["h"], STEP, TINY32, balance=False, update_U=update_U)
    assert f["U"].dtype == np.float32 and f["d"].dtype == np.float32
    st32, inc32 = _errors(f, q, p, update_U)
    K = uc.gram_of(p)
    return dict(q=q, apply=orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"]), st32=st32, inc32=inc32,
                cond=float(np.linalg.cond(K)), ex=(uc.lu_exchanges(K), uc.lu_exchanges(K.T)))


def _judge(route, N, r, kind, update_U, t, out=None):
    """the state in t (device tensors after the call) and the fused call's gradient against the bars of the module docstring"""
    p, ref = _problem(N, r, kind), _ref(N, r, kind, update_U)
    got = {k: t[k].cpu().numpy() for k in ("U", "V", "d")}
    st, inc = _errors(got, ref["q"], p, update_U)
    e_out = rel_err(out.cpu().numpy(), ref["apply"]) if out is not None else float("nan")
    line = ("%-9s N=%d r=%d %-10s update_%s cond %.3g exchanges K %d K' %d | kernel state %.2e inc %.2e apply %.2e | fp32 oracle state "
            "%.2e inc %.2e" % (route, N, r, kind, "U" if update_U else "V", ref["cond"], ref["ex"][0], ref["ex"][1], st,
                               max(inc.values()), e_out, ref["st32"], max(ref["inc32"].values())))
    print(line)
    _record(line)
    frozen = "V" if update_U else "U"
    assert np.array_equal(got[frozen], p[frozen]), line                          # only one factor changes (psgd.py:586)
    assert st < (2 * STATE_TOL if r > 32 else STATE_TOL), line
    for k, e in inc.items():
        bar = 2 * ref["inc32"][k] + INCR_TOL if kind in RELATIVE_KINDS else INCR_TOL
        assert e < bar, (line, k, e, bar)
    if out is not None:
        assert e_out < APPLY_TOL, line


# ------------------------------------------------------------------------------------------------ fp32 state, one GPU
@pytest.mark.parametrize("N,r,kind", _cases(LE32 + WIDE + CHUNK))
def test_update(psgd, N, r, kind):
    """update_precond_UVd_math_, default tuning: lu_solve_rows at RG = 8 .. 32 (r <= 32), at widths 40 / 48 / 56 / 64 (r = 33 .. 64),
    the device solve of the column chunks above"""
    for upd in (True, False):
        t = _to_dev(_problem(N, r, kind))
        assert psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=False, update_U=upd) is None
        _judge("update", N, r, kind, upd, t)


@pytest.mark.parametrize("N,r,kind", _cases(LE32))
def test_update_block_reference(psgd, hip_lib, N, r, kind):
    """the same call on lu_solve_block (psgd_set_tuning(2, 1)): against the oracle, not only against the register form"""
    for upd in (True, False):
        t = _to_dev(_problem(N, r, kind))
        try:
            assert hip_lib.psgd_set_tuning(2, 1) == 0
            psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=False, update_U=upd)
            torch.cuda.synchronize()
        finally:
            hip_lib.psgd_set_tuning(2, 0)
        _judge("block", N, r, kind, upd, t)


@pytest.mark.parametrize("N,r,kind", _cases(LE32 + WIDE + CHUNK))
def test_fused(psgd, N, r, kind):
    """update_precond_UVd_math_and_precond_grad: the state, and the gradient against the oracle's apply on the updated fp64 state"""
    for upd in (True, False):
        t = _to_dev(_problem(N, r, kind))
        out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32,
                                                            balance=False, update_U=upd)
        assert out.shape == t["g"].shape and out.dtype == torch.float32
        _judge("fused", N, r, kind, upd, t, out)


@pytest.mark.parametrize("N,r", [(1021, 32), (2049, 64), (2049, 100)])
@pytest.mark.parametrize("kind", ("cyclic", "cond1e3"))
@pytest.mark.parametrize("fused", (0, 1))
def test_balance_keeps_the_pivots(psgd, N, r, kind, fused):
    """balance=True with U scaled by 4 and V by 1/4 (rho = 4): the rescaling leaves K = I + V'U as it is -- exactly, the factors are
    powers of two -- so the r - 1 exchanges of `cyclic` (and the condition number of `cond1e3`) must survive it"""
    p = {k: v.copy() for k, v in _problem(N, r, kind).items()}
    p["U"] *= 4.0
    p["V"] *= 0.25
    K = uc.gram_of(p)
    assert np.array_equal(K, uc.gram_of(_problem(N, r, kind)))
    for upd in (True, False):
        t, q, f = _to_dev(p), {k: v.astype(np.float64) for k, v in p.items()}, {k: v.copy() for k, v in p.items()}
        out = None
        if fused:
            out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32,
                                                                balance=True, update_U=upd)
        else:
            psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=True, update_U=upd)
        for x in (q, f):                                   # the fp64 oracle, and the same oracle on float32 arrays
            orc.update_precond_UVd_math_(x["U"], x["V"], x["d"], x["v"], x["h"], STEP, TINY32, balance=True, update_U=upd)
        got = {k: t[k].cpu().numpy() for k in ("U", "V", "d")}
        # the increment over the balanced base (U / rho, V rho: exact)
        base = {k: p[k].astype(np.float64) * s for k, s in ((("U", 0.25) if upd else ("V", 4.0)), ("d", 1.0))}
        st, st32 = (max(rel_err(x[k], q[k]) for k in ("U", "V", "d")) for x in (got, f))
        inc, inc32 = ({k: rel_err(x[k] - b, q[k] - b) for k, b in base.items()} for x in (got, f))
        e_out = rel_err(out.cpu().numpy(), orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])) if fused else float("nan")
        line = ("%-9s N=%d r=%d %-10s update_%s cond %.3g exchanges K %d K' %d | kernel state %.2e inc %.2e apply %.2e | fp32 oracle "
                "state %.2e inc %.2e" % ("balance-" + ("fused" if fused else "update"), N, r, kind, "U" if upd else "V",
                                         np.linalg.cond(K), uc.lu_exchanges(K), uc.lu_exchanges(K.T), st, max(inc.values()), e_out,
                                         st32, max(inc32.values())))
        print(line)
        _record(line)
        assert st < (2 * STATE_TOL if r > 32 else STATE_TOL), line
        for k, e in inc.items():
            assert e < (2 * inc32[k] + INCR_TOL if kind in RELATIVE_KINDS else INCR_TOL), (line, k, e)
        if fused:
            assert e_out < APPLY_TOL, line


# ------------------------------------------------------------------------------------------------ bf16 state (Gauss-Jordan on [K | I])
def _bf16_dev(p):
    return {k: (_t(a).to(torch.bfloat16) if k in ("U", "V", "d") else _t(a)) for k, a in p.items()}


@pytest.mark.parametrize("fused", (0, 1))
@pytest.mark.parametrize("rounding", ("nearest", "stochastic"))
@pytest.mark.parametrize("N,r,kind", _cases(uc.GRAM_SHAPES_LE32, uc.GRAM_KINDS_BF16) + _cases(uc.EXACT_SHAPES_BF16, uc.EXACT_KINDS_BF16))
def test_bf16_state(psgd, N, r, kind, rounding, fused):
    """U, V, d rounded to bf16 first (the K of the rounded codes keeps its exchanges and its condition number: the CPU self-check), the
    oracle on the widened codes, check_bf16_state unchanged: the element bound, p_native <= 2 p_widen + 1e-4.
    The exact kinds (ties, ties_late, zeropivot; r = 8, 16, 32): every entry of U and V is a bf16 number, so the rounding changes
    nothing and the Gauss-Jordan of psgd_uvd_bf16.hip gets K == A bit for bit.  On zeropivot every pivot candidate on the diagonal is
    exactly zero: a Gauss-Jordan whose pivot search or row swap does nothing divides by zero there and misses the element bound."""
    p = {k: (to_bf16_np(v.copy()) if k in ("U", "V", "d") else v) for k, v in _problem(N, r, kind).items()}
    if kind in uc.EXACT_KINDS_BF16:
        assert all(np.array_equal(p[k], _problem(N, r, kind)[k]) for k in ("U", "V"))
        assert np.array_equal(uc.gram_of(p), uc.exact_gram_kinds(r)[kind])
    for upd in (True, False):
        q = {k: v.astype(np.float64) for k, v in p.items()}
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=False, update_U=upd)
        w = _to_dev(p)                                     # the yardstick: the fp32 kernels on the widened inputs
        psgd.update_precond_UVd_math_(w["U"], w["V"], w["d"], w["v"], w["h"], STEP, TINY32, balance=False, update_U=upd)
        widen32 = {k: w[k].cpu().numpy() for k in ("U", "V", "d")}
        t = _bf16_dev(p)
        kw = dict(balance=False, update_U=upd, rounding=rounding, rounding_seed=77 + r)
        if fused:
            out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32, **kw)
        else:
            assert psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, **kw) is None
        assert all(t[k].dtype == torch.bfloat16 for k in ("U", "V", "d"))
        stored = {k: t[k].float().cpu().numpy().astype(np.float64) for k in ("U", "V", "d")}
        frozen = "V" if upd else "U"
        assert np.array_equal(stored[frozen], p[frozen].astype(np.float64))
        tag = "bf16-%s N=%d r=%d %s update_%s %s" % ("fused" if fused else "update", N, r, kind, "U" if upd else "V", rounding)
        pn, pw, worst = check_bf16_state(tag, stored, {k: q[k] for k in ("U", "V", "d")}, widen32, {"d", "U" if upd else "V"}, rounding)
        K = uc.gram_of(p)
        line = "%s cond %.3g exchanges K %d K' %d | p_native %.3e p_widen %.3e worst err/bound %.2f | fp32 kernels state %.2e" % (
            tag, np.linalg.cond(K), uc.lu_exchanges(K), uc.lu_exchanges(K.T), pn, pw, worst,
            max(rel_err(widen32[k], q[k]) for k in ("U", "V", "d")))
        print(line)
        _record(line)
        assert pn <= 2 * pw + 1e-4, line
        if fused:
            e = rel_err(out.cpu().numpy(), orc.precond_grad_UVd_math(stored["U"], stored["V"], stored["d"], q["g"]))
            assert e < APPLY_TOL, (line, e)


# ------------------------------------------------------------------------------------------------ two row shards in one process
@pytest.mark.parametrize("kind", ("cyclic", "cond1e2", "cond1e3"))
@pytest.mark.parametrize("fused", (0, 1))
def test_two_shards_rank32(psgd, kind, fused):
    """the harness of tests/test_sharded_gpu.py (each shard its own HipStages, the exchange emulated by concatenation + the product's
    fold kernel): a K folded from two partial Grams takes the same solve"""
    from psgd_tf_amd import sharded
    N, r, cut = 1021, 32, 448
    p = _problem(N, r, kind)
    for upd in (True, False):
        sh = [{k: _t(v[a:b]) for k, v in p.items()} for a, b in ((0, cut), (cut, N))]
        bes = [sharded.HipStages(torch.device("cuda:0"), s["U"].shape[0], r) for s in sh]
        for be, s in zip(bes, sh):
            be.update_sweep1(s["U"], s["V"], s["d"], s["v"], s["h"])
        _gather_fold_emulated(bes, 11)
        out = None
        if fused:
            for be, s in zip(bes, sh):
                be.update_sweep2_fused(s["U"], s["V"], s["d"], s["v"], s["h"], s["g"], STEP, TINY32, upd)
            _gather_fold_emulated(bes, 13)
            for be in bes:
                be.fused_post(STEP, TINY32, upd)
            out = torch.cat([be.fused_final(s["U"], s["V"], s["d"], s["g"], STEP, TINY32) for be, s in zip(bes, sh)], 0)
        else:
            for be, s in zip(bes, sh):
                be.update_sweep2(s["U"], s["V"], s["d"], s["v"], s["h"], STEP, TINY32, upd)
            _gather_fold_emulated(bes, 12)
            for be, s in zip(bes, sh):
                be.update_sweep3(s["d"], STEP, TINY32)
        t = {k: torch.cat([s[k] for s in sh], 0) for k in ("U", "V", "d")}
        _judge("shards-" + ("fused" if fused else "update"), N, r, kind, upd, t, out)


def _wide_two_shards(psgd, p, cut, update_U, fused):
    """uvd_wide.update on two row shards in one process.  Its `reduce` callback is the exchange; the shards cannot run side by side
    here, so the sequence is repeated on fresh copies, each pass handing back the true totals of the exchanges whose partial results
    the earlier passes have recorded (exchange k depends on the totals of exchanges < k only) until every exchange was answered."""
    from psgd_tf_amd import uvd_wide
    N = p["U"].shape[0]
    totals = []
    while True:
        partial, shards, outs = [], [], []
        for a, b in ((0, cut), (cut, N)):
            s = {k: _t(v[a:b]) for k, v in p.items()}
            mine = []

            def reduce(t, op, mine=mine):
                mine.append((t.clone(), op))
                return totals[len(mine) - 1].clone() if len(mine) <= len(totals) else t
            outs.append(uvd_wide.update(s["U"], s["V"], s["d"], s["v"], s["h"], STEP, TINY32, False, update_U, psgd.uvd_workspace,
                                        reduce=reduce, fused_g=s["g"] if fused else None))
            partial.append(mine)
            shards.append(s)
        assert len(partial[0]) == len(partial[1]) and [op for _, op in partial[0]] == [op for _, op in partial[1]]
        if len(totals) == len(partial[0]):
            break
        (x, op), (y, _) = partial[0][len(totals)], partial[1][len(totals)]
        if op == "sum":
            tot = x + y
        elif op == "max":
            tot = torch.maximum(x, y)
        else:
            assert op == "summax"
            tot = torch.cat([x[:-1] + y[:-1], torch.maximum(x[-1:], y[-1:])])
        totals.append(tot)
    assert len(totals) >= 2
    t = {k: torch.cat([s[k] for s in shards], 0) for k in ("U", "V", "d")}
    return t, (torch.cat([o.reshape(-1, 1) for o in outs], 0) if fused else None)


@pytest.mark.parametrize("kind", ("cyclic", "cond1e2", "cond1e3"))
@pytest.mark.parametrize("fused", (0, 1))
def test_two_shards_rank64(psgd, kind, fused):
    """ranks above 32 on row shards (uvd_wide.update with a reduce: the building blocks and the device solve of K)"""
    N, r = 2049, 64
    for upd in (True, False):
        t, out = _wide_two_shards(psgd, _problem(N, r, kind), 960, upd, fused)
        _judge("shards-" + ("fused" if fused else "update"), N, r, kind, upd, t, out)


# ------------------------------------------------------------------------------------------------ exact Grams: ties, a singular K
@pytest.mark.parametrize("N,r", uc.EXACT_SHAPES)
@pytest.mark.parametrize("kind", ("ties", "ties_late", "zeropivot"))
def test_exact_ties(psgd, hip_lib, N, r, kind):
    """K == A bit for bit whatever the summation order.  ties, ties_late: at every step the candidates of the pivot column are of one
    size, and the documented difference in tie order from LAPACK must not show in the result.  zeropivot: every diagonal entry of K is
    exactly zero -- the one input on which a solver that never exchanges rows fails outright (it divides by zero; on a pivot that is only
    small an fp64 elimination loses ~1e-12, which no bar here sees).  Two-call and fused route at the hard bars; the
    register form and the block form agree to 1e-7 (r <= 32); a second run is bit-identical."""
    for upd in (True, False):
        runs = []
        for fused in (0, 1, 1, 0):
            t = _to_dev(_problem(N, r, kind))
            out = None
            if fused:
                out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32,
                                                                    balance=False, update_U=upd)
            else:
                psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=False, update_U=upd)
            runs.append((t, out))
        for (ta, oa), (tb, ob) in ((runs[0], runs[3]), (runs[1], runs[2])):
            for k in ("U", "V", "d"):
                assert torch.equal(ta[k], tb[k]), (k, upd)
            assert oa is None or torch.equal(oa, ob)
        _judge("update", N, r, kind, upd, runs[0][0])
        _judge("fused", N, r, kind, upd, *runs[1])
        if r <= 32:
            b = _to_dev(_problem(N, r, kind))
            try:
                assert hip_lib.psgd_set_tuning(2, 1) == 0
                psgd.update_precond_UVd_math_(b["U"], b["V"], b["d"], b["v"], b["h"], STEP, TINY32, balance=False, update_U=upd)
                torch.cuda.synchronize()
            finally:
                hip_lib.psgd_set_tuning(2, 0)
            for k in ("U", "V", "d"):
                assert rel_err(runs[0][0][k].cpu().numpy(), b[k].cpu().numpy()) < 1e-7, (k, upd)
            _judge("block", N, r, kind, upd, b)


@pytest.mark.parametrize("N,r", [(257, 8), (2049, 40)])
@pytest.mark.parametrize("update_U", (True, False))
def test_singular_gram_propagates_silently(psgd, N, r, update_U):
    """An exactly singular K (a zero row; np.linalg.solve refuses it, so there is no oracle to compare with): the call returns
    without an error code or an exception, and the rewritten factor and d are not all finite (the silent-propagation contract)."""
    p = _problem(N, r, "singular")
    K = uc.gram_of(p)
    assert np.linalg.matrix_rank(K) == r - 1 and not K[min(3, r - 1)].any()
    t = _to_dev(p)
    assert psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=False, update_U=update_U) is None
    torch.cuda.synchronize()
    assert not torch.isfinite(t["U" if update_U else "V"]).all()
    assert not torch.isfinite(t["d"]).all()
    assert torch.equal(t["V" if update_U else "U"], _t(p["V" if update_U else "U"]))
