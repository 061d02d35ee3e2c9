"""multi_vec_precond_update / multi_vec_precond_grad (psgd_multi_vec_update_f32, psgd_multi_vec_apply_f32) on the GPU: every vector
against the fp64 oracle on its [1, n] view, the mechanics of the list (any k, more vectors than workgroups, one vector's bits do not
depend on its neighbours, repeatable, in place), and the non-finite contract.  The kernels have no scratch in memory (their folds
live in LDS); what a first call could read unwritten are the outputs of the apply, which are poisoned here."""
import numpy as np
import pytest
import torch

from tests import multi_vec_cases as mv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _dev_tensor(a, shift=0, shape=None):
    """a float32 device tensor with the values of `a` that starts `shift` floats past a 16-byte boundary (a contiguous slice)"""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    buf = torch.full((a.size + 4,), float("nan"), dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[shift:shift + a.size]
    t.copy_(torch.from_numpy(a.copy()))
    assert t.data_ptr() % 16 == 4 * shift and t.is_contiguous()
    return t if shape is None else t.view(shape)


def _lists(cases, shifts=(1, 2, 3, 0)):
    """(qls, qrs, dXs, dGs, gs) on the device from cases of mv.case; vector i starts shifts[i % 4] (+ 0, 1, 2 per operand) floats
    past a 16-byte boundary"""
    out = [[], [], [], [], []]
    for i, (ql, qr, dx, dg, g) in enumerate(cases):
        s = shifts[i % len(shifts)]
        out[0].append(_dev_tensor(ql, s % 4, (1, 1)))
        out[1].append(_dev_tensor(qr, s, (1, -1)))
        out[2].append(_dev_tensor(dx, (s + 1) % 4))
        out[3].append(_dev_tensor(dg, (s + 2) % 4))
        out[4].append(_dev_tensor(g, (s + 3) % 4))
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _np(t):
    return t.detach().cpu().numpy().reshape(-1).copy()


# ----------------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("state", mv.STATES)
def test_update_and_apply_against_the_fp64_oracle(psgd, state):
    """all lengths of one factor state in one list, no tensor 16-byte aligned except every fourth; factors within 1e-5, increments
    within 2e-3, the apply within 1e-5 of the oracle on the [1, n] view (relative, norm-wise, per factor)"""
    cases = [mv.case(n, state) for n in mv.LENGTHS]
    qls, qrs, dXs, dGs, gs = _lists(cases)
    outs = [torch.full_like(g, float("nan")) for g in gs]                          # poisoned: nothing reads them before writing
    psgd.multi_vec_precond_grad(qls, qrs, gs, outs)
    psgd.multi_vec_precond_update(qls, qrs, dXs, dGs, mv.STEP)
    torch.cuda.synchronize()
    for n, (ql, qr, dx, dg, g), q0, q1, out in zip(mv.LENGTHS, cases, qls, qrs, outs):
        e_fac, e_inc = mv.update_errors(float(q0), _np(q1), ql, qr, dx, dg)
        e_app = mv.rel(_np(out), mv.oracle_apply(ql, qr, g))
        print("%-7s n = %5d: factors %.2e, increments %.2e, apply %.2e" % (state, n, e_fac, e_inc, e_app))
        assert e_fac < mv.BAR_FACTORS and e_inc < mv.BAR_INCREMENT and e_app < mv.BAR_APPLY, (n, state, e_fac, e_inc, e_app)


def test_twenty_chained_updates_stay_with_the_oracle(psgd):
    """the kernel's own state after 20 chained updates, each with a new pair (dx, dg), against the fp64 oracle chained on the same
    pairs: within 1e-5, and the apply with that state too"""
    ns = (3, 65, 257, 1025, 4099)
    rng = np.random.default_rng(7)
    hs = [np.exp(rng.uniform(-1.0, 1.0, n)) for n in ns]
    qls = [torch.ones(1, 1, device=_dev()) for _ in ns]
    qrs = [_dev_tensor(np.ones(n), 1, (1, -1)) for n in ns]
    ref = [(1.0, np.ones(n)) for n in ns]
    for _ in range(20):
        pairs = [(lambda dx: (dx.astype(np.float32), (h * dx + 0.1 * rng.standard_normal(dx.size)).astype(np.float32)))
                 (rng.standard_normal(n)) for n, h in zip(ns, hs)]
        psgd.multi_vec_precond_update(qls, qrs, [_dev_tensor(p[0], 2) for p in pairs], [_dev_tensor(p[1], 3) for p in pairs], mv.STEP)
        ref = [mv.oracle_update(r[0], r[1], p[0], p[1], mv.STEP) for r, p in zip(ref, pairs)]
    gs = [rng.standard_normal(n).astype(np.float32) for n in ns]
    outs = psgd.multi_vec_precond_grad(qls, qrs, [_dev_tensor(g) for g in gs], [torch.full((n,), float("nan"), device=_dev()) for n in ns])
    for n, q0, q1, r, g, out in zip(ns, qls, qrs, ref, gs, outs):
        errs = (mv.rel(float(q0), r[0]), mv.rel(_np(q1), r[1]), mv.rel(_np(out), mv.oracle_apply(r[0], r[1], g)))
        print("n = %4d after 20 chained updates: ql %.2e, qr %.2e, apply %.2e" % ((n,) + errs))
        assert max(errs) < 1e-5, (n, errs)


# ------------------------------------------------------------------------------------------------------------- list mechanics
MIXED = (2, 3, 5, 64, 65, 257, 1025, 4099)                 # few distinct lengths: the calls on single vectors share their plans


def _mixed_cases(k):
    return [mv.case(MIXED[(i * 5 + i // 8) % len(MIXED)], mv.STATES[i % 3], seed=i) for i in range(k)]


def _run(psgd, cases, idx=None):
    """update and apply of the list (or of the vectors idx alone, one call each); returns per vector (ql bits, qr bits, out bits)"""
    qls, qrs, dXs, dGs, gs = _lists(cases)
    outs = [torch.full_like(g, float("nan")) for g in gs]
    if idx is None:
        psgd.multi_vec_precond_grad(qls, qrs, gs, outs)
        psgd.multi_vec_precond_update(qls, qrs, dXs, dGs, mv.STEP)
        idx = range(len(cases))
    else:
        for i in idx:
            psgd.multi_vec_precond_grad(qls[i:i + 1], qrs[i:i + 1], gs[i:i + 1], outs[i:i + 1])
            psgd.multi_vec_precond_update(qls[i:i + 1], qrs[i:i + 1], dXs[i:i + 1], dGs[i:i + 1], mv.STEP)
    torch.cuda.synchronize()
    return {i: (_bits(qls[i]), _bits(qrs[i]), _bits(outs[i])) for i in idx}


def _assert_same_bits(a, b, what):
    for i in b:
        for x, y, name in zip(a[i], b[i], ("ql", "qr", "out")):
            assert np.array_equal(x, y), "%s: %s of vector %d differs" % (what, name, i)


@pytest.mark.parametrize("k", [1, 3, 300])
def test_list_mechanics(psgd, k):
    cases = _mixed_cases(k)
    whole = _run(psgd, cases)
    _assert_same_bits(_run(psgd, cases), whole, "two calls on equal inputs")
    alone = _run(psgd, cases, idx=range(k) if k <= 3 else list(range(0, k, 7)) + [k - 1])
    _assert_same_bits(whole, alone, "a vector of a list of %d against the same vector alone" % k)
    # the same values at other addresses and alignments: still the same bits
    qls, qrs, dXs, dGs, gs = _lists(cases, shifts=(0, 3, 1, 2))
    psgd.multi_vec_precond_grad(qls, qrs, gs, gs)                                  # in place
    psgd.multi_vec_precond_update(qls, qrs, dXs, dGs, mv.STEP)
    torch.cuda.synchronize()
    moved = {i: (_bits(qls[i]), _bits(qrs[i]), _bits(gs[i])) for i in range(k)}
    _assert_same_bits(moved, whole, "in-place apply, other alignments")
    for i in range(k):
        assert np.isfinite(_np(qrs[i])).all() and not np.array_equal(_np(qrs[i]), cases[i][1])      # finite, and it did move


def test_more_vectors_than_workgroups(psgd):
    """2 050 vectors of length 5: the grid is capped at 2 048 workgroups, so two of them take a second vector"""
    k, n = 2050, 5
    rng = np.random.default_rng(3)
    ql = np.exp(rng.uniform(-1, 1, k)).astype(np.float32)
    qr, dx, g = (f(size=(k, n)).astype(np.float32) for f in (lambda size: np.exp(rng.uniform(-1, 1, size)), rng.standard_normal,
                                                            rng.standard_normal))
    dg = (1.5 * dx + 0.1 * rng.standard_normal((k, n))).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).to(_dev())
    QL, QR, DX, DG, G = dev(ql), dev(qr), dev(dx), dev(dg), dev(g)
    OUT = torch.full_like(G, float("nan"))
    rows = lambda T: list(T.unbind(0))                                             # views of one storage: rows start at 20-byte steps
    psgd.multi_vec_precond_grad(rows(QL.view(k, 1)), rows(QR), rows(G), rows(OUT))
    psgd.multi_vec_precond_update(rows(QL.view(k, 1)), rows(QR), rows(DX), rows(DG), mv.STEP)
    torch.cuda.synchronize()
    new_ql, new_qr, out = QL.cpu().numpy(), QR.cpu().numpy(), OUT.cpu().numpy()
    worst = [0.0, 0.0, 0.0]
    for i in range(k):
        e = mv.update_errors(new_ql[i], new_qr[i], ql[i], qr[i], dx[i], dg[i]) + (mv.rel(out[i], mv.oracle_apply(ql[i], qr[i], g[i])),)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert e[0] < mv.BAR_FACTORS and e[1] < mv.BAR_INCREMENT and e[2] < mv.BAR_APPLY, (i, e)
    print("2050 vectors of length 5: worst factors %.2e, increments %.2e, apply %.2e" % tuple(worst))


def test_wrappers_refuse_short_vectors_and_mismatched_lists(psgd):
    q = torch.ones(1, 1, device=_dev())
    v1, v5, v6 = (torch.ones(n, device=_dev()) for n in (1, 5, 6))
    with pytest.raises(ValueError, match="at least 2"):
        psgd.multi_vec_precond_update([q], [v1], [v1], [v1], 0.01)
    with pytest.raises(ValueError, match=r"dGs\[0\] has 6 elements"):
        psgd.multi_vec_precond_update([q], [v5], [v5], [v6], 0.01)
    with pytest.raises(ValueError, match=r"qls\[0\] has 5 elements"):
        psgd.multi_vec_precond_grad([v5], [v5], [v5], [v5])
    with pytest.raises(ValueError, match="qls has 2 tensors"):
        psgd.multi_vec_precond_grad([q, q], [v5], [v5], [v5])
    assert torch.equal(v5, torch.ones(5, device=_dev())) and float(q) == 1.0


# --------------------------------------------------------------------------------------------------------- non-finite contract
def _oracle_pair(ql, qr, dx, dg):
    with np.errstate(all="ignore"):
        return mv.oracle_update(ql, qr, dx, dg, mv.STEP)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["dG", "dX", "qr"])
def test_a_non_finite_value_stays_in_its_vector(psgd, where, value):
    """one NaN or +Inf in dG, dX or qr of the middle vector of three: its NaN mask is the oracle's, the other two vectors keep the
    bits of the clean run"""
    cases = [mv.case(n, "random", seed=9) for n in (65, 257, 1025)]
    clean = _run(psgd, cases)
    ql, qr, dx, dg, g = (np.array(a) for a in cases[1])
    {"dG": dg, "dX": dx, "qr": qr}[where][100] = value
    dirty = [cases[0], (ql, qr, dx, dg, g), cases[2]]
    got = _run(psgd, dirty)
    for i in (0, 2):
        _assert_same_bits({i: got[i]}, {i: clean[i]}, "a clean neighbour of a vector with %r in %s" % (value, where))
    ref_ql, ref_qr = _oracle_pair(ql, qr, dx, dg)
    got_ql, got_qr = got[1][0].view(np.float32).reshape(-1), got[1][1].view(np.float32).reshape(-1)
    assert bool(np.isnan(got_ql[0])) == bool(np.isnan(ref_ql)), (where, value, got_ql, ref_ql)
    assert np.array_equal(np.isnan(got_qr), np.isnan(ref_qr)), (where, value, int(np.isnan(got_qr).sum()), int(np.isnan(ref_qr).sum()))
    assert np.isnan(got_ql[0]) or np.isnan(got_qr).any()                           # it did not pass unseen
    with np.errstate(all="ignore"):
        ref_out = mv.oracle_apply(ql, qr, g)
    got_out = got[1][2].view(np.float32).reshape(-1)
    assert np.array_equal(np.isnan(got_out), np.isnan(ref_out)) and np.array_equal(np.isinf(got_out), np.isinf(ref_out))


def test_zero_pairs_give_what_the_oracle_gives(psgd):
    """dX = 0 and dG = 0: both gradients are 0, the steps are step / tiny times 0, and what is left is the balance"""
    cases = []
    for n in (3, 257):
        ql, qr, dx, dg, g = mv.case(n, "random", seed=4)
        cases.append((ql, qr, np.zeros_like(dx), np.zeros_like(dg), g))
    got = _run(psgd, cases)
    for i, (ql, qr, dx, dg, g) in enumerate(cases):
        ref_ql, ref_qr = _oracle_pair(ql, qr, dx, dg)
        got_ql, got_qr = got[i][0].view(np.float32).reshape(-1), got[i][1].view(np.float32).reshape(-1)
        assert np.isfinite(got_ql).all() and np.isfinite(got_qr).all()
        assert mv.rel(got_ql[0], ref_ql) < 1e-6 and mv.rel(got_qr, ref_qr) < 1e-6
        assert abs(got_ql[0] - got_qr.max()) <= 4 * np.spacing(np.float32(got_ql[0]))       # balanced: ql = max(qr)
