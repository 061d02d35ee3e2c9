"""QUAD with one diagonal side (include/psgd_kron_quad_diag_hip.h, psgd_kron_qdiag.hip) against a float64 restatement of the
header in plain torch.  Bars: README, "Parity" -- state 1e-5, increment 2e-3, apply 1e-5, L 1e-5, relative and norm-wise over the
matrix, over each 64 x 64 tile of the dense factor and over the diagonal vector.  tests/test_kron_qdiag_cpu.py evaluates the
restatement in float32 on every case: the inputs, not the kernels, are what it judges."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import kron_quad_diag as qd
from tests import kron_quad_cases as qc
from tests.guard_bands import DEFAULT_GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (D, n): the diagonal side's length and the dense side's.  (1000, 5), (1064, 64) and (1024, 5) split the Gram along K, the last
# slice short in the first two (both D are 8 mod 16, so it also ends in a partial K step) and whole in the third; (300, 130) folds
# the sum-of-squares partials over three tile columns, one partial; (1064, .) has five maxima for the diagonal Lipschitz fold and
# (262145, 1) has 1025 of them, one past a trip of its loop.  An odd case number starts L above ell, an even one below.
CASES = [(5, 1), (1, 5), (67, 3), (1000, 5), (1064, 64), (300, 130), (515, 33), (5, 130), (1024, 5), (262145, 1)]
SPLIT = {(1000, 5): 4, (1064, 64): 5, (1024, 5): 4}
_cache = {}


def shape_of(D, n, side):
    return (n, D) if side else (D, n)


def ref_apply(side, q, Q, G):
    return (q * q)[:, None] * ((G @ Q) @ Q) if side == 0 else (Q @ (Q @ G)) * (q * q)[None, :]


def ref_terms(side, q, Q, G):
    """(t, T): the sums of squares along the diagonal side and the Gram matrix of the dense side"""
    A = q[:, None] * (G @ Q) if side == 0 else (Q @ G) * q[None, :]
    return ((A * A).sum(1), A.T @ A) if side == 0 else ((A * A).sum(0), A @ A.T)


def ref_update(side, q, Q, L, G, step=qc.STEP, decay=qc.DECAY):
    """(new q, new Q, new L) from the old state, in the dtype of its inputs; q is the vector, L = [Ll, Lr]"""
    t, T_ = ref_terms(side, q, Q, G)
    D, n = float(q.numel()), float(Q.shape[0])
    ell = t.max() + n
    Ld = torch.maximum(decay * L[side] + (1 - decay) * ell, ell)
    gain = 1 - step / (2 * Ld) * (t - n)
    ell = qc.quad_bound(T_) + D
    LQ = torch.maximum(decay * L[1 - side] + (1 - decay) * ell, ell)
    c = step / (2 * LQ)
    P1 = Q - c * (T_ @ Q - D * Q)
    P2 = P1 - c * (P1 @ T_ - D * P1)
    return q * gain * gain, (P2 + P2.T) / 2, torch.stack([Ld, LQ] if side == 0 else [LQ, Ld])


def problem(D, n, side):
    """float32 q [1, D], Q, L, G and float64 out, new_q, new_Q, new_L, out_new; made once, never modified"""
    if (D, n, side) not in _cache:
        k = CASES.index((D, n))
        gen = torch.Generator().manual_seed(8100 + 2 * k + side)
        M, N = shape_of(D, n, side)
        G = torch.randn(M, N, generator=gen)
        G[0, :] *= 1.5
        G[:, 0] *= 1.5
        q, Q = 1 + 0.2 * torch.randn(D, generator=gen), qc._spd(n, gen)
        t, T_ = ref_terms(side, q.double(), Q.double(), G.double())
        top = torch.sort((T_ * T_).sum(0), descending=True).values[:2]      # problem()'s rule: no near-tie in the choice of j
        assert len(top) < 2 or float(top[0] - top[1]) >= 0.01 * float(top[0]), (D, n, side)
        ell = torch.stack([t.max() + n, qc.quad_bound(T_) + D] if side == 0 else [qc.quad_bound(T_) + D, t.max() + n])
        p = dict(q=q[None, :], Q=Q, G=G, L=((2.0 if k % 2 else 0.5) * ell).float())
        d = {key: x.double() for key, x in p.items()}
        p["out"] = ref_apply(side, d["q"][0], d["Q"], d["G"])
        new_q, p["new_Q"], p["new_L"] = ref_update(side, d["q"][0], d["Q"], d["L"], d["G"])
        p["new_q"] = new_q[None, :]
        p["out_new"] = ref_apply(side, new_q, p["new_Q"], d["G"])
        _cache[(D, n, side)] = p
    return _cache[(D, n, side)]


def errors(p, out, q, Q, L, out_new):
    """{bar name: the largest error of its kind} of a result in any dtype against the float64 fields of p"""
    inc = lambda f, new, old, key: f(new.double().cpu() - p[old].double(), p[key] - p[old].double())
    return dict(apply=max(qc.err(out, p["out"]), qc.err(out_new, p["out_new"])),
                state=max(qc.tile_err(Q, p["new_Q"]), qc.err(q, p["new_q"])),
                increment=max(inc(qc.tile_err, Q, "Q", "new_Q"), inc(qc.err, q, "q", "new_q")),
                L=float(((L.double().cpu() - p["new_L"]).abs() / p["new_L"]).max()))


def assert_bars(e, what):
    print(what, " ".join("%s %.2e" % kv for kv in sorted(e.items())))
    assert e["apply"] < qc.APPLY_BAR and e["state"] < qc.STATE_BAR and e["increment"] < qc.INCREMENT_BAR and e["L"] < qc.L_BAR, e


def factors(side, q, Q):
    return (q, Q) if side == 0 else (Q, q)


def run(side, p, G=None):
    """apply -> update -> apply on the device from p's state: (out, q, Q, L, out_new)"""
    q, Q, L = (p[k].to(DEV).clone() for k in ("q", "Q", "L"))
    G = (p["G"] if G is None else G).to(DEV)
    out = qd.apply(side, *factors(side, q, Q), G)
    qd.update(side, *factors(side, q, Q), L, G, qc.STEP, qc.DECAY)
    return out, q, Q, L, qd.apply(side, *factors(side, q, Q), G)


@pytest.mark.parametrize("side", [0, 1], ids=["left-diagonal", "right-diagonal"])
@pytest.mark.parametrize("D, n", CASES)
def test_apply_update_apply(D, n, side):
    p = problem(D, n, side)
    if (D, n) in SPLIT:
        assert qd.slices(*shape_of(D, n, side), side) == SPLIT[(D, n)] >= 2
    first, again = run(side, p), run(side, p)
    assert_bars(errors(p, *first), (D, n, side))
    assert torch.equal(first[2], first[2].T)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("side", [0, 1], ids=["left-diagonal", "right-diagonal"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_non_finite_gradient_has_the_restatements_nan_mask(value, where, side):
    p = problem(67, 3, side)
    G = p["G"].clone()
    G.view(-1)[dict(first=0, middle=G.numel() // 2, last=G.numel() - 1)[where]] = value
    d = {k: p[k].double() for k in ("q", "Q", "L")}
    new_q, new_Q, new_L = ref_update(side, d["q"][0], d["Q"], d["L"], G.double())
    ref = (ref_apply(side, d["q"][0], d["Q"], G.double()), new_q[None, :], new_Q, new_L, ref_apply(side, new_q, new_Q, G.double()))
    assert any(bool(torch.isnan(r).any()) for r in ref)
    for got, want, name in zip(run(side, p, G), ref, ("out", "q", "Q", "L", "out_new")):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want)), name


@pytest.mark.parametrize("side", [0, 1], ids=["left-diagonal", "right-diagonal"])
def test_zero_gradient_grows_both_factors(side):
    D, n = 300, 130
    M, N = shape_of(D, n, side)
    p = dict(problem(D, n, side), G=torch.zeros(M, N), L=torch.zeros(2))
    d = {k: p[k].double() for k in ("q", "Q", "L", "G")}
    new_q, new_Q, new_L = ref_update(side, d["q"][0], d["Q"], d["L"], d["G"])
    out, q, Q, L, out_new = run(side, p)
    assert L.tolist() == new_L.tolist() == [float(N), float(M)]               # [t2l, t2r], exactly
    assert not out.any() and not out_new.any()
    assert qc.err(q, new_q[None, :]) < qc.STATE_BAR and qc.tile_err(Q, new_Q) < qc.STATE_BAR
    assert float((q.cpu() / p["q"]).min()) > 1 and float((Q.diagonal().cpu() / p["Q"].diagonal()).min()) > 1


@pytest.mark.parametrize("side", [0, 1], ids=["left-diagonal", "right-diagonal"])
@pytest.mark.parametrize("entry", ["apply", "update"])
def test_entry_point_stays_inside_its_extents(entry, side):
    """both compute entry points between guard bands, bases aligned to 16 bytes and no better, on a NaN-filled workspace of
    exactly the bytes asked for: the bands stay whole and the bits are those of the plain call"""
    D, n = 515, 33
    M, N = shape_of(D, n, side)
    p, lib = problem(D, n, side), qd.load()
    ws_bytes = lib.psgd_kron_qdiag_workspace_bytes(M, N, side)
    shapes = dict(q=(1, D), Q=(n, n), L=(2,), G=(M, N), out=(M, N))
    arena = Arena(4 * (D + n * n + 2 * M * N + 2) + ws_bytes + 7 * (2 * DEFAULT_GUARD + 4096), 0xFF, DEV)
    t = {k: arena.take(s, torch.float32, align=16, name=k) for k, s in shapes.items()}
    ws = arena.take_bytes(ws_bytes)
    writes = ("out",) if entry == "apply" else ("q", "Q", "L")
    for k in t:
        if k != "out":
            t[k].copy_(p[k])
        if k not in writes:
            arena.freeze(k)
    Ql, Qr = (x.data_ptr() for x in factors(side, t["q"], t["Q"]))
    stream = torch.cuda.current_stream(DEV).cuda_stream
    plain = run(side, p)
    if entry == "apply":
        rc = lib.psgd_kron_qdiag_apply_f32(Ql, Qr, t["G"].data_ptr(), t["out"].data_ptr(), M, N, side, ws.data_ptr(), ws_bytes, stream)
        want = dict(out=plain[0])
    else:
        rc = lib.psgd_kron_qdiag_update_f32(Ql, Qr, t["L"].data_ptr(), t["G"].data_ptr(), M, N, side, qc.STEP, qc.DECAY, ws.data_ptr(),
                                            ws_bytes, stream)
        want = dict(q=plain[1], Q=plain[2], L=plain[3])
    assert rc == 0
    arena.check()
    for k, x in want.items():
        assert bool(torch.isfinite(x).all()) and torch.equal(t[k], x), k


SHAPES, FORMATS = [(70, 6), (6, 70), (5, 7)], [("scale", "dense"), ("dense", "scale"), "dense"]


def _model():
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(DEV) for s in SHAPES]
    return params, lambda: sum(((x - t) ** 2).sum() for x, t in zip(params, targets))     # separable: no layer sees another


def _opt(params):
    return psgd.Kron(params, FORMATS, 1.0, 0.01, 0.1, preconditioner_fit="whitening", probe_seed=3, preconditioner_update="quad",
                     generator=torch.Generator().manual_seed(1), quad_diagonal=True)


def test_class_runs_the_functional_calls_and_resumes_bit_for_bit():
    params, closure = _model()
    opt = _opt(params)
    assert opt.quad_layers == [0, 1, 2]
    hand, hand_closure = _model()
    fmts = [("scale", "dense"), ("dense", "scale"), ("dense", "dense")]
    state = [psgd.kron_quad_initial_state(*s, device=DEV, formats=f) for s, f in zip(SHAPES, fmts)]
    lr = float(torch.tensor(0.01, dtype=torch.float32))
    for step in range(4):
        if step == 3:                                   # the fourth step twice: uninterrupted, and from the saved state
            sd, saved = opt.state_dict(), [x.detach().clone() for x in params]
            assert sd["quad_diagonal"] is True and len(sd["quad_L"]) == 3
        opt.step(closure)
        grads = torch.autograd.grad(hand_closure(), hand)
        with torch.no_grad():
            for (Ql, Qr, L), g, x in zip(state, grads, hand):
                psgd.update_precond_kron_quad_(Ql, Qr, L, g, 0.1)
                x.sub_(lr * psgd.precond_grad_kron_quad(Ql, Qr, g))
    for i, (Ql, Qr, L) in enumerate(state):
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [opt.quad_L[i], params[i]], [Ql, Qr, L, hand[i]])), i
    again_params, again_closure = _model()
    with torch.no_grad():
        for x, s in zip(again_params, saved):
            x.copy_(s)
    again = _opt(again_params)
    again.load_state_dict(sd)
    again.step(again_closure)
    for i in range(3):
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [opt.quad_L[i], params[i]],
                                                     again.factors[i] + [again.quad_L[i], again_params[i]])), i
