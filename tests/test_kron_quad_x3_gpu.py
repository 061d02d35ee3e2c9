"""psgd_kron_quad_x3.hip (products="bf16x3") against the float64 restatement of tests/kron_quad_cases.py and against the fp32
route on the same inputs.

The relative bar, err_x3 <= max(8 err_fp32, 2^-21): the terms m l' + l m' + l l' that the truncating split drops are at most
2^-21 relative, against one fp32 rounding of 2^-24; a route that loses any of the six kept terms is off by 2^-15 or more."""
import numpy as np
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import kron_quad_x3
from tests import kron_quad_cases as qc
from tests.guard_bands import DEFAULT_GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
X3 = dict(products="bf16x3")
# macro-tile (128) edges the 64-tile cases do not reach; K = 127, 128, 129, 260 are 31, 0, 1, 4 (mod 32)
EDGE_CASES = [(127, 129, 30), (128, 128, 30), (129, 260, 30), (256, 384, 30), (5, 131, 31)]
FLOOR = 2.0 ** -21


def _state(p):
    return [p[k].to(DEV).clone() for k in ("Ql", "Qr", "L")]


def _run(p, **kw):
    """apply -> update -> apply; {name: tensor}"""
    G = p["G"].to(DEV)
    Ql, Qr, L = _state(p)
    out = psgd.precond_grad_kron_quad(Ql, Qr, G, **kw)
    assert psgd.update_precond_kron_quad_(Ql, Qr, L, G, qc.STEP, qc.DECAY, **kw) is None
    return dict(out=out, new_Ql=Ql, new_Qr=Qr, new_L=L, out_new=psgd.precond_grad_kron_quad(Ql, Qr, G, **kw))


@pytest.mark.parametrize("M, N, seed", qc.CASES + EDGE_CASES)
def test_apply_update_apply(M, N, seed):
    p = qc.problem(M, N, seed)
    x3, f32 = _run(p, **X3), _run(p)
    bars = dict(out=qc.APPLY_BAR, out_new=qc.APPLY_BAR, new_Ql=qc.STATE_BAR, new_Qr=qc.STATE_BAR)
    for k, bar in bars.items():
        e, et, e32 = qc.err(x3[k], p[k]), qc.tile_err(x3[k], p[k]), qc.err(f32[k], p[k])
        print("x3 parity", M, N, k, "err %.3e tile-wise %.3e fp32 route %.3e ratio %.2f" % (e, et, e32, e / e32 if e32 else 0.0))
        assert e < bar and et < bar and e <= max(8 * e32, FLOOR)
    for k in ("Ql", "Qr"):
        inc = lambda err: err(x3["new_" + k].double().cpu() - p[k].double(), p["new_" + k] - p[k].double())
        assert inc(qc.err) < qc.INCREMENT_BAR and inc(qc.tile_err) < qc.INCREMENT_BAR
        assert torch.equal(x3["new_" + k], x3["new_" + k].T)
    assert qc.err(x3["new_L"], p["new_L"]) < qc.L_BAR
    again = _run(p, **X3)                                                    # equal inputs: equal bits
    assert all(torch.equal(again[k], x3[k]) for k in x3)


@pytest.mark.parametrize("M, N, seed", qc.EXACT_CASES)
def test_exact_cases_bit_for_bit(M, N, seed):
    """every product operand of these cases has at most 8 significant bits: one bf16 term, exact partial sums in any order"""
    p = qc.exact_problem(M, N, seed)
    G = p["G"].to(DEV)
    Ql, Qr, L = _state(p)
    assert torch.equal(psgd.precond_grad_kron_quad(Ql, Qr, G, **X3).double().cpu(), p["out"])
    psgd.update_precond_kron_quad_(Ql, Qr, L, G, p["step"], p["decay"], **X3)
    for got, key in ((Ql, "new_Ql"), (Qr, "new_Qr"), (L, "new_L")):
        assert torch.equal(got.double().cpu(), p[key]), key


@pytest.mark.parametrize("M, N, seed, shift", qc.SHIFT_CASES)
def test_shift_cases_carry_all_three_planes(M, N, seed, shift):
    """one non-zero term per sum and a dense fp32 G: h, m and l of G (a B-side operand) and of W, A (A-side) must all arrive"""
    p = qc.shift_problem(M, N, seed, shift)
    out = psgd.precond_grad_kron_quad(p["Ql"].to(DEV), p["Qr"].to(DEV), p["G"].to(DEV), **X3)
    assert torch.equal(out.double().cpu(), p["out"])


@pytest.mark.parametrize("M, N, seed", [EDGE_CASES[2], EDGE_CASES[4]])
@pytest.mark.parametrize("entry", ["apply", "update"])
def test_entry_point_stays_inside_its_extents(entry, M, N, seed):
    """guard bands, a base skewed by 4 bytes, a NaN-filled workspace of exactly the bytes asked for: the bits of the aligned call"""
    p = qc.problem(M, N, seed)
    lib = kron_quad_x3.load()
    ws_bytes = lib.psgd_kron_quad_x3_workspace_bytes(M, N)
    shapes = dict(Ql=(M, M), Qr=(N, N), L=(2,), G=(M, N), out=(M, N))
    writes = ("out",) if entry == "apply" else ("Ql", "Qr", "L")
    arena = Arena(4 * (M * M + N * N + 2 * M * N + 2) + ws_bytes + 7 * (2 * DEFAULT_GUARD + 4096), 0xFF, DEV)
    t = {k: arena.take(s, torch.float32, align=16, skew=1, name=k) for k, s in shapes.items()}
    ws = arena.take_bytes(ws_bytes)
    for k in t:
        if k != "out":
            t[k].copy_(p[k])
        if k not in writes:
            arena.freeze(k)
    ptr = {k: x.data_ptr() for k, x in t.items()}
    stream = torch.cuda.current_stream(DEV).cuda_stream
    plain = {k: p[k].to(DEV).clone() for k in ("Ql", "Qr", "L", "G")}
    if entry == "apply":
        rc = lib.psgd_kron_quad_x3_apply_f32(ptr["Ql"], ptr["Qr"], ptr["G"], ptr["out"], M, N, ws.data_ptr(), ws_bytes, stream)
        plain["out"] = psgd.precond_grad_kron_quad(plain["Ql"], plain["Qr"], plain["G"], **X3)
    else:
        rc = lib.psgd_kron_quad_x3_update_f32(ptr["Ql"], ptr["Qr"], ptr["L"], ptr["G"], M, N, qc.STEP, qc.DECAY, ws.data_ptr(),
                                              ws_bytes, stream)
        psgd.update_precond_kron_quad_(plain["Ql"], plain["Qr"], plain["L"], plain["G"], qc.STEP, qc.DECAY, **X3)
    assert rc == 0
    arena.check()
    for k in writes:
        assert bool(torch.isfinite(plain[k]).all()) and torch.equal(t[k], plain[k]), k


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("value", ["nan", "inf", "-inf"])
def test_non_finite_gradient(where, value):
    """update: the whole state NaN; apply: the restatement's non-finite mask (an Inf of the restatement may be a NaN here)"""
    M, N = 65, 131
    p = qc.problem(M, N, 30)
    G = p["G"].clone()
    G.view(-1)[{"first": 0, "middle": (M // 2) * N + N // 2, "last": G.numel() - 1}[where]] = float(value)
    ref = qc.quad_apply_ref(p["Ql"].double(), p["Qr"].double(), G.double())
    Ql, Qr, L = _state(p)
    out = psgd.precond_grad_kron_quad(Ql, Qr, G.to(DEV), **X3)
    assert torch.equal(~torch.isfinite(out).cpu(), ~torch.isfinite(ref)) and bool((~torch.isfinite(ref)).any())
    psgd.update_precond_kron_quad_(Ql, Qr, L, G.to(DEV), qc.STEP, **X3)
    assert bool(torch.isnan(Ql).all()) and bool(torch.isnan(Qr).all()) and bool(torch.isnan(L).all())


SHAPES, ROUTED = [(70, 96), (40, 50)], [0]                                   # short sides above and below the threshold of 64
LR, LR_Q = 0.01, 0.1


def _model():
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(DEV) for s in SHAPES]
    return params, lambda: sum(((q - t) ** 2).sum() for q, t in zip(params, targets))


def _opt(params):
    return psgd.Kron(params, "dense", 1.0, LR, LR_Q, preconditioner_fit="whitening", probe_seed=3,
                     generator=torch.Generator().manual_seed(1), preconditioner_update="quad", quad_products="bf16x3",
                     quad_products_min_dim=64)


def test_class_step_is_the_functional_calls_and_resumes_bit_for_bit():
    params, closure = _model()
    opt = _opt(params)
    assert opt.quad_layers == [0, 1] and opt.quad_x3_layers == ROUTED
    hand, hand_closure = _model()
    state = [psgd.kron_quad_initial_state(*s, device=DEV) for s in SHAPES]
    opt.step(closure)
    grads = torch.autograd.grad(hand_closure(), hand)
    with torch.no_grad():
        for i, (Ql, Qr, L) in enumerate(state):
            kw = X3 if i in ROUTED else {}
            psgd.update_precond_kron_quad_(Ql, Qr, L, grads[i], LR_Q, **kw)
            hand[i].sub_(float(np.float32(LR)) * psgd.precond_grad_kron_quad(Ql, Qr, grads[i], **kw))
    for i in range(len(SHAPES)):
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [opt.quad_L[i]], state[i]))
        assert torch.equal(params[i], hand[i])
    sd = opt.state_dict()
    assert sd["quad_products"] == "bf16x3"
    saved = [q.detach().clone() for q in params]
    opt.step(closure)
    again_params, again_closure = _model()
    with torch.no_grad():
        for q, s in zip(again_params, saved):
            q.copy_(s)
    again = _opt(again_params)
    again.load_state_dict(sd)
    again.step(again_closure)
    for i in range(len(SHAPES)):
        assert torch.equal(params[i], again_params[i])
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [opt.quad_L[i]], again.factors[i] + [again.quad_L[i]]))
