"""The three-factor QUAD update (include/psgd_kron_quad_nd_hip.h, psgd_kron_qnd.hip) against the float64 restatement of
tests/kron_quad_nd_cases.py.  Bars: README, "Parity" -- state 1e-5, increment 2e-3, apply 1e-5, L 1e-5, relative and norm-wise."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import kron_quad_nd as qn
from tests import kron_quad_cases as qc
from tests import kron_quad_nd_cases as nc
from tests.guard_bands import DEFAULT_GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def run(p, G=None):
    """apply -> update -> apply on the device from p's state: [out, Qa, Qb, Qc, L, out_new]"""
    Qs, L = [Q.to(DEV).clone() for Q in p["Qs"]], p["L"].to(DEV).clone()
    G = (p["G"] if G is None else G).to(DEV)
    out = psgd.precond_grad_kron_quad_nd(Qs, G)
    psgd.update_precond_kron_quad_nd_(Qs, L, G, qc.STEP, qc.DECAY)
    return [out, *Qs, L, psgd.precond_grad_kron_quad_nd(Qs, G)]


@pytest.mark.parametrize("case", nc.CASES, ids=lambda c: "-".join(map(str, c)))
def test_apply_update_apply(case):
    p = nc.problem(*case)
    first, again = run(p), run(p)
    out, *Qs, L, out_new = first
    inc = lambda new, old, ref: qc.err(new.double().cpu() - old.double(), ref - old.double())
    e = dict(apply=max(qc.err(out, p["out"]), qc.err(out_new, p["out_new"])),
             state=max(qc.err(Q, ref) for Q, ref in zip(Qs, p["new_Qs"])),
             increment=max(inc(Q, old, ref) for Q, old, ref in zip(Qs, p["Qs"], p["new_Qs"])),
             L=float(((L.double().cpu() - p["new_L"]).abs() / p["new_L"]).max()))
    print(case, " ".join("%s %.2e" % kv for kv in sorted(e.items())))
    assert e["apply"] < qc.APPLY_BAR and e["state"] < qc.STATE_BAR and e["increment"] < qc.INCREMENT_BAR and e["L"] < qc.L_BAR, e
    assert all(torch.equal(Q, Q.T) for Q in Qs)                              # one value written twice
    assert all(torch.equal(a, b) for a, b in zip(first, again))  # a second call: the same bits


@pytest.mark.parametrize("B, C, seed", nc.BIT_CASES)
def test_unit_first_mode_is_the_two_factor_update_bit_for_bit(B, C, seed):
    q = qc.problem(B, C, seed)
    Ql, Qr, L2, G = (q[k].to(DEV).clone() for k in ("Ql", "Qr", "L", "G"))
    Qs = [torch.ones(1, 1, device=DEV), Ql.clone(), Qr.clone()]
    L3 = torch.cat([torch.zeros(1, device=DEV), L2])
    out2 = psgd.precond_grad_kron_quad(Ql, Qr, G)
    out3 = psgd.precond_grad_kron_quad_nd(Qs, G[None])
    psgd.update_precond_kron_quad_(Ql, Qr, L2, G, qc.STEP, qc.DECAY)
    psgd.update_precond_kron_quad_nd_(Qs, L3, G[None], qc.STEP, qc.DECAY)
    assert torch.equal(Qs[1], Ql) and torch.equal(Qs[2], Qr) and torch.equal(L3[1:], L2) and torch.equal(out3[0], out2)


def test_zero_gradient_grows_every_factor():
    A, B, C, seed = nc.CASES[6]
    p = dict(nc.problem(A, B, C, seed), G=torch.zeros(A, B, C), L=torch.zeros(3))
    out, *Qs, L, out_new = run(p)
    t2 = [float(B * C), float(A * C), float(A * B)]
    assert L.tolist() == t2 and not out.any() and not out_new.any()          # ell = t2 exactly
    for Q, old, t in zip(Qs, p["Qs"], t2):                                   # c = step / (2 t2): (1 + c t2)^2 = (1 + step / 2)^2
        assert qc.err(Q, old.double() * (1 + qc.STEP / 2) ** 2) < qc.STATE_BAR


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_nan_gradient_has_the_restatements_nan_mask(where):
    p = nc.problem(*nc.CASES[2])
    G = p["G"].clone()
    G.view(-1)[dict(first=0, middle=G.numel() // 2, last=G.numel() - 1)[where]] = float("nan")
    dQ = [Q.double() for Q in p["Qs"]]
    new_Qs, new_L = nc.nd_update_ref(dQ, p["L"].double(), G.double())
    ref = [nc.nd_apply_ref(dQ, G.double()), *new_Qs, new_L, nc.nd_apply_ref(new_Qs, G.double())]
    assert all(bool(torch.isnan(r).all()) for r in ref[1:5])
    for got, want in zip(run(p, G), ref):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want))


@pytest.mark.parametrize("entry", ["apply", "update"])
def test_entry_point_stays_inside_its_extents(entry):
    """between guard bands, every base 4 bytes off a 16-byte boundary, on a NaN-filled workspace of exactly the bytes asked for"""
    A, B, C, seed = nc.CASES[3]                                              # the shape whose aligned call takes 16-byte loads
    p, lib = nc.problem(A, B, C, seed), qn.load()
    ws_bytes = lib.psgd_kron_qnd_workspace_bytes(A, B, C)
    shapes = dict(Qa=(A, A), Qb=(B, B), Qc=(C, C), L=(3,), G=(A, B, C), out=(A, B, C))
    arena = Arena(4 * (A * A + B * B + C * C + 2 * A * B * C + 3) + ws_bytes + 8 * (2 * DEFAULT_GUARD + 4096), 0xFF, DEV)
    t = {k: arena.take(s, torch.float32, align=16, skew=1, name=k) for k, s in shapes.items()}
    ws = arena.take_bytes(ws_bytes)
    writes = ("out",) if entry == "apply" else ("Qa", "Qb", "Qc", "L")
    for k, src in dict(Qa=p["Qs"][0], Qb=p["Qs"][1], Qc=p["Qs"][2], L=p["L"], G=p["G"]).items():
        t[k].copy_(src)
    for k in set(t) - set(writes):
        arena.freeze(k)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    out, *Qs, L, _ = run(p)
    ptr = lambda *names: [t[k].data_ptr() for k in names]
    if entry == "apply":
        rc = lib.psgd_kron_qnd_apply_f32(*ptr("Qa", "Qb", "Qc", "G", "out"), A, B, C, ws.data_ptr(), ws_bytes, stream)
        want = dict(out=out)
    else:
        rc = lib.psgd_kron_qnd_update_f32(*ptr("Qa", "Qb", "Qc", "L", "G"), A, B, C, qc.STEP, qc.DECAY, ws.data_ptr(), ws_bytes, stream)
        want = dict(Qa=Qs[0], Qb=Qs[1], Qc=Qs[2], L=L)
    assert rc == 0
    arena.check()
    for k, x in want.items():
        assert bool(torch.isfinite(x).all()) and torch.equal(t[k], x), k


def _model(SHAPES=((6, 5, 3, 3), (5, 7), (7,))):
    gen = torch.Generator().manual_seed(5)
    params = [torch.randn(s, generator=gen).to(DEV).requires_grad_() for s in SHAPES]
    targets = [torch.randn(s, generator=gen).to(DEV) for s in SHAPES]
    return params, lambda: sum(((x - t) ** 2).sum() for x, t in zip(params, targets))     # separable: no layer sees another


def _opt(params, quad_tensor=True):
    return psgd.Kron(params, "dense", 1.0, 0.01, 0.1, preconditioner_fit="whitening", probe_seed=3, preconditioner_update="quad",
                     generator=torch.Generator().manual_seed(1), any_rank=True, quad_tensor=quad_tensor)


def test_class_runs_the_functional_calls_and_resumes_bit_for_bit():
    params, closure = _model()
    opt = _opt(params)
    assert opt.quad_layers == [0, 1] and opt.quad_tensor_layers == [0] and tuple(opt.quad_L[0].shape) == (3,)
    folded_params, folded_closure = _model()
    folded = _opt(folded_params, quad_tensor=False)                          # the conv layer is the folded matrix layer of today
    assert folded.quad_layers == [0, 1] and folded.quad_tensor_layers == [] and "quad_tensor" not in folded.state_dict()
    assert [tuple(Q.shape) for Q in folded.factors[0]] == [(6, 6), (45, 45)]
    hand, hand_closure = _model()
    conv, conv_L = psgd.kron_quad_nd_initial_state((6, 5, 9), device=DEV)
    Ql, Qr, mat_L = psgd.kron_quad_initial_state(5, 7, device=DEV)
    lr = float(torch.tensor(0.01, dtype=torch.float32))
    for step in range(3):
        if step == 1:                                   # saved after step 1: steps 2 and 3 run twice
            sd, saved = opt.state_dict(), [x.detach().clone() for x in params]
            assert sd["quad_tensor"] is True and [tuple(L.shape) for L in sd["quad_L"]] == [(3,), (2,)] and len(sd["factors"][0]) == 3
        opt.step(closure)
        folded.step(folded_closure)
        grads = torch.autograd.grad(hand_closure(), hand)
        with torch.no_grad():
            g = grads[0].view(6, 5, 9)
            psgd.update_precond_kron_quad_nd_(conv, conv_L, g, 0.1)
            hand[0].sub_(lr * psgd.precond_grad_kron_quad_nd(conv, g).view(6, 5, 3, 3))
            psgd.update_precond_kron_quad_(Ql, Qr, mat_L, grads[1], 0.1)
            hand[1].sub_(lr * psgd.precond_grad_kron_quad(Ql, Qr, grads[1]))
    want = [conv + [conv_L, hand[0]], [Ql, Qr, mat_L, hand[1]], folded.factors[2] + [folded_params[2]]]
    have = [opt.factors[i] + [opt.quad_L[i], params[i]] for i in (0, 1)] + [opt.factors[2] + [params[2]]]
    assert all(torch.equal(a, b) for x, y in zip(have, want) for a, b in zip(x, y))
    again_params, again_closure = _model()
    with torch.no_grad():
        for x, s in zip(again_params, saved):
            x.copy_(s)
    again = _opt(again_params)
    again.load_state_dict(sd)
    with pytest.raises(ValueError, match="quad_tensor"):
        folded.load_state_dict(sd)
    for _ in range(2):
        again.step(again_closure)
    for i in range(3):
        assert all(torch.equal(a, b) for a, b in zip(opt.factors[i] + [params[i]], again.factors[i] + [again_params[i]])), i
    assert all(torch.equal(opt.quad_L[i], again.quad_L[i]) for i in (0, 1))
