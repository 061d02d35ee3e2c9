"""psgd_kron_quad.hip against the float64 restatement of tests/kron_quad_cases.py."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib
from tests import kron_quad_cases as qc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _state(p):
    return [p[k].to(DEV).clone() for k in ("Ql", "Qr", "L")]


def _increment_err(new, old, ref_new, err=qc.err):
    return err(new.double().cpu() - old.double(), ref_new - old.double())


def _apply_update_apply(p, M, N):
    """every error norm-wise over the matrix and over each T x T tile, against the same bar"""
    G = p["G"].to(DEV)
    Ql, Qr, L = _state(p)
    out = psgd.precond_grad_kron_quad(Ql, Qr, G)
    e, et = qc.err(out, p["out"]), qc.tile_err(out, p["out"])
    print("out", M, N, "apply %.2e tile-wise %.2e" % (e, et))
    assert e < qc.APPLY_BAR and et < qc.APPLY_BAR
    assert psgd.update_precond_kron_quad_(Ql, Qr, L, G, qc.STEP, qc.DECAY) is None
    for k, new in (("Ql", Ql), ("Qr", Qr)):
        e, ei = qc.err(new, p["new_" + k]), _increment_err(new, p[k], p["new_" + k])
        et, eit = qc.tile_err(new, p["new_" + k]), _increment_err(new, p[k], p["new_" + k], qc.tile_err)
        print(k, M, N, "state %.2e increment %.2e tile-wise %.2e %.2e" % (e, ei, et, eit))
        assert e < qc.STATE_BAR and ei < qc.INCREMENT_BAR
        assert et < qc.STATE_BAR and eit < qc.INCREMENT_BAR
        assert torch.equal(new, new.T)
    e = qc.err(L, p["new_L"])
    print("L", M, N, "%.2e" % e)
    assert e < qc.L_BAR
    out = psgd.precond_grad_kron_quad(Ql, Qr, G)
    e, et = qc.err(out, p["out_new"]), qc.tile_err(out, p["out_new"])
    print("out_new", M, N, "apply %.2e tile-wise %.2e" % (e, et))
    assert e < qc.APPLY_BAR and et < qc.APPLY_BAR
    again = _state(p)                                   # the same call from the same start: the same bits
    psgd.update_precond_kron_quad_(*again, G, qc.STEP, qc.DECAY)
    assert all(torch.equal(a, b) for a, b in zip(again, (Ql, Qr, L)))


@pytest.mark.parametrize("M, N, seed", qc.CASES)
def test_apply_update_apply(M, N, seed):
    _apply_update_apply(qc.problem(M, N, seed), M, N)


def test_lipschitz_kernel_past_its_1024_threads():
    """N > kLipT with the right side's j in the second trip of the strided loops (tests/test_kron_quad_cpu.py asserts j >= 1024)"""
    M, N, seed, col = qc.LIP_CASE
    _apply_update_apply(qc.problem(M, N, seed, col), M, N)


@pytest.mark.parametrize("M, N, seed", [qc.CASES[3], qc.CASES[6]])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_nan_masks_are_the_restatements(M, N, seed, where):
    p = qc.problem(M, N, seed)
    G = p["G"].clone()
    G.view(-1)[{"first": 0, "middle": G.numel() // 2, "last": G.numel() - 1}[where]] = float("nan")
    d = {k: p[k].double() for k in ("Ql", "Qr", "L")}
    ref = (qc.quad_apply_ref(d["Ql"], d["Qr"], G.double()),) + qc.quad_update_ref(d["Ql"], d["Qr"], d["L"], G.double())
    Ql, Qr, L = _state(p)
    out = psgd.precond_grad_kron_quad(Ql, Qr, G.to(DEV))
    psgd.update_precond_kron_quad_(Ql, Qr, L, G.to(DEV), qc.STEP)
    for got, want in zip((out, Ql, Qr, L), ref):
        assert torch.equal(torch.isnan(got).cpu(), torch.isnan(want))


@pytest.mark.parametrize("M, N, seed", [qc.CASES[3], qc.CASES[6]])
@pytest.mark.parametrize("where", ["first", "middle", "last", "edge"])
@pytest.mark.parametrize("value", ["inf", "-inf"])
def test_inf_anywhere_in_g_makes_the_whole_state_nan(M, N, seed, where, value):
    """the Inf half of the header's sentence, asserted itself and not as the restatement's mask (the NaN half is the test above);
    edge: the last element of the partial tile at the top right"""
    p = qc.problem(M, N, seed)
    G = p["G"].clone()
    at = {"first": 0, "middle": G.numel() // 2, "last": G.numel() - 1, "edge": (min(M, qc.T) - 1) * N + N - 1}[where]
    G.view(-1)[at] = float(value)
    Ql, Qr, L = _state(p)
    psgd.update_precond_kron_quad_(Ql, Qr, L, G.to(DEV), qc.STEP)
    assert bool(torch.isnan(Ql).all()) and bool(torch.isnan(Qr).all()) and bool(torch.isnan(L).all())


def test_zero_gradient_grows_the_factors():
    M, N, seed = qc.CASES[4]
    p = qc.problem(M, N, seed)
    Ql, Qr, _ = _state(p)
    L, G = torch.zeros(2, device=DEV), torch.zeros(M, N)
    ref = qc.quad_update_ref(p["Ql"].double(), p["Qr"].double(), L.double().cpu(), G.double())
    psgd.update_precond_kron_quad_(Ql, Qr, L, G.to(DEV), qc.STEP)
    assert L.tolist() == [float(N), float(M)]
    assert qc.err(Ql, ref[0]) < qc.STATE_BAR and qc.err(Qr, ref[1]) < qc.STATE_BAR


def test_out_aliasing_an_input_is_refused():
    p = qc.problem(*qc.CASES[5])
    Ql, Qr, _ = _state(p)
    G = p["G"].to(DEV)
    with pytest.raises(_lib.PsgdHipError, match="psgd_kron_quad_apply_f32"):
        psgd.precond_grad_kron_quad(Ql, Qr, G, out=G)
    assert torch.equal(G.cpu(), p["G"])


def test_trajectory_300_steps():
    M, N, steps = 12, 20, 300
    gen = torch.Generator().manual_seed(123)

    def cov(n):
        X = torch.randn(n, n, generator=gen, dtype=torch.float64)
        C = X @ X.T / n + 0.1 * torch.eye(n, dtype=torch.float64)
        e, v = torch.linalg.eigh(C)
        return C, (v * e.sqrt()) @ v.T
    (Cl, Hl), (Cr, Hr) = cov(M), cov(N)
    Gs = (Hl @ torch.randn(steps, M, N, generator=gen, dtype=torch.float64) @ Hr).float()

    def residual(Ql, Qr):                               # E[Ql G Qr Qr G' Ql] / N - I in closed form
        return float((Ql @ Cl @ Ql * torch.trace(Cr @ Qr @ Qr) / N - torch.eye(M, dtype=torch.float64)).norm())
    r64 = [t.double() for t in psgd.kron_quad_initial_state(M, N)]
    r32 = list(psgd.kron_quad_initial_state(M, N))
    hip = list(psgd.kron_quad_initial_state(M, N, device=DEV))
    start = residual(r64[0], r64[1])
    Gd = Gs.to(DEV)
    for t in range(steps):
        r64 = qc.quad_update_ref(*r64, Gs[t].double())
        r32 = qc.quad_update_ref(*r32, Gs[t])
        psgd.update_precond_kron_quad_(*hip, Gd[t], qc.STEP)
    assert residual(r64[0], r64[1]) < start             # the definition whitens, on the reference alone
    for got, f32, ref in zip(hip, r32, r64):
        e, e32 = qc.err(got, ref), qc.err(f32, ref)
        print("drift hip %.2e fp32 %.2e" % (e, e32))
        assert e < 1e-5 and e <= 3 * max(e32, 1e-7)
