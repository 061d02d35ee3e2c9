"""include/psgd_kron_quad_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, class refusals."""
import ctypes
import os
import re

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, kron_quad
from tests import kron_quad_cases as qc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_kron_quad_hip.h")


def test_header_symbols_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psgd_kron_quad_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(kron_quad.SIGNATURES) and len(declared) == 3
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), kron_quad.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == kron_quad.SIGNATURES[n][1] for n in declared)
    assert not set(declared) & set(_lib.SIGNATURES)
    assert int(re.search(r"#define\s+PSGD_KRON_QUAD_TILE\s+(\d+)", text).group(1)) == kron_quad.KRON_QUAD_TILE == qc.T


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS = kron_quad.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    Ql, Qr, L, G, out, ws = (0x10000 * k for k in range(1, 7))          # never dereferenced: the checks fail first
    need = lib.psgd_kron_quad_workspace_bytes(70, 5)
    assert need > 4 * (2 * 70 * 5 + 2 * 70 * 70 + 2 * 5 * 5)
    assert lib.psgd_kron_quad_workspace_bytes(0, 5) == BAD and lib.psgd_kron_quad_workspace_bytes(5, -1) == BAD
    for args in ((None, Qr, G, out, 70, 5), (Ql, None, G, out, 70, 5), (Ql, Qr, None, out, 70, 5), (Ql, Qr, G, None, 70, 5),
                 (Ql, Qr, G, out, 0, 5), (Ql, Qr, G, out, 70, 0), (Ql, Qr, G, G, 70, 5), (Ql, Qr, G, Ql, 70, 5), (Ql, Qr, G, Qr, 70, 5)):
        assert lib.psgd_kron_quad_apply_f32(*args, ws, need, None) == BAD
    for args in ((None, Qr, L, G, 70, 5), (Ql, None, L, G, 70, 5), (Ql, Qr, None, G, 70, 5), (Ql, Qr, L, None, 70, 5),
                 (Ql, Qr, L, G, 70, -1), (Ql, Ql, L, G, 70, 5), (Ql, Qr, L, Ql, 70, 5), (Ql, Qr, Qr, G, 70, 5)):
        assert lib.psgd_kron_quad_update_f32(*args, 0.1, 0.95, ws, need, None) == BAD
    for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
        assert lib.psgd_kron_quad_apply_f32(Ql, Qr, G, out, 70, 5, *bad_ws, None) == WS
        assert lib.psgd_kron_quad_update_f32(Ql, Qr, L, G, 70, 5, 0.1, 0.95, *bad_ws, None) == WS


def test_functions_refuse_bad_operands_by_name():
    Ql, Qr, L = psgd.kron_quad_initial_state(3, 5)
    G = torch.zeros(3, 5)
    with pytest.raises(ValueError, match="Qr"):
        psgd.precond_grad_kron_quad(Ql, Ql, G)
    with pytest.raises(TypeError, match="Ql"):
        psgd.precond_grad_kron_quad(Ql.double(), Qr, G)
    with pytest.raises(ValueError, match="L "):
        psgd.update_precond_kron_quad_(Ql, Qr, torch.zeros(3), G, 0.1)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        psgd.update_precond_kron_quad_(Ql, Qr, L, G, 0.1)


def test_every_compute_entry_point_has_an_extent_test():
    """tests/test_cabi_cpu.py's rule for this header: no kernel without a guard-band test, in the entry table of
    tests/test_kron_quad_extents_gpu.py and really called there."""
    from tests import test_kron_quad_extents_gpu as ext
    compute = set(kron_quad.SIGNATURES) - {"psgd_kron_quad_workspace_bytes"}
    assert set(ext.ENTRY_POINTS.values()) == compute and len(ext.ENTRY_POINTS) == len(compute)
    src = open(ext.__file__).read()
    for name in sorted(compute):
        assert "lib.%s(" % name in src, name + " is in the entry table but nothing calls it"
    assert "arena.check()" in src and set(ext.FILLS) == {0xA5, 0xFF}


def _least_tile_density(mask):
    T = qc.T
    return min(float(mask[i:i + T, j:j + T].double().mean()) for i in range(0, mask.shape[0], T) for j in range(0, mask.shape[1], T))


@pytest.mark.parametrize("M, N, seed", qc.EXACT_CASES)
def test_exact_cases_are_exact_in_any_summation_order(M, N, seed):
    """The conditions under which tests/test_kron_quad_exact_gpu.py may ask for equal bits, decided here and not by a kernel."""
    p = qc.exact_problem(M, N, seed)
    Ql, Qr, G = p["Ql"], p["Qr"], p["G"]
    assert torch.equal(Ql, Ql.T) and torch.equal(Qr, Qr.T) and int((G.abs().sum(0) == 0).sum()) == 0
    assert all(torch.equal(t, t.round()) for t in (Ql, Qr, G)) and float(G.abs().max()) <= 2
    bounds = qc.exact_bounds(p)
    print(M, N, "largest scaled magnitude: %s" % " ".join("%s %.3g" % kv for kv in sorted(bounds.items())))
    assert len(bounds) == 11 and max(bounds.values()) < qc.EXACT_LIMIT, bounds
    d = {k: p[k].double() for k in ("Ql", "Qr", "G")}
    ell = [float(qc.quad_bound(T_) + t2) for T_, t2 in qc.quad_terms(d["Ql"], d["Qr"], d["G"])]
    assert max(ell) <= qc.EXACT_L0 / 2 and p["L"].tolist() == [qc.EXACT_L0] * 2   # a factor of 2, not an fp64 rounding, decides the max
    assert qc.EXACT_C == p["step"] / (2 * qc.EXACT_L0) == 0.25 and p["decay"] == 1.0
    assert torch.equal(qc.quad_apply_ref(Ql, Qr, G).double(), p["out"])
    new = qc.quad_update_ref(Ql, Qr, p["L"], G, p["step"], p["decay"])
    for got, key in zip(new, ("new_Ql", "new_Qr", "new_L")):
        assert got.dtype == torch.float32 and torch.equal(got.double(), p[key]), key
    assert p["new_L"].tolist() == [qc.EXACT_L0] * 2
    for k in ("Ql", "Qr"):                                                  # the update really moves the factors, off the diagonal too
        moved = p["new_" + k] != d[k]
        assert bool(moved.diagonal().any()) and (moved.numel() == 1 or bool((moved & ~torch.eye(len(moved), dtype=torch.bool)).any()))
        assert _least_tile_density(moved) >= 1 / 3                          # ... in every tile, so a wrong tile cannot hide in zeros
    assert _least_tile_density(p["out"] != 0) >= 0.1


@pytest.mark.parametrize("M, N, seed, shift", qc.SHIFT_CASES)
def test_shift_cases_rotate_by_two(M, N, seed, shift):
    p = qc.shift_problem(M, N, seed, shift)
    assert not torch.equal(p["Ql"], p["Ql"].T) and not torch.equal(p["Qr"], p["Qr"].T)
    assert torch.equal(qc.quad_apply_ref(p["Ql"].double(), p["Qr"].double(), p["G"].double()), p["out"])
    assert float(p["out"][0, 2 * shift % N]) == float(p["G"][2 * shift % M, 0]) != 0.0


def _float32_restatement(p):
    """{bar name: largest tile-wise error of the float32 restatement against the float64 one}"""
    out = qc.quad_apply_ref(p["Ql"], p["Qr"], p["G"])
    new_Ql, new_Qr, _ = qc.quad_update_ref(p["Ql"], p["Qr"], p["L"], p["G"])
    out_new = qc.quad_apply_ref(new_Ql, new_Qr, p["G"])
    pairs = [(new_Ql, "Ql"), (new_Qr, "Qr")]
    return dict(apply=max(qc.tile_err(out, p["out"]), qc.tile_err(out_new, p["out_new"])),
                state=max(qc.tile_err(new, p["new_" + k]) for new, k in pairs),
                increment=max(qc.tile_err(new.double() - p[k].double(), p["new_" + k] - p[k].double()) for new, k in pairs))


@pytest.mark.parametrize("case", qc.CASES + [qc.LIP_CASE], ids=lambda c: "-".join(map(str, c)))
def test_float32_restatement_leaves_a_factor_of_three_under_each_tile_bar(case):
    """The tile-wise bars of tests/test_kron_quad_gpu.py are the README's norm-wise ones; that fp32 arithmetic on THESE inputs
    stays under a third of each, tile by tile, is a condition on the inputs (a row that fails it gets another seed)."""
    e = _float32_restatement(qc.problem(*case))
    print(case, "apply %.2e state %.2e increment %.2e" % (e["apply"], e["state"], e["increment"]))
    assert e["apply"] < qc.APPLY_BAR / 3 and e["state"] < qc.STATE_BAR / 3 and e["increment"] < qc.INCREMENT_BAR / 3


def test_tile_err_sees_one_wrong_corner_that_the_norm_hides():
    ref = torch.ones(2 * qc.T + 3, 2 * qc.T + 3, dtype=torch.float64)
    x = ref.clone()
    x[-1, -1] += 1e-3                                                       # alone in a 3 x 3 edge tile
    assert qc.err(x, ref) < 1e-5 < 3e-4 < qc.tile_err(x, ref)
    assert qc.tile_err(ref, ref) == 0.0 and qc.tile_err(x[:1, :1], ref[:1, :1]) == 0.0


def test_lipschitz_case_chooses_a_column_past_1024():
    M, N, seed, col = qc.LIP_CASE
    p = qc.problem(M, N, seed, col)                                         # (asserts the tie condition on both sides)
    Tr = qc.quad_terms(p["Ql"].double(), p["Qr"].double(), p["G"].double())[1][0]
    assert N > 1024 and int(torch.argmax((Tr * Tr).sum(0))) == col >= 1024


@pytest.mark.parametrize("kw", [dict(preconditioner_update="quad"), dict(preconditioner_update="qr", preconditioner_fit="whitening"),
                                dict(preconditioner_update="quad", preconditioner_fit="whitening", operands="bfloat16")])
def test_class_refusals_before_a_device_is_touched(kw):
    with pytest.raises(ValueError, match="preconditioner_update"):
        psgd.Kron([torch.zeros(3, 5, requires_grad=True)], **kw)
