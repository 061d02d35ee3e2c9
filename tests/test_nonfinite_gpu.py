"""Error convention of the hot path (reference README.md:56): no exceptions, NaN/Inf propagate silently --
and zero inputs give exact zeros.  Checked for every HIP entry point family; this file holds the first three rows:

    UVd, r <= 32 (r = 10): apply, update, the NaN-propagating maxima     here; the balance branch at r = 10: test_nonfinite_families_gpu.py
    sparse LU, r <= 32 (r = 7)                                           here
    Kron (small, large and bf16-operand routes, its balance branch)      here
    UVd ranks 33 .. 64 (whole-matrix kernels) and above (column chunks), N < r, the matrix-g apply, the balance branch,
      the fused update -> apply; sparse LU ranks 33 .. 65                 test_nonfinite_families_gpu.py (masks against the oracle)
    fold entry points of the row-sharded routes (fp32 UVd, sparse LU,
      bf16 UVd), a NaN in one rank's slot                                test_nonfinite_families_gpu.py::test_fold_gathered
    dense preconditioner                                                 test_dense_gpu.py::test_nan_propagates
    bf16-state UVd kernels                                               test_uvd_bf16_gpu.py::test_nan_in_h_propagates
    step-tail kernels (pack, sum of squares, parameter update, clip)     test_uvd_tail_gpu.py (special values, NaN clip norm)
    row-sharded wide ranks, a NaN that one rank alone owns               test_sharded_cpu.py (gloo), test_sharded_2proc_gpu.py"""
import numpy as np
import pytest
import torch

from tests.splu_cases import make_splu_problem
from tests.uvd_cases import TINY32, make_uvd_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import preconditioned_stochastic_gradient_descent as m
    return m


def _dev(p):
    return {k: torch.from_numpy(v).cuda() for k, v in p.items()}


def test_uvd_nan_propagates_and_zero_stays_zero(psgd):
    t = _dev(make_uvd_problem(5000, 10, seed=1))
    assert float(psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], torch.zeros_like(t["g"])).abs().max()) == 0.0
    g = t["g"].clone()
    g[1234] = float("nan")
    out = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], g)
    assert torch.isnan(out).all()                         # a NaN in g reaches V'(d g), hence every row
    g = t["g"].clone()
    g[77] = float("inf")
    assert not torch.isfinite(psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], g)).all()
    h = t["h"].clone()
    h[5] = float("nan")
    psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], h, 0.01, TINY32, balance=False, update_U=True)
    assert torch.isnan(t["U"]).any() and torch.isnan(t["d"]).any()      # silently poisoned state, no exception


def test_maxima_propagate_nan_like_tf_reduce_max(psgd, hip_lib):
    """tf.reduce_max returns NaN if any element is NaN, so the step sizes of psgd.py:582, :177-178, :41 become NaN and the
    WHOLE updated factor is NaN -- a hardware max (fmaxf / v_max_f32) returns the non-NaN operand and would hide the NaN
    behind a finite step.  UVd: a NaN that reaches only nablaD (through the per-row d, not through any inner product);
    Kron: a NaN in one gradient entry; the balance branch."""
    import ctypes
    from psgd_tf_amd import _lib
    N, r = 5000, 10
    t = _dev(make_uvd_problem(N, r, seed=3))
    # the raw max reduction of sweep 2: plant a NaN in the workspace of block maxima is not reachable from outside, so
    # go through the call: v = 0 except one NaN row keeps every column sum finite?  no -- w = v/d enters the Gram.  Use the
    # staged entry points instead: run sweep 1 on clean data, then sweep 2 with a NaN in v (row-local only from here on).
    ws = psgd.uvd_workspace(t["U"].device, N, r)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda x: x.data_ptr()
    assert hip_lib.psgd_uvd_update_sweep1_f32(P(t["U"]), P(t["V"]), P(t["d"]), P(t["v"]), P(t["h"]), N, r, P(ws), ws.numel(), st) == 0
    v = t["v"].clone()
    v[321] = float("nan")
    d0 = t["d"].clone()
    assert hip_lib.psgd_uvd_update_sweep2_f32(P(t["U"]), P(t["V"]), P(t["d"]), P(v), P(t["h"]), N, r, 0.01, TINY32, 1, P(ws), ws.numel(), st) == 0
    assert hip_lib.psgd_uvd_update_sweep3_f32(P(t["d"]), N, r, 0.01, TINY32, P(ws), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(t["d"]).all(), "max|nablaD| must be NaN -> mu NaN -> every d_i NaN (psgd.py:582-584)"
    assert int(torch.isnan(t["U"]).sum()) == r          # the U rows themselves only see the NaN row-locally (:600)
    # Kron: one NaN in dG -> NaN rows/columns of A -> max|grad| NaN -> both factors entirely NaN (psgd.py:177-179)
    rng = np.random.default_rng(0)
    M, Nn = 151, 16
    Ql = torch.from_numpy((np.triu(rng.standard_normal((M, M)) * 0.05, 1) + np.eye(M)).astype(np.float32)).cuda()
    Qr = torch.from_numpy((np.triu(rng.standard_normal((Nn, Nn)) * 0.05, 1) + np.eye(Nn)).astype(np.float32)).cuda()
    dX = torch.from_numpy(rng.standard_normal((M, Nn)).astype(np.float32)).cuda()
    dG = dX.clone()
    dG[7, 3] = float("nan")
    up = lambda x: x[torch.triu(torch.ones_like(x)).bool()]           # the factors' upper triangles (what is ever read)
    a, b = psgd.update_precond_kron(Ql, Qr, dX, dG, 0.01)
    assert torch.isnan(up(a)).all() and torch.isnan(up(b)).all()
    # balance (psgd.py:166-170): a NaN on a diagonal makes rho NaN
    Qb = Ql.clone()
    Qb[5, 5] = float("nan")
    a, b = psgd.update_precond_kron(Qb, Qr, dX, dX, 0.01)
    assert torch.isnan(up(a)).all() and torch.isnan(up(b)).all()


def test_splu_nan_propagates_and_zero_stays_zero(psgd):
    t = _dev(make_splu_problem(5003, 7, seed=2))
    st = [t[k] for k in ("L12", "l3", "U12", "u3")]
    assert float(psgd.precond_grad_splu(*st, [torch.zeros_like(t["g"])])[0].abs().max()) == 0.0
    g = t["g"].clone()
    g[4000] = float("nan")
    assert torch.isnan(psgd.precond_grad_splu(*st, [g])[0]).all()
    dx = t["dx"].clone()
    dx[3] = float("nan")
    new = psgd.update_precond_splu(*st, [dx], [t["dg"]], 0.1)
    assert all(torch.isnan(x).any() for x in new)


def test_kron_nan_propagates_and_zero_stays_zero(psgd):
    rng = np.random.default_rng(0)
    M, N = 151, 16
    Ql = torch.from_numpy((np.triu(rng.standard_normal((M, M)) * 0.05, 1) + np.eye(M)).astype(np.float32)).cuda()
    Qr = torch.from_numpy((np.triu(rng.standard_normal((N, N)) * 0.05, 1) + np.eye(N)).astype(np.float32)).cuda()
    G = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda()
    assert float(psgd.precond_grad_kron(Ql, Qr, torch.zeros_like(G)).abs().max()) == 0.0
    G[7, 3] = float("nan")
    assert torch.isnan(psgd.precond_grad_kron(Ql, Qr, G)).any()
    a, b = psgd.update_precond_kron(Ql, Qr, G, G, 0.01)
    assert torch.isnan(a).any() or torch.isnan(b).any()


@pytest.mark.parametrize("M,N", [(640, 512), (1024, 1536)])
def test_kron_large_and_bf16_paths_propagate_nan(psgd, M, N):
    """The large-problem kernels (bf16 x 3 split GEMMs with the truncating split, register-resident solve strips, the
    bf16-operand apply and update): zero in -> zero out for the apply, a NaN / Inf in the data reaches the outputs."""
    rng = np.random.default_rng(1)
    tri = lambda n: torch.from_numpy((np.triu(rng.standard_normal((n, n)) * (0.3 / n ** 0.5), 1) + np.eye(n)).astype(np.float32)).cuda()
    Ql, Qr = tri(M), tri(N)
    G = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda()
    dX = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).cuda()
    assert float(psgd.precond_grad_kron(Ql, Qr, torch.zeros_like(G)).abs().max()) == 0.0
    assert float(psgd.precond_grad_kron(Ql, Qr, torch.zeros_like(G).bfloat16()).float().abs().max()) == 0.0
    for bad in (float("nan"), float("inf")):
        Gb = G.clone()
        Gb[M // 3, N // 5] = bad
        for data in (Gb, Gb.bfloat16()):
            out = psgd.precond_grad_kron(Ql, Qr, data).float()
            assert not torch.isfinite(out).all()
            a, b = psgd.update_precond_kron(Ql, Qr, dX.to(data.dtype), data, 0.01)
            assert not (torch.isfinite(a).all() and torch.isfinite(b).all())
            a, b = psgd.update_precond_kron(Ql, Qr, data, dX.to(data.dtype), 0.01)      # through the triangular solves
            assert not (torch.isfinite(a).all() and torch.isfinite(b).all())
