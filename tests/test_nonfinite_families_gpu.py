"""Error convention (see tests/test_nonfinite_gpu.py) of the families that file does not reach: UVd and sparse LU of rank 33 .. 64
(the whole-matrix kernels), the column-chunk route above 64, the matrix-g apply, the UVd balance branch, the fused update -> apply,
and the fold entry points of the row-sharded routes driven directly with a NaN in one rank's slot.

The reference is the fp64 oracle on the same input.  For a NaN input the NaN mask of every output equals the oracle's and what the
oracle leaves untouched keeps its bits; an Inf input only has to leave something non-finite (Inf - Inf patterns depend on the
summation order); zero in gives exact zeros."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from tests.splu_cases import make_splu_problem
from tests.uvd_cases import TINY32, make_uvd_problem

pytestmark = pytest.mark.gpu

# 33, 40, 64: the whole-matrix kernels; 65, 100: column chunks (copies / views); (20, 40): fewer rows than columns
UVD_SHAPES = [(5000, 33), (5000, 40), (5000, 64), (5000, 65), (5000, 100), (20, 40)]
SPLU_SHAPES = [(5003, 33), (5003, 47), (5003, 64), (5003, 65)]


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import preconditioned_stochastic_gradient_descent as m
    return m


_problems = {}


def _uvd(N, r):
    """the problem (fp32 numpy, never modified) and its fp64 copy maker"""
    if (N, r) not in _problems:
        _problems[(N, r)] = make_uvd_problem(N, r, seed=100 + r)
    return _problems[(N, r)]


def _dev(p):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in p.items()}


def _f64(p):
    return {k: v.astype(np.float64) for k, v in p.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mask_equal(got, ref, what):
    g, r = np.isnan(got.cpu().numpy()), np.isnan(ref)
    assert g.shape == r.shape and np.array_equal(g, r), (what, "NaN in got / oracle:", int(g.sum()), int(r.sum()), "of", r.size)


# ------------------------------------------------------------------------------------------------------------------------- UVd
@pytest.mark.parametrize("N,r", UVD_SHAPES)
def test_uvd_wide_apply(psgd, N, r):
    p = _uvd(N, r)
    t, q = _dev(p), _f64(p)
    row = N // 3
    out = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], torch.zeros_like(t["g"]))
    assert float(out.abs().max()) == 0.0
    g = t["g"].clone()
    g[row] = float("nan")
    q["g"][row] = np.nan
    ref = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])
    assert np.isnan(ref).all()                            # the NaN reaches V'(d g), hence every row
    _mask_equal(psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], g), ref, "apply")
    g = t["g"].clone()
    g[row] = float("inf")
    assert not torch.isfinite(psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], g)).all()


@pytest.mark.parametrize("N,r", UVD_SHAPES)
def test_uvd_wide_apply_matrix_g(psgd, N, r):
    """k = 5 columns (one group of four and a remainder), a NaN in column 2 only: it stays in its column"""
    p = _uvd(N, r)
    t, q = _dev(p), _f64(p)
    G = torch.from_numpy(np.random.default_rng(5).standard_normal((N, 5)).astype(np.float32)).cuda()
    clean = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], G)
    assert torch.isfinite(clean).all()
    Gb = G.clone()
    Gb[N // 3, 2] = float("nan")
    out = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], Gb)
    ref = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], Gb.cpu().numpy().astype(np.float64))
    assert np.isnan(ref[:, 2]).all() and not np.isnan(ref[:, [0, 1, 3, 4]]).any()
    _mask_equal(out[:, 2], ref[:, 2], "column 2")
    for j in (0, 1, 3, 4):
        assert torch.equal(_bits(out[:, j]), _bits(clean[:, j])), j


def _nan_h(N, r):
    p = _uvd(N, r)
    t, q = _dev(p), _f64(p)
    t["h"][N // 3] = float("nan")
    q["h"][N // 3] = np.nan
    return p, t, q


@pytest.mark.parametrize("update_U", [True, False])
@pytest.mark.parametrize("N,r", UVD_SHAPES)
def test_uvd_wide_update(psgd, N, r, update_U):
    """a NaN in one row of h: a = Qh and nablaD are NaN everywhere, so d and the updated factor are; the other factor is not read for
    writing and keeps its bits"""
    p, t, q = _nan_h(N, r)
    psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], 0.01, TINY32, balance=False, update_U=update_U)
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], 0.01, TINY32, balance=False, update_U=update_U)
    upd, other = ("U", "V") if update_U else ("V", "U")
    assert np.isnan(q["d"]).all() and torch.isnan(t["d"]).all()
    _mask_equal(t["d"], q["d"], "d")
    _mask_equal(t[upd], q[upd], upd)
    assert torch.equal(_bits(t[other]), _bits(torch.from_numpy(p[other]).cuda())), other


@pytest.mark.parametrize("N,r", UVD_SHAPES + [(5000, 10)])
def test_uvd_balance_branch(psgd, N, r):
    """psgd.py:563-564: a NaN in one element of U makes max|U| and rho NaN, and with them both factors entirely"""
    p = _uvd(N, r)
    for update_U in (True, False):
        t, q = _dev(p), _f64(p)
        t["U"][N // 2, r // 2] = float("nan")
        q["U"][N // 2, r // 2] = np.nan
        psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], 0.01, TINY32, balance=True, update_U=update_U)
        with np.errstate(invalid="ignore"):
            orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], 0.01, TINY32, balance=True, update_U=update_U)
        assert np.isnan(q["U"]).all() and np.isnan(q["V"]).all()
        for k in ("U", "V", "d"):
            _mask_equal(t[k], q[k], (k, update_U))


@pytest.mark.parametrize("update_U", [True, False])
@pytest.mark.parametrize("N,r", UVD_SHAPES)
def test_uvd_wide_fused_update_apply(psgd, N, r, update_U):
    """the UVd.step pattern (ranks 33 .. 64: psgd_uvd_wide_update_apply_f32): the state as in the unfused update, out all NaN"""
    p, t, q = _nan_h(N, r)
    out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], 0.01, TINY32,
                                                        balance=False, update_U=update_U)
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], 0.01, TINY32, balance=False, update_U=update_U)
    ref = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])
    upd, other = ("U", "V") if update_U else ("V", "U")
    assert np.isnan(ref).all() and np.isnan(q["d"]).all()
    _mask_equal(out, ref, "out")
    _mask_equal(t["d"], q["d"], "d")
    _mask_equal(t[upd], q[upd], upd)
    assert torch.equal(_bits(t[other]), _bits(torch.from_numpy(p[other]).cuda())), other


# ------------------------------------------------------------------------------------------------------------------- sparse LU
@pytest.mark.parametrize("N,r", SPLU_SHAPES)
def test_splu_wide(psgd, N, r):
    p = make_splu_problem(N, r, seed=200 + r)
    t, q = _dev(p), _f64(p)
    keys = ("L12", "l3", "U12", "u3")
    st = [t[k] for k in keys]
    assert float(psgd.precond_grad_splu(*st, [torch.zeros_like(t["g"])])[0].abs().max()) == 0.0
    g = t["g"].clone()
    g[4000] = float("nan")
    q["g"][4000] = np.nan
    ref = orc.precond_grad_splu(*[q[k] for k in keys], [q["g"]])[0]
    _mask_equal(psgd.precond_grad_splu(*st, [g])[0], ref, "apply")
    g = t["g"].clone()
    g[4000] = float("inf")
    assert not torch.isfinite(psgd.precond_grad_splu(*st, [g])[0]).all()
    dx = t["dx"].clone()
    dx[3] = float("nan")
    q["dx"][3] = np.nan
    new = psgd.update_precond_splu(*st, [dx], [t["dg"]], 0.1)
    with np.errstate(invalid="ignore"):
        want = orc.update_precond_splu(*[q[k] for k in keys], [q["dx"]], [q["dg"]], 0.1)
    assert all(np.isnan(w).any() for w in want)
    for k, a, b in zip(keys, new, want):
        _mask_equal(a, b, k)
    for k, a in zip(keys, st):                            # the call is pure: the inputs keep their bits
        assert torch.equal(_bits(a), _bits(torch.from_numpy(p[k]).cuda())), k


# ------------------------------------------------------------------------------------------------- folds of the sharded routes
# family -> (workspace bytes, region query, fold, {stage: number of leading SUM entries, None = all, 0 = none (all maxima)})
def _families(r):
    return {
        "uvd": ("psgd_uvd_workspace_bytes", "psgd_uvd_ws_region", "psgd_uvd_fold_gathered_f64",
                {1: None, 2: None, 11: None, 10: 0, 12: 0, 13: 4 * r}),
        "splu": ("psgd_splu_workspace_bytes", "psgd_splu_ws_region", "psgd_splu_fold_gathered_f64", {1: None, 2: None, 3: r}),
        "uvd_bf16": ("psgd_uvd_bf16_workspace_bytes", "psgd_uvd_bf16_ws_region", "psgd_uvd_bf16_fold_gathered_f64",
                     {1: None, 2: None, 11: None, 10: 0, 12: 0}),
    }


def _region(lib, fn, which, stage, N, r):
    off, cnt = ctypes.c_int64(0), ctypes.c_int64(0)
    assert getattr(lib, fn)(which, stage, N, r, ctypes.byref(off), ctypes.byref(cnt)) == 0, (fn, which, stage)
    return off.value, cnt.value


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("r", [10, 32])
@pytest.mark.parametrize("family", ["uvd", "splu", "uvd_bf16"])
def test_fold_gathered(hip_lib, family, r, world):
    """psgd_*_fold_gathered_f64 on a synthetic [world][count] buffer, no process group: the sum slots are the fp64 sum in rank
    order (bit-equal to numpy's), the maximum slots the exact maximum -- and NaN, in the fp64 region AND in the fp32 word(s) the
    next kernel reads, when exactly one rank's slot holds a NaN, whichever rank that is.  The fp32 words are found as what the fold
    changed outside the send region (and, where the family reports its fp32 maximum region, checked to be that region)."""
    from psgd_tf_amd import _lib
    N = 1021
    wsb, regf, foldf, stages = _families(r)[family]
    nbytes = int(getattr(hip_lib, wsb)(N, r))
    assert nbytes > 0
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(1000 * r + world)
    for stage, nsum in stages.items():
        off, cnt = _region(hip_lib, regf, _lib.PSGD_WS_SEND_F64, stage, N, r)
        nsum = cnt if nsum is None else nsum
        nmax = cnt - nsum
        nan_cases = [None] + ([(k, j) for k in range(world) for j in range(nmax)] if nmax else [])
        for nan_at in nan_cases:
            host = rng.standard_normal((world, cnt))
            host[:, nsum:] = np.abs(host[:, nsum:]).astype(np.float32)          # maxima travel as (double)float
            if nan_at is not None:
                host[nan_at[0], nsum + nan_at[1]] = np.nan
            want = host[0].copy()
            for k in range(1, world):                                            # rank order
                want[:nsum] = want[:nsum] + host[k][:nsum]
            if nmax:
                want[nsum:] = np.max(host[:, nsum:], axis=0)                     # numpy's max propagates NaN
            ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
            gathered = torch.from_numpy(host.reshape(-1)).cuda()
            assert getattr(hip_lib, foldf)(stage, gathered.data_ptr(), world, N, r, ws.data_ptr(), ws.numel(), st) == 0
            raw = ws.cpu().numpy()
            got = raw[off:off + 8 * cnt].view(np.float64)
            tag = (family, stage, world, nan_at)
            if family == "uvd_bf16" and stage == 11:
                # include/psgd_hip.h: the folded Gram is an fp64 [.][80] matrix of which the first 16 ceil((2r + 6) / 16) columns
                # are in use; the fold leaves the others alone
                used = (np.arange(cnt) % 80) < 16 * ((2 * r + 6 + 15) // 16)
                assert np.array_equal(got[used].view(np.int64), want[used].view(np.int64)), tag
                assert (raw[off:off + 8 * cnt].reshape(-1, 8)[~used] == 0x5A).all(), tag
                continue
            assert np.array_equal(got[:nsum].view(np.int64), want[:nsum].view(np.int64)), tag
            assert np.array_equal(np.isnan(got[nsum:]), np.isnan(want[nsum:])), tag
            ok = ~np.isnan(want[nsum:])
            assert np.array_equal(got[nsum:][ok], want[nsum:][ok]), tag
            if nan_at is not None:
                assert np.isnan(got[nsum + nan_at[1]]), tag
            if not nmax:
                continue
            words = raw.view(np.uint32).copy()
            words[off // 4:off // 4 + 2 * cnt] = 0x5A5A5A5A                      # (mask the send region out)
            changed = np.nonzero(words != 0x5A5A5A5A)[0]
            f32 = words[changed].view(np.float32)
            w32 = want[nsum:].astype(np.float32)
            assert changed.size == nmax and np.array_equal(np.diff(changed), np.ones(nmax - 1, dtype=changed.dtype)), (tag, changed)
            assert np.array_equal(np.isnan(f32), np.isnan(w32)) and np.array_equal(f32[~np.isnan(w32)], w32[~np.isnan(w32)]), tag
            if nan_at is not None:
                assert np.isnan(f32[nan_at[1]]), tag
            if family != "uvd_bf16":                                             # the fp32 maximum region the family reports
                mstage = 12 if (family, stage) == ("uvd", 13) else stage
                moff, mcnt = _region(hip_lib, regf, _lib.PSGD_WS_MAX_F32, mstage, N, r)
                assert (moff // 4, mcnt) == (int(changed[0]), nmax), tag
