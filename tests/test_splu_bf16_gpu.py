"""The sparse-LU preconditioner on a bf16-stored state (psgd_splu_bf16.hip) against the fp64 oracle on the widened codes (GPU).

Apply: within 1e-5, relative and norm-wise (the project's bar for preconditioned gradients).  Update: the fp64 oracle on the
widened inputs gives the exact new factors; with rounding="nearest" every stored code is the nearest bf16 code of the oracle
value or one of its two neighbours, and the share of codes that are a neighbour is at most twice that of the fp32 kernels'
outputs rounded by torch, plus 1e-4 (both shares are printed per shape; PSGD_SPLU_BF16_PARITY_OUT=<file> writes them); with
rounding="stochastic" every code is one of the two codes bracketing the oracle value."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from psgd_tf_amd import _lib
from tests.splu_cases import make_splu_problem

pytestmark = pytest.mark.gpu

RANKS = (1, 7, 10, 20, 32)
STEP = 0.01


def tile_rows(r):
    """rows of one tile of the kernel family at rank r (make_geo of bf16_state.h)"""
    m = min(256 // r, 32)
    ri = 8 * m
    return (256 // ri) * ri


def shapes(r):
    tr = tile_rows(r)
    return sorted({n for n in (r, r + 1, 63, 64, 65, 257, 1021, 4099, 2 * tr - 1, 2 * tr + 1) if n >= r})


@pytest.fixture(scope="module")
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


# ------------------------------------------------------------------ bf16 codes as ordered integers
def ordered(codes):
    """bf16 codes (int64, 0 .. 65535) -> integers in the order of the values they stand for (+0 and -0 both 0)"""
    mag = codes & 0x7fff
    return np.where(codes & 0x8000, -mag, mag)


def value(o):
    """the fp64 value of an ordered code"""
    code = np.where(o < 0, (-o) | 0x8000, o).astype(np.uint32)
    return (code << np.uint32(16)).view(np.float32).astype(np.float64)


def codes_of(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.int64).reshape(-1) & 0xffff


def nearest(v):
    """ordered code of the bf16 value nearest to the fp64 value v (ties to the even code)"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    with np.errstate(over="ignore"):
        o0 = ordered((v.astype(np.float32).view(np.uint32) >> 16).astype(np.int64))
    best, bd = o0.copy(), np.abs(value(o0) - v)
    for o in (o0 - 1, o0 + 1):
        d = np.abs(value(o) - v)
        take = (d < bd) | ((d == bd) & (o % 2 == 0) & (best % 2 != 0))
        best, bd = np.where(take, o, best), np.where(take, d, bd)
    return best


def widen64(t):
    return t.detach().cpu().float().numpy().astype(np.float64)


# ------------------------------------------------------------------ problems, stored state and references (computed once)
_cache = {}


def problem(N, r, seed=0):
    """(bf16 state on the device, fp32 dx, dg, g on the device, the fp64 oracle's new factors and preconditioned gradient)"""
    key = (N, r, seed)
    if key not in _cache:
        p = make_splu_problem(N, r, seed=seed + 7 * N + r)
        st = [torch.from_numpy(p[k]).cuda().bfloat16() for k in ("L12", "l3", "U12", "u3")]
        vec = {k: torch.from_numpy(p[k]).cuda() for k in ("dx", "dg", "g")}
        w = [widen64(t) for t in st]
        with np.errstate(all="ignore"):
            new = orc.update_precond_splu(*w, [p["dx"].astype(np.float64)], [p["dg"].astype(np.float64)], STEP)
            pre = orc.precond_grad_splu(*w, [p["g"].astype(np.float64)])[0]
        _cache[key] = (st, vec, new, pre)
    return _cache[key]


def off_by(out, ref):
    """|ordered code of the output - nearest ordered code of the oracle value|, all four tensors in one array"""
    return np.concatenate([np.abs(ordered(codes_of(o)) - nearest(x)) for o, x in zip(out, ref)])


def brackets(out, ref):
    """every stored code is one of the two codes bracketing the oracle value"""
    for o, x in zip(out, ref):
        oc, x = ordered(codes_of(o)), np.asarray(x, dtype=np.float64).reshape(-1)
        v = value(oc)
        ok = ((v <= x) & (value(oc + 1) > x)) | ((v >= x) & (value(oc - 1) < x))
        if not ok.all():
            return False
    return True


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("r", RANKS)
def test_apply_matches_the_oracle_on_the_stored_codes(psgd, r):
    for N in shapes(r):
        st, vec, _, pre = problem(N, r)
        out = psgd.precond_grad_splu(*st, [vec["g"]])[0]
        assert out.dtype == torch.float32 and out.shape == vec["g"].shape
        got = out.cpu().numpy().astype(np.float64)
        err = np.linalg.norm(got - pre) / np.linalg.norm(pre)
        print("apply N=%d r=%d rel err %.3g" % (N, r, err))
        assert err <= 1e-5, (N, r, err)


# ------------------------------------------------------------------ update, nearest
@pytest.mark.parametrize("r", RANKS)
def test_update_nearest_codes_and_parity_with_the_fp32_kernels(psgd, r):
    rows = []
    for N in shapes(r):
        st, vec, new, _ = problem(N, r)
        before = [t.clone() for t in st]
        out = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP)
        assert all(o.dtype == torch.bfloat16 and o.shape == t.shape for o, t in zip(out, st))
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(before, st)), "inputs modified"
        d = off_by(out, new)
        ref32 = psgd.update_precond_splu(*[t.float() for t in st], [vec["dx"]], [vec["dg"]], STEP)
        d32 = off_by([t.bfloat16() for t in ref32], new)
        share, share32 = float((d != 0).mean()), float((d32 != 0).mean())
        rows.append("N=%d r=%d codes=%d bf16_share=%.3e fp32_share=%.3e" % (N, r, d.size, share, share32))
        print(rows[-1])
        assert d.max() <= 1, (N, r, int(d.max()))
        assert share <= 2.0 * share32 + 1e-4, (N, r, share, share32)
    path = os.environ.get("PSGD_SPLU_BF16_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(rows) + "\n")


def test_tail_vectors_as_columns_or_flat(psgd):
    N, r = 257, 7
    st, vec, _, _ = problem(N, r)
    flat = [st[0], st[1].reshape(-1), st[2], st[3].reshape(-1)]
    a = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP)
    b = psgd.update_precond_splu(*flat, [vec["dx"]], [vec["dg"]], STEP)
    assert b[1].shape == (N - r,) and a[1].shape == (N - r, 1)
    assert all(torch.equal(x.reshape(-1).view(torch.int16), y.reshape(-1).view(torch.int16)) for x, y in zip(a, b))
    assert torch.equal(psgd.precond_grad_splu(*st, [vec["g"]])[0], psgd.precond_grad_splu(*flat, [vec["g"]])[0])


def test_no_tail(psgd):
    """N = r: l3 and u3 are empty, reduce_max over them is -inf and the tail maxima are 0"""
    for r in (1, 10, 32):
        st, vec, new, pre = problem(r, r)
        assert st[1].numel() == 0
        out = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP)
        assert out[1].numel() == 0 and out[3].numel() == 0
        assert off_by(out, new).max() <= 1
        got = psgd.precond_grad_splu(*st, [vec["g"]])[0].cpu().numpy().astype(np.float64)
        assert np.linalg.norm(got - pre) <= 1e-5 * np.linalg.norm(pre)


# ------------------------------------------------------------------ update, stochastic
@pytest.mark.parametrize("r", RANKS)
def test_update_stochastic_brackets_and_is_reproducible(psgd, r):
    for N in shapes(r):
        st, vec, new, _ = problem(N, r)
        upd = lambda seed: psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP, rounding="stochastic", rounding_seed=seed)
        a, b, c = upd(11), upd(11), upd(12)
        assert brackets(a, new) and brackets(c, new), (N, r)
        assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b)), (N, r)
        if N * r >= 64:
            assert any(not torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, c)), (N, r)


def test_stochastic_seed_is_drawn_from_the_branch_generator(psgd):
    st, vec, new, _ = problem(257, 7)
    psgd.manual_seed(5)
    a = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP, rounding="stochastic")
    b = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP, rounding="stochastic")
    psgd.manual_seed(5)
    c = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP, rounding="stochastic")
    assert brackets(a, new) and brackets(b, new)
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, c))
    assert any(not torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))


def biased_problem(N=4099, r=10):
    """A state on which round-to-nearest is biased: max_l = 1 + 2^-7 and max_u = 1 (both bf16 codes), so rho = sqrt(1 + 2^-7)
    = 1 + 2^-8 - ... and l3 / rho lies (m / 2) ulp below the code l3 = m 2^e, m in [1, 2): between half an ulp and one ulp, so
    nearest lands on the code below and is too small by up to half an ulp, every time.  The step is 1e-6: the gradient
    term moves a value by far less than an ulp."""
    rng = np.random.default_rng(4099)
    p = make_splu_problem(N, r, seed=1)
    bf = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16()
    L12, U12 = p["L12"].copy(), p["U12"].copy()
    L12[np.arange(r), np.arange(r)] = rng.uniform(0.5, 1.0, r)
    U12[np.arange(r), np.arange(r)] = rng.uniform(0.5, 1.0, r)
    L12[0, 0], U12[0, 0] = 1.0 + 2.0 ** -7, 1.0
    l3, u3 = rng.uniform(0.5, 1.0, (N - r, 1)), rng.uniform(0.35, 0.7, (N - r, 1))
    st = [bf(L12), bf(l3), bf(U12), bf(u3)]
    w = [widen64(t) for t in st]
    new = orc.update_precond_splu(*w, [p["dx"].astype(np.float64)], [p["dg"].astype(np.float64)], 1e-6)
    return st, p, new


def test_stochastic_rounding_removes_the_bias_of_nearest(psgd):
    st, p, new = biased_problem()
    ref = new[1].reshape(-1)
    # the oracle side, on the CPU: rounding the exact l3 to nearest is biased, by about a quarter of an ulp (2^-9 relative)
    cpu_bias = float(np.mean(value(nearest(ref)) - ref))
    assert cpu_bias < -2.0 ** -11, cpu_bias
    st = [t.cuda() for t in st]
    dx, dg = torch.from_numpy(p["dx"]).cuda(), torch.from_numpy(p["dg"]).cuda()
    near = psgd.update_precond_splu(*st, [dx], [dg], 1e-6)
    bias_nearest = float(np.mean(widen64(near[1]).reshape(-1) - ref))
    acc = np.zeros_like(ref)
    for seed in range(64):
        out = psgd.update_precond_splu(*st, [dx], [dg], 1e-6, rounding="stochastic", rounding_seed=seed)
        acc += widen64(out[1]).reshape(-1) - ref
    bias_stochastic = float(np.mean(acc / 64))
    print("mean(l3 - oracle): nearest %.3e (on the CPU %.3e)  stochastic over 64 seeds %.3e" % (bias_nearest, cpu_bias, bias_stochastic))
    assert abs(bias_nearest - cpu_bias) <= 0.05 * abs(cpu_bias)
    assert abs(bias_stochastic) < abs(bias_nearest)


# ------------------------------------------------------------------ non-finite contract
def _substitution(A, b, lower, adjoint=False):
    """A triangular solve by plain substitution: a zero on the diagonal divides (inf, NaN), as tf.linalg.triangular_solve and the
    kernels do, where the LAPACK routine behind the oracle's solve refuses the matrix as singular."""
    T = A.T if adjoint else A
    low = lower != adjoint
    x = np.array(b, dtype=np.float64).reshape(-1)
    n = x.size
    for p in (range(n) if low else range(n - 1, -1, -1)):
        x[p] = x[p] / T[p, p]
        rest = slice(p + 1, n) if low else slice(0, p)
        x[rest] -= T[rest, p] * x[p]
    return x.reshape(-1, 1)


def _nan_masks(psgd, st, dx, dg, monkeypatch=None):
    w = [widen64(t) for t in st]
    with np.errstate(all="ignore"):
        try:
            ref = orc.update_precond_splu(*w, [widen64(dx)], [widen64(dg)], STEP)
        except np.linalg.LinAlgError:        # a balance with rho = 0 leaves a zero diagonal: the same oracle, solves by substitution
            monkeypatch.setattr(orc, "_tri_solve", _substitution)
            ref = orc.update_precond_splu(*w, [widen64(dx)], [widen64(dg)], STEP)
            monkeypatch.undo()
    out = psgd.update_precond_splu(*st, [dx], [dg], STEP)
    return [np.isnan(widen64(o)).reshape(-1) for o in out], [np.isnan(x).reshape(-1) for x in ref], out, ref


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("where", ["dg", "L12", "u3"])
def test_nonfinite_element_gives_the_oracles_nan_mask(psgd, monkeypatch, where, bad):
    N, r = 1021, 7
    st, vec, _, _ = problem(N, r)
    st, dx, dg = [t.clone() for t in st], vec["dx"].clone(), vec["dg"].clone()
    if where == "dg":
        dg[600, 0] = bad
    elif where == "L12":
        st[0][500, 3] = bad
    else:
        st[3][300, 0] = bad
    got, want, _, _ = _nan_masks(psgd, st, dx, dg, monkeypatch)
    for name, a, b in zip(("L12", "l3", "U12", "u3"), got, want):
        assert np.array_equal(a, b), "%s: %d NaN, the oracle has %d (%s in %s)" % (name, a.sum(), b.sum(), bad, where)


def test_zero_dx_and_dg(psgd):
    """max_abs_grad = 0: step0 = step / tiny, times a zero gradient -- the new factors are the balanced old ones"""
    for N, r in ((257, 10), (10, 10)):
        st, vec, _, _ = problem(N, r)
        z = torch.zeros_like(vec["dx"])
        got, want, out, ref = _nan_masks(psgd, st, z, z)
        assert not any(m.any() for m in got) and not any(m.any() for m in want)
        assert off_by(out, ref).max() <= 1


# ------------------------------------------------------------------ first call on a poisoned workspace
def test_first_call_equals_second(psgd, monkeypatch):
    from tests.test_first_call_gpu import _Poison, _twice
    poison = _Poison(monkeypatch)
    try:
        for N, r in ((1021, 10), (4099, 32), (7, 7)):
            st, vec, new, pre = problem(N, r)
            _twice(lambda: psgd.precond_grad_splu(*st, [vec["g"]]), poison)
            _twice(lambda: psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP), poison)
            _twice(lambda: psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP, rounding="stochastic", rounding_seed=3), poison)
            poison.reset()
            out = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP)
            got = psgd.precond_grad_splu(*st, [vec["g"]])[0].cpu().numpy().astype(np.float64)
            assert off_by(out, new).max() <= 1
            assert np.linalg.norm(got - pre) <= 1e-5 * np.linalg.norm(pre)
    finally:
        monkeypatch.undo()
        poison.reset()


# ------------------------------------------------------------------ the C ABI with raw pointers
def test_c_abi_with_raw_pointers(psgd):
    N, r = 1021, 20
    st, vec, new, pre = problem(N, r)
    lib = _lib.load()
    need = lib.psgd_splu_bf16_workspace_bytes(N, r)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.full_like(vec["g"], float("nan"))
    rc = lib.psgd_splu_apply_bf16(*map(ptr, st), ptr(vec["g"]), ptr(out), N, r, ptr(ws), need, stream)
    assert rc == 0
    got = out.cpu().numpy().astype(np.float64)
    assert np.linalg.norm(got - pre) <= 1e-5 * np.linalg.norm(pre)
    fresh = [torch.full_like(t, float("nan")) for t in st]
    rc = lib.psgd_splu_update_bf16(*map(ptr, st), ptr(vec["dx"]), ptr(vec["dg"]), *map(ptr, fresh), N, r, STEP, float(psgd._tiny), 0, 0,
                                   ptr(ws), need, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert off_by(fresh, new).max() <= 1
    host = psgd.update_precond_splu(*st, [vec["dx"]], [vec["dg"]], STEP)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(fresh, host))
    # aliasing is refused, on the device as on the host
    rc = lib.psgd_splu_update_bf16(*map(ptr, st), ptr(vec["dx"]), ptr(vec["dg"]), *map(ptr, st), N, r, STEP, float(psgd._tiny), 0, 0,
                                   ptr(ws), need, stream)
    assert rc == _lib.PSGD_ERR_BAD_ARG
