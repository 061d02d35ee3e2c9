"""The bf16-stored UVd state (psgd_uvd_bf16.hip) against the fp64 oracle (GPU).

Inputs: tests/uvd_cases.py problems with U, V, d rounded to bf16 first; the oracle runs in fp64 on those same (widened) values, so
the only differences are the kernels' fp32 arithmetic and the one final rounding.  y64 = the oracle's result, s(y) = the bf16 spacing
at y.  Bounds:
  * apply, and the fused call's gradient (against the oracle applied to the state the call STORED): 1e-5, relative, norm-wise;
  * every stored element: |stored - y64| <= 2^-7 |y64| + 1e-5 rms(y64) (the right code or its neighbour);
  * the share of stored codes that differ from RNE_bf16(y64) (stochastic: that are neither floor nor ceil of y64) is measured
    against the same share of the existing fp32 kernels on the widened inputs, rounded to bf16 (the `widen` route):
    p_native <= 2 p_widen + 1e-4;
  * stochastic rounding is unbiased on d where round to nearest is not: slope = <stored - d_old, inc> / <inc, inc>, inc = y64 - d_old,
    |slope - 1| <= 5 sigma with sigma = 0.5 sqrt(sum inc^2 s^2) / sum inc^2 -- and the same assertion fails for "nearest".
The new family has no tuning keys (psgd_set_tuning does not reach it), so there is no grid knob to vary.
Set PSGD_UVD_BF16_PARITY_OUT to a file name to collect the measured p_native / p_widen per case.
"""
import os

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from tests.uvd_cases import TINY32, bf16_grid, check_bf16_state, make_uvd_problem, rel_err, to_bf16_np

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 3, 7, 8, 10, 16, 20, 31, 32)
STEP = 0.01


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import psgd_tf_amd.preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def problem(N, r, seed, d_spread=0.3):
    p = make_uvd_problem(N, r, seed=seed, d_spread=d_spread)
    for k in ("U", "V", "d"):
        p[k] = to_bf16_np(p[k])
    return p


def on_device(p, state_dtype):
    t = {}
    for k, a in p.items():
        x = torch.from_numpy(a).to(_dev())
        t[k] = x.to(state_dtype) if k in ("U", "V", "d") else x
    return t


def widened64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _record(line):
    path = os.environ.get("PSGD_UVD_BF16_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("N", (1, 5, 37, 255, 777, 65539, (1 << 20) + 11))
def test_apply(psgd, N, r):
    p = problem(N, r, seed=N % 97 + r)
    t = on_device(p, torch.bfloat16)
    out = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"])
    ref = orc.precond_grad_UVd_math(*(p[k].astype(np.float64) for k in ("U", "V", "d", "g")))
    assert out.dtype == torch.float32 and out.shape == t["g"].shape
    e = rel_err(out.cpu().numpy(), ref)
    print("apply N=%d r=%d rel err %.2e" % (N, r, e))
    assert e < 1e-5, e


# ------------------------------------------------------------------------------------------------ update, fused call
def _run_update_case(psgd, N, r, update_U, balance, fused, rounding, seed=1234):
    p = problem(N, r, seed=3 * r + N % 89 + 2 * update_U + balance)
    q = {k: v.astype(np.float64) for k, v in p.items()}
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=bool(balance), update_U=bool(update_U))
    # the yardstick: the existing fp32 kernels on the widened inputs (what state_route="widen" computes before it rounds)
    w = on_device(p, torch.float32)
    psgd.update_precond_UVd_math_(w["U"], w["V"], w["d"], w["v"], w["h"], STEP, TINY32, balance=bool(balance), update_U=bool(update_U))
    widen32 = {k: w[k].cpu().numpy() for k in ("U", "V", "d")}
    t = on_device(p, torch.bfloat16)
    kw = dict(balance=bool(balance), update_U=bool(update_U), rounding=rounding, rounding_seed=seed)
    if fused:
        out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32, **kw)
    else:
        assert psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, **kw) is None
    assert all(t[k].dtype == torch.bfloat16 for k in ("U", "V", "d"))
    stored = {k: widened64(t[k]) for k in ("U", "V", "d")}
    written = {"d", "U" if update_U else "V"} | ({"U", "V"} if balance else set())
    for k in ("U", "V"):
        if k not in written:
            assert np.array_equal(stored[k], p[k].astype(np.float64)), k      # the other factor is not touched
    tag = "%s N=%d r=%d update_U=%d balance=%d %s" % ("fused" if fused else "update", N, r, update_U, balance, rounding)
    pn, pw, _ = check_bf16_state(tag, stored, {k: q[k] for k in ("U", "V", "d")}, widen32, written, rounding)
    line = "%s p_native=%.3e p_widen=%.3e" % (tag, pn, pw)
    print(line)
    _record(line)
    assert pn <= 2 * pw + 1e-4, line
    if fused:
        ref = orc.precond_grad_UVd_math(stored["U"], stored["V"], stored["d"], q["g"])
        e = rel_err(out.cpu().numpy(), ref)
        print(tag + " gradient rel err %.2e" % e)
        assert e < 1e-5, (tag, e)
    return t


@pytest.mark.parametrize("fused", (0, 1))
@pytest.mark.parametrize("balance", (0, 1))
@pytest.mark.parametrize("update_U", (1, 0))
@pytest.mark.parametrize("r", RANKS)
def test_update_nearest(psgd, r, update_U, balance, fused):
    for N in (5, 777, 65539):
        _run_update_case(psgd, N, r, update_U, balance, fused, "nearest")


@pytest.mark.parametrize("fused", (0, 1))
@pytest.mark.parametrize("update_U", (1, 0))
def test_update_nearest_large(psgd, update_U, fused):
    _run_update_case(psgd, (1 << 20) + 11, 10, update_U, 0, fused, "nearest")
    _run_update_case(psgd, (1 << 20) + 11, 32, update_U, 1, fused, "nearest")


@pytest.mark.parametrize("fused", (0, 1))
@pytest.mark.parametrize("balance", (0, 1))
@pytest.mark.parametrize("update_U", (1, 0))
@pytest.mark.parametrize("r", RANKS)
def test_update_stochastic_floor_or_ceil(psgd, r, update_U, balance, fused):
    for N in (5, 777, 65539):
        _run_update_case(psgd, N, r, update_U, balance, fused, "stochastic", seed=99 + r)


def _d_slope(psgd, rounding, fused):
    N, r = 262144, 10
    p = problem(N, r, seed=5, d_spread=0.0)          # d = 1 (psgd.py:690): every increment of d is below one bf16 spacing
    q = {k: v.astype(np.float64) for k, v in p.items()}
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=False, update_U=True)
    t = on_device(p, torch.bfloat16)
    kw = dict(balance=False, update_U=True, rounding=rounding, rounding_seed=2024)
    if fused:
        psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32, **kw)
    else:
        psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, **kw)
    d_old = p["d"].astype(np.float64)
    inc = q["d"] - d_old
    s = bf16_grid(q["d"])[3]
    slope = float(np.sum((widened64(t["d"]) - d_old) * inc) / np.sum(inc * inc))
    sigma = float(0.5 * np.sqrt(np.sum(inc * inc * s * s)) / np.sum(inc * inc))
    print("d slope %s fused=%d: %.4f (sigma %.4f)" % (rounding, fused, slope, sigma))
    return slope, sigma


@pytest.mark.parametrize("fused", (0, 1))
def test_stochastic_rounding_is_unbiased_on_d(psgd, fused):
    slope, sigma = _d_slope(psgd, "stochastic", fused)
    assert abs(slope - 1.0) <= 5 * sigma, (slope, sigma)
    slope_n, sigma_n = _d_slope(psgd, "nearest", fused)
    assert not abs(slope_n - 1.0) <= 5 * sigma_n, (slope_n, sigma_n)      # round to nearest loses most of d's increment


def _bits(t):
    return {k: t[k].view(torch.int16).clone() for k in ("U", "V", "d")}


def test_seed_and_stream_reproducibility(psgd):
    N, r = 40003, 20
    p = problem(N, r, seed=8)

    def run(seed, stream=None, fused=True):
        t = on_device(p, torch.bfloat16)
        torch.cuda.synchronize()
        kw = dict(balance=True, update_U=False, rounding="stochastic", rounding_seed=seed)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            if fused:
                out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32, **kw)
            else:
                psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, **kw)
                out = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"])
        torch.cuda.synchronize()
        return _bits(t), out.clone()
    a, oa = run(7)
    b, ob = run(7)
    c, _ = run(8)
    s, os_ = run(7, stream=torch.cuda.Stream())
    u, ou = run(7, fused=False)
    for k in ("U", "V", "d"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], s[k]), k
        assert torch.equal(a[k], u[k]), k            # the update and the fused call store the same state
        assert not torch.equal(a[k], c[k]), k        # balance rewrites both factors: every tensor depends on the seed
    assert torch.equal(oa, ob) and torch.equal(oa, os_) and torch.equal(oa, ou)
    # the draw of a seed comes from the given generator, not from the global CUDA generator
    t1, t2 = on_device(p, torch.bfloat16), on_device(p, torch.bfloat16)
    for t, cuda_seed in ((t1, 1), (t2, 2)):
        torch.cuda.manual_seed(cuda_seed)
        psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=False, update_U=True,
                                      rounding="stochastic", generator=torch.Generator().manual_seed(5))
    assert torch.equal(t1["U"].view(torch.int16), t2["U"].view(torch.int16)) and torch.equal(t1["d"].view(torch.int16), t2["d"].view(torch.int16))


def test_first_call_on_poisoned_memory(psgd, monkeypatch):
    """fresh workspace and outputs filled with 0xFF / NaN, every entry point twice: finite and identical"""
    from psgd_tf_amd import _lib
    orig = torch.empty

    def empty(*a, **k):
        x = orig(*a, **k)
        if x.is_cuda and x.numel():
            if x.dtype == torch.uint8:
                x.fill_(0xFF)
            elif x.dtype.is_floating_point:
                x.fill_(float("nan"))
        return x
    monkeypatch.setattr(torch, "empty", empty)
    for N, r in ((1000, 7), (70001, 32)):
        p = problem(N, r, seed=4)
        results = []
        for _ in range(2):
            monkeypatch.setattr(psgd, "_ws_cache", _lib.WorkspaceCache())
            t = on_device(p, torch.bfloat16)
            o1 = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"], out=torch.full_like(t["g"], float("nan")))
            psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=True, update_U=True,
                                          rounding="stochastic", rounding_seed=1)
            o2 = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32,
                                                               balance=False, update_U=False, rounding="nearest",
                                                               out=torch.full_like(t["g"], float("nan")))
            torch.cuda.synchronize()
            results.append((_bits(t), o1.clone(), o2.clone()))
        (sa, a1, a2), (sb, b1, b2) = results
        for k in ("U", "V", "d"):
            assert torch.equal(sa[k], sb[k]) and torch.isfinite(sa[k].view(torch.bfloat16).float()).all(), k
        assert torch.equal(a1, b1) and torch.equal(a2, b2)
        assert torch.isfinite(a1).all() and torch.isfinite(a2).all()


@pytest.mark.parametrize("nan_bits", (None, 0x7F800001, 0xFF80BEEF))
@pytest.mark.parametrize("fused", (0, 1))
@pytest.mark.parametrize("update_U", (1, 0))
def test_nan_in_h_propagates(psgd, update_U, fused, nan_bits):
    N, r = 5000, 10
    p = problem(N, r, seed=6)
    if nan_bits is None:
        p["h"][17, 0] = np.nan
    else:           # a NaN whose payload lies in the low 16 mantissa bits only (signalling): its top 16 bits alone are an Inf
        p["h"].view(np.uint32)[17, 0] = nan_bits
        assert np.isnan(p["h"][17, 0])
    t = on_device(p, torch.bfloat16)
    kw = dict(balance=False, update_U=bool(update_U), rounding="stochastic", rounding_seed=3)
    if fused:
        out = psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32, **kw)
    else:
        psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(t["d"].float()).all()
    assert torch.isnan(t["U" if update_U else "V"].float()).all()
    assert torch.isfinite(t["V" if update_U else "U"].float()).all()
    if fused:
        assert torch.isnan(out).all()


def test_functional_errors(psgd):
    p = problem(100, 4, seed=1)
    t = on_device(p, torch.bfloat16)
    f = on_device(p, torch.float32)
    with pytest.raises(TypeError, match="mixed"):
        psgd.precond_grad_UVd_math(t["U"], f["V"], t["d"], t["g"])
    with pytest.raises(TypeError, match="float16"):
        psgd.precond_grad_UVd_math(t["U"].half(), t["V"].half(), t["d"].half(), t["g"])
    with pytest.raises(TypeError, match="float32"):
        psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"].bfloat16(), t["h"], STEP, TINY32, balance=False, update_U=True)
    with pytest.raises(ValueError, match="matrix"):
        psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], torch.randn(100, 3, device=_dev()))
    with pytest.raises(ValueError, match="rounding"):
        psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, balance=False, update_U=True, rounding="up")
    with pytest.raises(ValueError, match="rounding"):       # validated for an fp32 state too, where nothing is rounded
        psgd.update_precond_UVd_math_(f["U"], f["V"], f["d"], f["v"], f["h"], STEP, TINY32, balance=False, update_U=True, rounding="up")
    with pytest.raises(ValueError, match="bfloat16 state only"):
        psgd.update_precond_UVd_math_(f["U"], f["V"], f["d"], f["v"], f["h"], STEP, TINY32, balance=False, update_U=True,
                                      rounding="stochastic")
    with pytest.raises(ValueError, match="bfloat16 state only"):
        psgd.update_precond_UVd_math_and_precond_grad(f["U"], f["V"], f["d"], f["v"], f["h"], f["g"], STEP, TINY32, balance=False,
                                                      update_U=True, rounding_seed=3)
    big = on_device(problem(50, 40, seed=1), torch.bfloat16)
    with pytest.raises(ValueError, match="32"):
        psgd.precond_grad_UVd_math(big["U"], big["V"], big["d"], big["g"])


# ------------------------------------------------------------------------------------------------ class
def _quadratic(psgd, state_route, seed=2, **kw):
    dev = _dev()
    torch.manual_seed(11)
    A = torch.randn(200, 200, device=dev) * 0.1
    H = (A @ A.t() + 0.3 * torch.eye(200, device=dev))
    torch.manual_seed(3)
    w = (torch.randn(200, 1, device=dev) * 0.5).to(torch.bfloat16).requires_grad_(True)
    opt = psgd.UVd([w], rank_of_modification=10, lr_params=0.05, lr_preconditioner=0.05, generator=torch.Generator().manual_seed(seed),
                   state_dtype="param", state_route=state_route, **kw)
    return w, opt, (lambda: 0.5 * (w.float().t() @ H @ w.float()).sum())


def test_class_native_route(psgd):
    runs = []
    for _ in range(2):
        w, opt, closure = _quadratic(psgd, "native")
        assert opt._U.dtype == torch.bfloat16 and opt._state_rounding == "stochastic"
        torch.manual_seed(5)
        l0 = float(opt.step(closure).detach())
        for _ in range(60):
            l = float(opt.step(closure).detach())
        assert all(x.dtype == torch.bfloat16 for x in (opt._U, opt._V, opt._d))
        assert all(torch.isfinite(x.float()).all() for x in (opt._U, opt._V, opt._d, w))
        assert l < 0.5 * l0, (l, l0)
        runs.append([x.detach().view(torch.int16).clone() for x in (opt._U, opt._V, opt._d, w)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    _, opt_n, _ = _quadratic(psgd, "native", state_rounding="nearest")
    assert opt_n._state_rounding == "nearest"


def test_class_step_seeds_give_distinct_streams(psgd, hip_lib, monkeypatch):
    """the seeds three consecutive steps hand to the kernels: the keys of d at step k, V at k + 1 and U at k + 2 all differ"""
    seen = []
    real = psgd.update_precond_UVd_math_and_precond_grad

    def spy(*a, **k):
        seen.append(k["rounding_seed"])
        return real(*a, **k)
    monkeypatch.setattr(psgd, "update_precond_UVd_math_and_precond_grad", spy)
    w, opt, closure = _quadratic(psgd, "native")
    for _ in range(5):
        opt.step(closure)
    assert len(seen) == 5 and len(set(seen)) == 5
    assert seen == [psgd.uvd_step_rounding_seed(opt._round_seed0, k) for k in range(5)]
    key = hip_lib.psgd_uvd_bf16_rounding_key
    keys = {(k, t): key(seen[k], t) for k in range(5) for t in range(3)}
    assert len(set(keys.values())) == 15
    for k in range(3):
        assert len({keys[(k, 2)], keys[(k + 1, 1)], keys[(k + 2, 0)]}) == 3


def test_class_constructor_errors(psgd):
    dev = _dev()
    w16 = torch.zeros(50, 1, device=dev, dtype=torch.float16, requires_grad=True)
    wb = torch.zeros(50, 1, device=dev, dtype=torch.bfloat16, requires_grad=True)
    w32 = torch.zeros(50, 1, device=dev, requires_grad=True)
    with pytest.raises(ValueError, match="bfloat16"):
        psgd.UVd([w16], state_dtype="param", state_route="native")
    with pytest.raises(ValueError, match="bfloat16"):
        psgd.UVd([w32], state_route="native")
    with pytest.raises(ValueError, match="32"):
        psgd.UVd([wb], rank_of_modification=40, state_dtype="param", state_route="native")
    with pytest.raises(ValueError, match="group"):
        psgd.UVd([wb], state_dtype="param", state_route="native", stage_backend="nccl")
    with pytest.raises(ValueError, match="group"):
        psgd.UVd([wb], state_dtype="param", state_route="native", group=object())
    with pytest.raises(ValueError, match="state_route"):
        psgd.UVd([wb], state_dtype="param", state_route="fast")
    with pytest.raises(ValueError, match="state_rounding"):
        psgd.UVd([wb], state_dtype="param", state_route="native", state_rounding="up")
    opt = psgd.UVd([w32], state_dtype=torch.bfloat16, state_route="native")     # fp32 parameters, bf16 state: allowed
    assert opt._U.dtype == torch.bfloat16


def test_step_memory(psgd):
    """the point of the feature: no fp32 copy of the state exists during a native step (N = 4M, r = 20)"""
    dev = _dev()
    N, r = 4 * 1024 * 1024, 20
    peaks = {}
    for route in ("native", "widen"):
        torch.manual_seed(1)
        w = (torch.randn(N, device=dev) * 0.1).to(torch.bfloat16).requires_grad_(True)
        c = torch.rand(N, device=dev) + 0.5
        opt = psgd.UVd([w], rank_of_modification=r, lr_params=0.01, lr_preconditioner=0.01, generator=torch.Generator().manual_seed(1),
                       state_dtype="param", state_route=route, placement=None)
        closure = lambda: 0.5 * (c * w.float() * w.float()).sum()      # noqa: E731
        opt.step(closure)                                               # warm-up: workspaces exist
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        opt.step(closure)
        torch.cuda.synchronize()
        peaks[route] = torch.cuda.max_memory_allocated() - before
        print("step memory %s: %.1f MB over the state (one fp32 factor: %.1f MB)" % (route, peaks[route] / 1e6, 4 * N * r / 1e6))
        del opt, w, c, closure
        torch.cuda.empty_cache()
    assert peaks["native"] < 4 * N * r, peaks
    assert peaks["widen"] > 4 * N * r, peaks
