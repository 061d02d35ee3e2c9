"""Seeded synthetic UVd problems shared by the CPU and GPU tests (SURVEY 8d inputs)."""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)


def make_uvd_problem(N, r, seed=0, uv_gain=1.0, d_spread=0.0):
    """U, V ~ N(0,1) * uv_gain * (N r)^-1/2 (psgd.py:687-689), d = exp(d_spread * N(0,1))
    (d = 1 at d_spread = 0, psgd.py:690), g, v ~ N(0,1) (psgd.py:713), h = c .* v with
    c ~ LogUniform[1e-2, 1e2] (a diagonal SPD Hessian).  All fp32 arrays; d,g,v,h are [N,1]."""
    rng = np.random.default_rng(seed)
    scale = uv_gain * (1.0 / (N * r)) ** 0.5
    U = (rng.standard_normal((N, r)) * scale).astype(np.float32)
    V = (rng.standard_normal((N, r)) * scale).astype(np.float32)
    d = np.exp(d_spread * rng.standard_normal((N, 1))).astype(np.float32)
    g = rng.standard_normal((N, 1)).astype(np.float32)
    v = rng.standard_normal((N, 1)).astype(np.float32)
    c = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=(N, 1)))
    h = (c * v).astype(np.float32)
    return dict(U=U, V=V, d=d, g=g, v=v, h=h)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


def bf16_grid(y):
    """(floor, ceil, round-to-nearest-even, spacing) of fp64 values on the bf16 grid (normal range)"""
    y = np.asarray(y, dtype=np.float64)
    _, ex = np.frexp(np.where(y == 0, 1.0, y))
    s = np.ldexp(1.0, ex - 1 - 7)
    q = y / s
    return np.floor(q) * s, np.ceil(q) * s, np.round(q) * s, s


def to_bf16_np(x):
    """fp32 array -> the fp32 array of its bf16 roundings (round to nearest even)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy()


def check_bf16_state(tag, stored, y64, widen32, written, rounding):
    """A bf16-stored UVd state against the fp64 oracle's y64 (dicts of arrays under "U", "V", "d"; stored: the codes widened to
    fp64; widen32: the fp32 kernels' result on the widened inputs; written: the tensors the call rewrote).  Asserts the element
    bound |stored - y64| <= 2^-7 |y64| + 1e-5 rms(y64) on every tensor; returns the pooled shares (p_native, p_widen) over the
    written tensors of codes that differ from RNE_bf16(y64) (stochastic: that are neither floor nor ceil of y64) and the largest
    err / bound met."""
    bad_n = bad_w = total = 0
    worst = 0.0
    for k in ("U", "V", "d"):
        s, y = stored[k], y64[k]
        rms = float(np.sqrt(np.mean(y * y)))
        err = np.abs(s - y)
        bound = 2.0 ** -7 * np.abs(y) + 1e-5 * rms
        assert np.all(err <= bound), (tag, k, float(np.max(err - bound)))
        if err.size:
            worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
        if k not in written:
            continue
        lo, hi, rne, _ = bf16_grid(y)
        if rounding == "nearest":
            bad_n += int(np.sum(s != rne))
        else:
            bad_n += int(np.sum((s != lo) & (s != hi)))
        bad_w += int(np.sum(to_bf16_np(widen32[k]).astype(np.float64) != rne))
        total += y.size
    return bad_n / total, bad_w / total, worst
