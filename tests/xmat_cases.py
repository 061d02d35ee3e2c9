"""The X-shaped preconditioner's reference (include/psgd_xmat_hip.h restated in plain torch, run in float64) and test inputs:
a = exp(U(-1, 1)), |b_i| <= 0.3 min(a_i, a_j), b = 0 at the middle of an odd N, v, h, g ~ N(0, 1).  Bars: README, "Parity"."""
import numpy as np
import torch

TINY32 = float(np.finfo(np.float32).tiny)
STEP = 0.1
STATE_BAR, INCREMENT_BAR, APPLY_BAR = 1e-5, 2e-3, 1e-5
T, GRID = 2048, 2048                 # elements one workgroup owns per trip; workgroups of the reading sweep
_flip = lambda x: torch.flip(x, [0])


def xmat_apply_ref(a, b, g):
    w = a * g + b * _flip(g)
    return a * w + _flip(b) * _flip(w)


def xmat_update_ref(a, b, v, h, step=STEP, tiny=TINY32, diagonal=False):
    A = a * h + b * _flip(h)
    B = (_flip(a) * v - _flip(b) * _flip(v)) / (a * _flip(a) - b * _flip(b))
    nA, nB = A * A - B * B, A * _flip(A) - B * _flip(B)
    if diagonal:
        nB = torch.zeros_like(nB)
    elif a.numel() % 2:
        nB[a.numel() // 2] = 0.0
    mu = step / (torch.maximum(nA.abs().max(), nB.abs().max()) + tiny)
    return a - mu * (nA * a + nB * _flip(b)), b - mu * (nA * b + nB * _flip(a))


_cache = {}


def problem(N, diagonal=False):
    """float32 a, b, v, h, g and float64 new_a, new_b, out (apply on the old state), out_new; made once, never modified"""
    if (N, diagonal) not in _cache:
        gen = torch.Generator().manual_seed(1000 + N)
        a = torch.exp(torch.rand(N, generator=gen) * 2 - 1)
        b = 0.3 * torch.minimum(a, _flip(a)) * (torch.rand(N, generator=gen) * 2 - 1)
        if N % 2:
            b[N // 2] = 0.0
        if diagonal:
            b = torch.zeros(N)
        p = dict(a=a, b=b, **{k: torch.randn(N, generator=gen) for k in "vhg"})
        d = {k: t.double() for k, t in p.items()}
        p["new_a"], p["new_b"] = xmat_update_ref(d["a"], d["b"], d["v"], d["h"], diagonal=diagonal)
        p["out"], p["out_new"] = xmat_apply_ref(d["a"], d["b"], d["g"]), xmat_apply_ref(p["new_a"], p["new_b"], d["g"])
        _cache[(N, diagonal)] = p
    return _cache[(N, diagonal)]


def err(x, ref):
    d, n = float((x.detach().double().cpu() - ref).norm()), float(ref.norm())
    return d / n if n else d
