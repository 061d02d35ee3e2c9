"""The inverse-free Kronecker whitening update (QUAD) on full symmetric factors, on psgd_kron_quad.hip.

The reference has no code for this update; the PyTorch line of PSGD, which its README names as the place for updates, uses it in
its Kron whitening optimizer.  include/psgd_kron_quad_hip.h states the definition in full: symmetric positive-definite factors
Ql (M x M), Qr (N x N) with P = (Ql Ql) (x) (Qr Qr), no solve, no inverse, no probe, and a step bounded by the running
Lipschitz estimates L = [Ll, Lr].

    kron_quad_initial_state(M, N, scale, device)               (Ql, Qr, L) = (scale I, I, zeros(2))
    update_precond_kron_quad_(Ql, Qr, L, G, step, decay)       the update, in place on Ql, Qr and L
    precond_grad_kron_quad(Ql, Qr, G, out=None)                out = Ql (Ql G Qr) Qr

The three C entry points are bound here, in a signature table of this module's own, on the library _lib.load() returns.  fp32 on
the HIP device only; no fallback.  class Kron(preconditioner_fit="whitening", preconditioner_update="quad") runs its
(dense, dense) matrix layers through these two functions.

One factor may be diagonal instead: a scale factor of shape [1, n], n >= 2, facing a square one sends both functions to
kron_quad_diag.py (psgd_kron_qdiag.hip, include/psgd_kron_quad_diag_hip.h); kron_quad_initial_state(formats=("scale", "dense"))
makes such a state.  Two scale factors are a ValueError.

products="fp32" (the default: not a launch or a bit moves) or "bf16x3" on both functions: "bf16x3" sends (dense, dense) factors
to kron_quad_x3.py (psgd_kron_quad_x3.hip, include/psgd_kron_quad_x3_hip.h): the same update with every product on the bf16 matrix
cores at fp32 grade.  Any other value, and "bf16x3" with a scale factor, is a ValueError.
"""
import ctypes

import torch

from . import _lib
from . import kron_quad_diag as _diag
from . import kron_quad_x3 as _x3
from . import preconditioned_stochastic_gradient_descent as _psgd

KRON_QUAD_TILE = 64          # PSGD_KRON_QUAD_TILE: edge of the output tile one workgroup owns

_p, _i64, _int, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
SIGNATURES = {
    "psgd_kron_quad_workspace_bytes": (_i64, [_int, _int]),
    "psgd_kron_quad_apply_f32": (_int, [_p, _p, _p, _p, _int, _int, _p, _i64, _p]),
    "psgd_kron_quad_update_f32": (_int, [_p, _p, _p, _p, _int, _int, _flt, _flt, _p, _i64, _p]),
}
_bound = None


def load():
    """_lib.load() with this module's entry points bound (once per loaded library)"""
    global _bound
    lib = _lib.load()
    if _bound is not lib:
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _bound = lib
    return lib


def _operands(name, Ql, Qr, G, **more):
    """Ql [M, M], Qr [N, N] and G [M, N] float32 and contiguous on one HIP device, like every further named operand (its value a
    (tensor, shape) pair).  Returns (device, M, N)."""
    named = dict(Ql=Ql, Qr=Qr, G=G, **{k: v[0] for k, v in more.items()})
    for k, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch tensor, got %r" % (name, k, type(t)))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, got %s" % (name, k, t.dtype))
    if G.dim() != 2 or G.shape[0] < 1 or G.shape[1] < 1:
        raise ValueError("%s: G must be a matrix [M, N] with M, N >= 1, got %s" % (name, tuple(G.shape)))
    M, N = (int(s) for s in G.shape)
    for k, (t, want) in dict(Ql=(Ql, (M, M)), Qr=(Qr, (N, N)), **more).items():
        if tuple(t.shape) != want:
            raise ValueError("%s: %s must have shape %s for G of shape %s, got %s" % (name, k, want, (M, N), tuple(t.shape)))
    for k, t in named.items():
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (name, k))
    return _psgd._require_hip(name, *named.values()), M, N


def _workspace(device, M, N):
    load()
    return _psgd._workspace(("kron_quad",), device, "psgd_kron_quad_workspace_bytes", M, N)


def kron_quad_initial_state(M, N, scale=1.0, device=None, formats=("dense", "dense")):
    """(Ql, Qr, L), float32: a "dense" side starts at I, a "scale" side at ones(1, n); the left factor is multiplied by scale;
    L = zeros(2).  formats: ("dense", "dense"), ("scale", "dense") or ("dense", "scale")."""
    M, N = int(M), int(N)
    if M < 1 or N < 1:
        raise ValueError("kron_quad_initial_state: M and N must be >= 1, got %d and %d" % (M, N))
    formats = tuple(formats)
    if formats not in (("dense", "dense"), ("scale", "dense"), ("dense", "scale")):
        raise ValueError("kron_quad_initial_state: formats must be ('dense', 'dense'), ('scale', 'dense') or ('dense', 'scale'), got %r"
                         % (formats,))
    if "scale" in formats and (M, N)[formats.index("scale")] < 2:
        raise ValueError("kron_quad_initial_state: a scale side has length >= 2 (a [1, 1] factor is a dense one), got %s" % ((M, N),))
    make = lambda side, n: (torch.eye(n, dtype=torch.float32, device=device) if side == "dense"
                            else torch.ones(1, n, dtype=torch.float32, device=device))
    return make(formats[0], M) * float(scale), make(formats[1], N), torch.zeros(2, dtype=torch.float32, device=device)


def precond_grad_kron_quad(Ql, Qr, G, out=None, products="fp32"):
    """out = Ql (Ql G Qr) Qr, four chained products.  out (made when None) must not be G, Ql or Qr.  With one scale factor
    [1, n]: out = diag(ql o ql) ((G Qr) Qr) or its mirror, two launches (kron_quad_diag.py).  products="bf16x3": the four
    products on the bf16 matrix cores at fp32 grade (kron_quad_x3.py), dense factors only."""
    G = _psgd._c(G)
    side = _diag.diag_side("precond_grad_kron_quad", Ql, Qr)
    _x3.check_products("precond_grad_kron_quad", products, side)
    if side is not None:
        return _diag.apply(side, Ql, Qr, G, out)
    if products == "bf16x3":
        return _x3.apply(_operands, Ql, Qr, G, out)
    more = {} if out is None else {"out": (out, tuple(G.shape) if isinstance(G, torch.Tensor) else ())}
    dev, M, N = _operands("precond_grad_kron_quad", Ql, Qr, G, **more)
    if out is None:
        out = torch.empty_like(G)
    ws = _workspace(dev, M, N)
    rc = load().psgd_kron_quad_apply_f32(Ql.data_ptr(), Qr.data_ptr(), G.data_ptr(), out.data_ptr(), M, N, ws.data_ptr(), ws.numel(),
                                         _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_quad_apply_f32")
    return out


def update_precond_kron_quad_(Ql, Qr, L, G, step, decay=0.95, products="fp32"):
    """Ql, Qr, L <- the QUAD step on the gradient G, in place, six launches; the host reads nothing.  Returns None.  With one
    scale factor [1, n] that side takes the diagonal rule (kron_quad_diag.py).  products="bf16x3": every product on the bf16
    matrix cores at fp32 grade (kron_quad_x3.py), dense factors only."""
    G = _psgd._c(G)
    side = _diag.diag_side("update_precond_kron_quad_", Ql, Qr)
    _x3.check_products("update_precond_kron_quad_", products, side)
    if side is not None:
        return _diag.update(side, Ql, Qr, L, G, step, decay)
    if products == "bf16x3":
        return _x3.update(_operands, Ql, Qr, L, G, step, decay)
    dev, M, N = _operands("update_precond_kron_quad_", Ql, Qr, G, L=(L, (2,)))
    ws = _workspace(dev, M, N)
    rc = load().psgd_kron_quad_update_f32(Ql.data_ptr(), Qr.data_ptr(), L.data_ptr(), G.data_ptr(), M, N, float(step), float(decay),
                                          ws.data_ptr(), ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_quad_update_f32")
