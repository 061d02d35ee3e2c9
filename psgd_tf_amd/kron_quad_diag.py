"""The QUAD Kronecker update with ONE DIAGONAL side, on psgd_kron_qdiag.hip: embedding-scale layers.

include/psgd_kron_quad_diag_hip.h states the definition in full.  One factor is the project's scale factor, a [1, D] tensor that
stands for diag(q); the other is a symmetric dense factor.  update_precond_kron_quad_ and precond_grad_kron_quad of kron_quad.py
tell the format by the factor shapes and come here when exactly one factor has the scale shape [1, n], n >= 2, and the other is
square:

    update(Ql, Qr, L, G, step, decay)      the update, in place on the vector, the dense factor and L
    apply(Ql, Qr, G, out=None)             out = diag(ql o ql) ((G Qr) Qr), or (Ql (Ql G)) diag(qr o qr)
    slices(M, N, diag_side)                S of the split-K Gram: a function of the shape alone

The four C entry points are bound here, in a signature table of this module's own.  fp32 on the HIP device only; no fallback.
class Kron(preconditioner_update="quad", quad_diagonal=True) runs its (dense, scale) and (scale, dense) matrix layers through
the two calls.
"""
import ctypes

import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd

_p, _i64, _int, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
SIGNATURES = {
    "psgd_kron_qdiag_workspace_bytes": (_i64, [_int, _int, _int]),
    "psgd_kron_qdiag_slices": (_int, [_int, _int, _int]),
    "psgd_kron_qdiag_apply_f32": (_int, [_p, _p, _p, _p, _int, _int, _int, _p, _i64, _p]),
    "psgd_kron_qdiag_update_f32": (_int, [_p, _p, _p, _p, _int, _int, _int, _flt, _flt, _p, _i64, _p]),
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


def _is_scale(t):
    return isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] == 1 and t.shape[1] >= 2


def diag_side(name, Ql, Qr):
    """None when neither factor has the scale shape [1, n], n >= 2 (the dense path judges the operands); 0 when Ql has it, 1 when
    Qr has; both is a ValueError"""
    left, right = _is_scale(Ql), _is_scale(Qr)
    if left and right:
        raise ValueError("%s: Ql %s and Qr %s are both scale factors; a diagonal factor always faces a dense one"
                         % (name, tuple(Ql.shape), tuple(Qr.shape)))
    return 0 if left else 1 if right else None


def _operands(name, side, Ql, Qr, G, **more):
    """the scale factor [1, D], the dense one [n, n] and G [M, N] float32 and contiguous on one HIP device, like every further named
    operand (its value a (tensor, shape) pair).  Returns (device, M, N)."""
    named = dict(Ql=Ql, Qr=Qr, G=G, **{k: v[0] for k, v in more.items()})
    for k, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch tensor, got %r" % (name, k, type(t)))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, got %s" % (name, k, t.dtype))
    if G.dim() != 2 or G.shape[0] < 1 or G.shape[1] < 1:
        raise ValueError("%s: G must be a matrix [M, N] with M, N >= 1, got %s" % (name, tuple(G.shape)))
    M, N = (int(s) for s in G.shape)
    want = dict(Ql=(1, M) if side == 0 else (M, M), Qr=(1, N) if side == 1 else (N, N))
    for k, (t, shape) in dict(Ql=(Ql, want["Ql"]), Qr=(Qr, want["Qr"]), **more).items():
        if tuple(t.shape) != shape:
            raise ValueError("%s: %s must have shape %s for G of shape %s, got %s" % (name, k, shape, (M, N), tuple(t.shape)))
    for k, t in named.items():
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (name, k))
    return _psgd._require_hip(name, *named.values()), M, N


def _workspace(device, M, N, side):
    load()
    return _psgd._workspace(("kron_qdiag",), device, "psgd_kron_qdiag_workspace_bytes", M, N, side)


def slices(M, N, diag_side):
    """S of the split-K Gram of an M x N layer whose left (0) or right (1) factor is diagonal"""
    S = int(load().psgd_kron_qdiag_slices(int(M), int(N), int(diag_side)))
    if S < 1:
        _lib.check(S, "psgd_kron_qdiag_slices")
    return S


def apply(side, Ql, Qr, G, out=None):
    """precond_grad_kron_quad with the factor on `side` diagonal: two launches"""
    more = {} if out is None else {"out": (out, tuple(G.shape) if isinstance(G, torch.Tensor) else ())}
    dev, M, N = _operands("precond_grad_kron_quad", side, Ql, Qr, G, **more)
    if out is None:
        out = torch.empty_like(G)
    ws = _workspace(dev, M, N, side)
    rc = load().psgd_kron_qdiag_apply_f32(Ql.data_ptr(), Qr.data_ptr(), G.data_ptr(), out.data_ptr(), M, N, side, ws.data_ptr(),
                                          ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_qdiag_apply_f32")
    return out


def update(side, Ql, Qr, L, G, step, decay):
    """update_precond_kron_quad_ with the factor on `side` diagonal: six launches, the host reads nothing"""
    dev, M, N = _operands("update_precond_kron_quad_", side, Ql, Qr, G, L=(L, (2,)))
    ws = _workspace(dev, M, N, side)
    rc = load().psgd_kron_qdiag_update_f32(Ql.data_ptr(), Qr.data_ptr(), L.data_ptr(), G.data_ptr(), M, N, side, float(step),
                                           float(decay), ws.data_ptr(), ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_qdiag_update_f32")
