"""The QUAD Kronecker update on ORDER-3 tensors with three symmetric factors, on psgd_kron_qnd.hip.

include/psgd_kron_quad_nd_hip.h states the definition in full: G is a tensor [A, B, C], Qs = [Qa, Qb, Qc] are symmetric factors
of the three modes with P = (Qa Qa) (x) (Qb Qb) (x) (Qc Qc), L = [La, Lb, Lc] the running Lipschitz estimates.  A conv kernel
[Cout, Cin, kh, kw] is the tensor [Cout, Cin, kh kw]: one factor for the output channels, one for the input channels, one for the
filter taps, where the folded matrix [Cout, Cin kh kw] has one (Cin kh kw)^2 factor for the last two together.

    kron_quad_nd_initial_state(shape3, scale, device)          ([Qa, Qb, Qc], L) = ([scale I, I, I], zeros(3))
    update_precond_kron_quad_nd_(Qs, L, G, step, decay)        the update, in place on the factors and L: seven launches
    precond_grad_kron_quad_nd(Qs, G, out=None)                 out = G x1 Qa^2 x2 Qb^2 x3 Qc^2: six launches

With A = 1 and Qa = [[1]] the update is update_precond_kron_quad_ on the matrix [B, C], bit for bit.  The three C entry points are
bound here, in a signature table of this module's own.  fp32 on the HIP device only; no fallback.
class Kron(preconditioner_update="quad", any_rank=True, quad_tensor=True) runs its parameters of rank >= 3 through these two
functions, on the view [s0, s1, prod(s2:)].
"""
import ctypes

import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd

_p, _i64, _int, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
SIGNATURES = {
    "psgd_kron_qnd_workspace_bytes": (_i64, [_int, _int, _int]),
    "psgd_kron_qnd_apply_f32": (_int, [_p, _p, _p, _p, _p, _int, _int, _int, _p, _i64, _p]),
    "psgd_kron_qnd_update_f32": (_int, [_p, _p, _p, _p, _p, _int, _int, _int, _flt, _flt, _p, _i64, _p]),
}
MAX_NUMEL = 2 ** 31 - 1      # the kernels index a tensor's elements with an int
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


def _shape3(name, shape):
    try:
        shape = tuple(int(s) for s in shape)
    except TypeError:
        raise ValueError("%s: a shape [A, B, C] is wanted, got %r" % (name, shape))
    if len(shape) != 3 or min(shape) < 1 or shape[0] * shape[1] * shape[2] > MAX_NUMEL:
        raise ValueError("%s: a shape [A, B, C] with A, B, C >= 1 and A B C < 2^31 is wanted, got %r" % (name, shape))
    return shape


def _operands(name, Qs, G, **more):
    """Qs three tensors [A, A], [B, B], [C, C] and G [A, B, C], float32 and contiguous on one HIP device, like every further named
    operand (its value a (tensor, shape) pair).  Returns (device, (A, B, C))."""
    if not isinstance(Qs, (list, tuple)) or len(Qs) != 3:
        raise ValueError("%s: Qs must be a list of three factors [Qa, Qb, Qc], got %r" % (name, type(Qs) if not isinstance(Qs, (list, tuple))
                                                                                        else len(Qs)))
    named = dict(Qa=Qs[0], Qb=Qs[1], Qc=Qs[2], G=G, **{k: v[0] for k, v in more.items()})
    for k, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch tensor, got %r" % (name, k, type(t)))
        if t.dtype != torch.float32:
            raise TypeError("%s: %s must be float32, got %s" % (name, k, t.dtype))
    if G.dim() != 3:
        raise ValueError("%s: G must be a tensor [A, B, C], got %s" % (name, tuple(G.shape)))
    shape = _shape3(name, G.shape)
    want = dict(Qa=(shape[0],) * 2, Qb=(shape[1],) * 2, Qc=(shape[2],) * 2, **{k: v[1] for k, v in more.items()})
    for k, t in named.items():
        if k != "G" and tuple(t.shape) != tuple(want[k]):
            raise ValueError("%s: %s must have shape %s for G of shape %s, got %s" % (name, k, tuple(want[k]), shape, tuple(t.shape)))
    for k, t in named.items():
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (name, k))
    return _psgd._require_hip(name, *named.values()), shape


def _workspace(device, shape):
    load()
    return _psgd._workspace(("kron_qnd",), device, "psgd_kron_qnd_workspace_bytes", *shape)


def kron_quad_nd_initial_state(shape3, scale=1.0, device=None):
    """([Qa, Qb, Qc], L), float32: identities, the first one times scale; L = zeros(3)"""
    shape = _shape3("kron_quad_nd_initial_state", shape3)
    Qs = [torch.eye(n, dtype=torch.float32, device=device) for n in shape]
    Qs[0] = Qs[0] * float(scale)
    return Qs, torch.zeros(3, dtype=torch.float32, device=device)


def precond_grad_kron_quad_nd(Qs, G, out=None):
    """out = G x1 Qa^2 x2 Qb^2 x3 Qc^2: six mode products, the modes in ascending extent (ties: the lower mode first), each factor
    applied twice back to back.  out (made when None) must not be G or a factor."""
    G = _psgd._c(G)
    more = {} if out is None else {"out": (out, tuple(G.shape) if isinstance(G, torch.Tensor) else ())}
    dev, (A, B, C) = _operands("precond_grad_kron_quad_nd", Qs, G, **more)
    if out is None:
        out = torch.empty_like(G)
    ws = _workspace(dev, (A, B, C))
    rc = load().psgd_kron_qnd_apply_f32(Qs[0].data_ptr(), Qs[1].data_ptr(), Qs[2].data_ptr(), G.data_ptr(), out.data_ptr(), A, B, C,
                                        ws.data_ptr(), ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_qnd_apply_f32")
    return out


def update_precond_kron_quad_nd_(Qs, L, G, step, decay=0.95):
    """Qa, Qb, Qc, L <- the QUAD step on the gradient tensor G, in place, seven launches; the host reads nothing.  Returns None."""
    G = _psgd._c(G)
    dev, (A, B, C) = _operands("update_precond_kron_quad_nd_", Qs, G, L=(L, (3,)))
    ws = _workspace(dev, (A, B, C))
    rc = load().psgd_kron_qnd_update_f32(Qs[0].data_ptr(), Qs[1].data_ptr(), Qs[2].data_ptr(), L.data_ptr(), G.data_ptr(), A, B, C,
                                         float(step), float(decay), ws.data_ptr(), ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_qnd_update_f32")
