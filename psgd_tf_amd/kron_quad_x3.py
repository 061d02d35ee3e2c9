"""The QUAD Kronecker update with its products on the bf16 matrix cores at fp32 grade ("bf16 x 3"), on psgd_kron_quad_x3.hip.

include/psgd_kron_quad_x3_hip.h states what differs from the fp32 route: every fp32 operand element is split exactly into three
bf16 terms on the way into LDS and a product is six v_mfma_f32_16x16x32_bf16 terms accumulated in fp32; the definition, the state
and the workspace are those of kron_quad.py, so a run may switch routes at any step.  update_precond_kron_quad_ and
precond_grad_kron_quad of kron_quad.py come here with products="bf16x3" and (dense, dense) factors:

    update(Ql, Qr, L, G, step, decay)      the update, in place on Ql, Qr and L: six launches
    apply(Ql, Qr, G, out=None)             out = Ql (Ql G Qr) Qr: four launches

The three C entry points are bound here, in a signature table of this module's own.  fp32 on the HIP device only; no fallback.
class Kron(preconditioner_update="quad", quad_products="bf16x3") runs its large (dense, dense) quad layers through the two calls
(opt.quad_x3_layers); profiles/kron_quad_x3_timing.txt has both routes side by side.
"""
import ctypes

import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd

PRODUCTS = ("fp32", "bf16x3")
# class Kron's default of quad_products_min_dim: the smallest square size of profiles/kron_quad_x3_timing.txt at which update +
# apply on this route beat the fp32 route outside the spread
QUAD_X3_MIN_DIM = 2048

_p, _i64, _int, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
SIGNATURES = {
    "psgd_kron_quad_x3_workspace_bytes": (_i64, [_int, _int]),
    "psgd_kron_quad_x3_apply_f32": (_int, [_p, _p, _p, _p, _int, _int, _p, _i64, _p]),
    "psgd_kron_quad_x3_update_f32": (_int, [_p, _p, _p, _p, _int, _int, _flt, _flt, _p, _i64, _p]),
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


def check_products(name, products, diag_side=None):
    """products is "fp32" or "bf16x3"; "bf16x3" with a scale factor (diag_side 0 or 1) is refused: that route stays fp32"""
    if products not in PRODUCTS:
        raise ValueError("%s: products must be 'fp32' or 'bf16x3', got %r" % (name, products))
    if products == "bf16x3" and diag_side is not None:
        raise ValueError("%s: products='bf16x3' runs (dense, dense) factors; %s is a scale factor, whose route stays 'fp32'"
                         % (name, ("Ql", "Qr")[diag_side]))


def _workspace(device, M, N):
    load()
    return _psgd._workspace(("kron_quad_x3",), device, "psgd_kron_quad_x3_workspace_bytes", M, N)


def apply(operands, Ql, Qr, G, out=None):
    """precond_grad_kron_quad on the bf16 x 3 core; operands: kron_quad._operands, which judges the tensors"""
    more = {} if out is None else {"out": (out, tuple(G.shape) if isinstance(G, torch.Tensor) else ())}
    dev, M, N = operands("precond_grad_kron_quad", Ql, Qr, G, **more)
    if out is None:
        out = torch.empty_like(G)
    ws = _workspace(dev, M, N)
    rc = load().psgd_kron_quad_x3_apply_f32(Ql.data_ptr(), Qr.data_ptr(), G.data_ptr(), out.data_ptr(), M, N, ws.data_ptr(),
                                            ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_quad_x3_apply_f32")
    return out


def update(operands, Ql, Qr, L, G, step, decay):
    """update_precond_kron_quad_ on the bf16 x 3 core: six launches, the host reads nothing"""
    dev, M, N = operands("update_precond_kron_quad_", Ql, Qr, G, L=(L, (2,)))
    ws = _workspace(dev, M, N)
    rc = load().psgd_kron_quad_x3_update_f32(Ql.data_ptr(), Qr.data_ptr(), L.data_ptr(), G.data_ptr(), M, N, float(step),
                                             float(decay), ws.data_ptr(), ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_kron_quad_x3_update_f32")
