"""The matrix-free preconditioners: X-shaped, Q = diag(a) + adiag(b), and diagonal (b absent), on psgd_xmat.hip.

The reference has no code for this family; its README names it and points to the PyTorch implementation.  The definition here
is the Lie-group update of psgd.py:554-617 specialised to the X-matrix group (include/psgd_xmat_hip.h states it in full): with
j = N-1-i every pair (i, j) is an independent 2 x 2 block, the state is 2 N floats (N for the diagonal form), and a fused
update -> apply moves about 48 bytes per parameter.

    xmat_initial_state(N, scale, device)                         a = scale, b = 0
    update_precond_Xmat_math_(a, b, v, h, step, tiny)            the update, in place
    precond_grad_Xmat_math(a, b, g, out=None)                    P g = Q'Q g
    update_precond_grad_Xmat_math_(a, b, v, h, g, step, tiny)    both in one pass: the bits of the two calls above
    XMat(...).step(closure)                                      the optimizer, a subclass of _FlatStep

b=None everywhere selects the diagonal preconditioner.  The four C entry points are declared in include/psgd_xmat_hip.h and bound
here, in a signature table of this module's own, on the library _lib.load() returns.  fp32 on the HIP device only; no fallback.
"""
import ctypes

import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd

XMAT_TILE_ELEMS = 2048       # PSGD_XMAT_TILE_ELEMS: elements one workgroup owns per trip
XMAT_MAX_GRID = 2048         # PSGD_XMAT_MAX_GRID: workgroups of the reading sweep

_p, _i64, _int, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
SIGNATURES = {
    "psgd_xmat_workspace_bytes": (_i64, [_i64]),
    "psgd_xmat_apply_f32": (_int, [_p, _p, _p, _p, _i64, _p]),
    "psgd_xmat_update_f32": (_int, [_p, _p, _p, _p, _i64, _flt, _flt, _p, _i64, _p]),
    "psgd_xmat_update_apply_f32": (_int, [_p, _p, _p, _p, _p, _p, _i64, _flt, _flt, _p, _i64, _p]),
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


def _workspace(device, N):
    load()
    return _psgd._workspace(("xmat",), device, "psgd_xmat_workspace_bytes", N)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _operands(name, a, b, *vectors):
    """a and b (None: diagonal) are float32 vectors of one length N on the HIP device, every further operand a float32 tensor of N
    elements there ([N] or [N, 1]: a matrix g is refused).  Returns (device, N)."""
    dev = _psgd._require_hip(name, *[t for t in (a, b) + vectors if t is not None])
    N = a.numel()
    if a.dim() != 1 or N < 1 or (b is not None and b.shape != a.shape):
        raise ValueError("%s: a and b must be vectors of one length N >= 1, got %s and %s"
                         % (name, tuple(a.shape), None if b is None else tuple(b.shape)))
    for t in vectors:
        if t.numel() != N or t.dim() > 2:
            raise ValueError("%s: every operand must hold N = %d elements ([N] or [N, 1]; the preconditioner takes one flat vector, "
                             "not a matrix), got %s" % (name, N, tuple(t.shape)))
    return dev, N


def xmat_initial_state(N, scale, device=None):
    """(a, b) = (scale, 0): Q = scale I, two float32 vectors of length N"""
    N = int(N)
    if N < 1:
        raise ValueError("xmat_initial_state: N must be >= 1, got %d" % N)
    return (torch.full((N,), float(scale), dtype=torch.float32, device=device), torch.zeros(N, dtype=torch.float32, device=device))


def precond_grad_Xmat_math(a, b, g, out=None):
    """out = Q'Q g, one launch, 16 bytes per parameter.  out (made when None) must not be g, a or b."""
    g = _psgd._c(g)
    dev, N = _operands("precond_grad_Xmat_math", a, b, g, *(() if out is None else (out,)))
    if out is None:
        out = torch.empty_like(g)
    rc = load().psgd_xmat_apply_f32(a.data_ptr(), _ptr(b), g.data_ptr(), out.data_ptr(), N, _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_xmat_apply_f32")
    return out


def update_precond_Xmat_math_(a, b, v, h, step, tiny):
    """a, b <- the Lie-group step on the pair (v, h), in place, two launches, 40 bytes per parameter"""
    v, h = _psgd._c(v), _psgd._c(h)
    dev, N = _operands("update_precond_Xmat_math_", a, b, v, h)
    ws = _workspace(dev, N)
    rc = load().psgd_xmat_update_f32(a.data_ptr(), _ptr(b), v.data_ptr(), h.data_ptr(), N, float(step), float(tiny),
                                     ws.data_ptr(), ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_xmat_update_f32")


def update_precond_grad_Xmat_math_(a, b, v, h, g, step, tiny, out=None):
    """update_precond_Xmat_math_ then precond_grad_Xmat_math with the new state, in the update's two launches: the second one reads
    g and writes out from the a, b it has just formed.  The same bits as the two calls."""
    v, h, g = _psgd._c(v), _psgd._c(h), _psgd._c(g)
    dev, N = _operands("update_precond_grad_Xmat_math_", a, b, v, h, g, *(() if out is None else (out,)))
    if out is None:
        out = torch.empty_like(g)
    ws = _workspace(dev, N)
    rc = load().psgd_xmat_update_apply_f32(a.data_ptr(), _ptr(b), v.data_ptr(), h.data_ptr(), g.data_ptr(), out.data_ptr(), N,
                                           float(step), float(tiny), ws.data_ptr(), ws.numel(), _psgd._stream_ptr(dev))
    _lib.check(rc, "psgd_xmat_update_apply_f32")
    return out


class XMat(_psgd._FlatStep):
    """The X-shaped preconditioner as an optimizer: _FlatStep (step(), every switch of the shared step layer, the checkpoint
    skeleton) with the state a, b -- two float32 vectors of length N, N the number of elements of the parameters with
    requires_grad.  The preconditioner to take when the 2 r N + N floats of class UVd do not fit.

    The arguments are class UVd's, same names, order and defaults, without those of its rank, narrow state, placement and process
    group: a user swaps the class name.  step(closure) is _FlatStep.step: an updating step calls the fused update -> apply once
    (update_precond_grad_Xmat_math_ fed (v, h) with step lr_preconditioner and the float32 tiny of the functions), any other step
    the apply, into a flat output this object owns.  The state is updated in place; a step the guard skips touches nothing.

    diagonal=True (keyword-only) keeps b = 0: the diagonal (equilibration) preconditioner, state N floats, the same kernels.
    opt.b is then None.

    state_dict() / load_state_dict() carry "preconditioner": "xmat", "a" and "b" (float32 [N]; "b" is absent when diagonal) and
    what _FlatStep saves ("rank" is 0); a resumed run is bit-identical to the uninterrupted one.

    Out of scope, refused before a device is touched: a narrow state (state_dtype=), group=, placement=."""

    def __init__(self, params_with_grad, preconditioner_init_scale=1.0, lr_params=0.01, lr_preconditioner=0.01,
                 grad_clip_max_norm=None, preconditioner_update_probability=1.0,
                 exact_hessian_vector_product: bool = True, generator=None, step_tail="torch",
                 momentum=0.0, weight_decay=0.0, nonfinite="propagate", loss_scale=None, loss_scale_growth_interval=2000,
                 *, param_rounding="nearest", param_rounding_seed=None, preconditioner_fit="hessian", probe_seed=None,
                 param_groups=None, mixed_dtypes=False, diagonal=False, state_dtype=None, group=None, placement=None):
        N = self._init_params(params_with_grad, generator, param_rounding, preconditioner_fit, mixed_dtypes)
        if state_dtype not in (None, torch.float32):
            raise TypeError("XMat: the state is float32 (2 N floats; a narrow state is not supported), got state_dtype=%r" % (state_dtype,))
        if group is not None:
            raise ValueError("XMat: group= (a row-sharded state) is not supported: a pair spans both ends of the flat vector")
        if placement is not None:
            raise ValueError("XMat: placement= is not supported (the state is two plain vectors)")
        if not isinstance(diagonal, bool):
            raise ValueError("XMat: diagonal must be a bool, got %r" % (diagonal,))
        self._rank, self._store_dtype, self._state_rounding, self._diagonal = 0, torch.float32, None, diagonal
        self._init_hypers(lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                          exact_hessian_vector_product, momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval)
        self._init_groups(param_groups)
        self._init_tail(step_tail)
        self._draw_seeds(False, param_rounding_seed, probe_seed)
        self._a, self._b = xmat_initial_state(N, preconditioner_init_scale, self._device)
        if diagonal:
            self._b = None
        self._flat_bufs = {k: torch.empty(N, dtype=torch.float32, device=self._device) for k in ("v", "h", "g")}
        self._out = torch.empty(N, dtype=torch.float32, device=self._device)

    a = property(lambda self: self._a, doc="the diagonal of Q, float32 [N], updated in place")
    b = property(lambda self: self._b, doc="the anti-diagonal of Q, float32 [N], updated in place; None when diagonal=True")

    def _flat_region(self, name, narrow=False):
        """v, h and g (the probe is drawn into v) live in buffers this object owns, on both tails; the momentum buffer is
        _FlatStep's"""
        return self._flat_bufs.get("v" if name == "probe" else name)

    def _precondition(self, v, h, grad):
        if self._device.type != "cuda":
            raise _lib.PsgdHipError("XMat.step runs on the HIP device only (the parameters are on %s); no CPU fallback" % self._device)
        if v is None:
            return precond_grad_Xmat_math(self._a, self._b, grad, out=self._out)
        return update_precond_grad_Xmat_math_(self._a, self._b, v, h, grad, float(self.lr_preconditioner), float(_psgd._tiny),
                                              out=self._out)

    # ------------------------------------------------------------------------------------------------- checkpoint / resume
    def _state_keys(self):
        return ("a",) if self._diagonal else ("a", "b")

    def _state_encode(self, sd, host):
        sd["preconditioner"] = "xmat"
        for k in self._state_keys():
            sd[k] = host(getattr(self, "_" + k))

    def _state_judge(self, sd, name, need, same):
        same("preconditioner", "xmat")
        if self._diagonal and "b" in sd:
            raise ValueError("%s: the state dict has 'b'; this optimizer is diagonal" % name)
        src = {k: need(k) for k in self._state_keys()}
        for k, t in src.items():
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(self._a.shape):
                raise ValueError("%s: %r must be a tensor of shape %s" % (name, k, tuple(self._a.shape)))
            if t.dtype != torch.float32:
                raise TypeError("%s: %r is %s; the state of class XMat is float32" % (name, k, t.dtype))
        return src

    def _state_commit(self, src):
        for k, t in src.items():
            getattr(self, "_" + k).copy_(t)
