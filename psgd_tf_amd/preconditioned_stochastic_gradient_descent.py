"""MI355X-native PSGD preconditioner engine -- host-side mirror of the reference module.

Same module name, function names, positional order and defaults as the reference
``preconditioned_stochastic_gradient_descent.py`` ("psgd.py" in the citations), so the
demo drivers' call patterns (``import preconditioned_stochastic_gradient_descent as psgd``,
hello_psgd.py:5) carry over with torch tensors in place of tf tensors:

    update_precond_dense(Q, dxs, dgs, step=0.01) -> Q                  psgd.py:26
    precond_grad_dense(Q, grads) -> list                               psgd.py:45
    update_precond_kron(Ql, Qr, dX, dG, step=0.01) -> (Ql, Qr)         psgd.py:72
    precond_grad_kron(Ql, Qr, Grad) -> Tensor                          psgd.py:116
    update_precond_splu(L12, l3, U12, u3, dxs, dgs, step=0.01) -> 4    psgd.py:396  (fp32 or bf16-stored factors)
    precond_grad_splu(L12, l3, U12, u3, grads) -> list                 psgd.py:483
    IpUVtmatvec(U, V, x)                                               psgd.py:540
    update_precond_UVd_math_(U, V, d, v, h, step, tiny) -> None        psgd.py:554  (in place)
    precond_grad_UVd_math(U, V, d, g) -> Tensor                        psgd.py:619
    class UVd(...).step(closure)                                       psgd.py:630
    class Kron(...).step(closure)                                      (extension: the train_step of mnist_with_lenet5.py:43-57)
    class SPLU(...).step(closure)                                      (extension: demo_usage_of_all_preconditioners.py:43-64)
    class Dense(...).step(closure)                                     (extension: demo_usage_of_all_preconditioners.py:26-41)

The UVd, sparse-LU and Kron arithmetic runs in hand-written HIP kernels behind the
C ABI of include/psgd_hip.h (bound in _lib.py).  Tensors must be fp32 and resident on a ROCm
device; anything else raises -- there is no CPU fallback for the hot path.  Strided views are
accepted (copied on the way in, in-place state written back on the way out); the kernels work on
contiguous memory.  The dense preconditioner (psgd.py:26-63) runs in HIP kernels too when Q and its
operands are fp32 on one ROCm device (psgd_dense.hip, O(N^2) per call); on the CPU (hello_psgd's 2x2),
in fp64 or bf16, or after ``set_dense_route("torch")``, it is the torch-op plumbing of the reference.

The reference draws its two branch decisions (psgd.py:562, :588) from TensorFlow's
global RNG; here they come from a torch.Generator (module default, or ``generator=``)
or are fixed through the keyword-only ``balance=`` / ``update_U=`` arguments.
"""
import ctypes
import os
import math

import numpy as np
import torch

from . import _lib
from . import kron as _kron
from . import uvd_wide as _wide
from . import splu_wide as _splu_wide

dtype = torch.float32                                  # psgd.py:20
_tiny = torch.finfo(torch.float32).tiny                # psgd.py:22 (smallest normal fp32)

_branch_rng = torch.Generator(device="cpu")
_branch_rng.manual_seed(0x50534744)


def manual_seed(seed):
    """Seed the generator behind the branch draws of update_precond_UVd_math_ and UVd.step."""
    _branch_rng.manual_seed(int(seed))


# --------------------------------------------------------------------------- helpers
_ws_cache = _lib.WorkspaceCache()


def _stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


def _require_hip(name, *tensors, dtypes=(), dtype_msg="fp32 tensors required"):
    """The one tensor check of the HIP entry points: every operand a torch tensor, on the HIP device, of the dtype wanted --
    dtypes[i] for tensor i, float32 for those past its end; dtype_msg: what a wrong one is told -- contiguous (the kernels take
    raw pointers), all on one device.  Returns that device."""
    dev = None
    for t, want in zip(tensors, dtypes + (torch.float32,) * (len(tensors) - len(dtypes))):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: expected torch tensors, got %r" % (name, type(t)))
        if not t.is_cuda:
            raise _lib.PsgdHipError("%s runs on the HIP device only (tensor is on %s); no CPU fallback" % (name, t.device))
        if t.dtype != want:
            raise TypeError("%s: %s, got %s" % (name, dtype_msg, t.dtype))
        if not t.is_contiguous():
            raise ValueError("%s: contiguous tensors required" % name)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError("%s: all tensors must be on one device" % name)
    return dev


def _c(t):
    """Read-only operand as the kernels need it (contiguous): a strided view is copied, as TensorFlow's ops would
    materialise it -- the reference has no notion of a non-contiguous tensor (SURVEY 8b's `ldU, ldV` are not in the ABI)."""
    return t if (not isinstance(t, torch.Tensor)) or t.is_contiguous() else t.contiguous()


class _InPlace:
    """State tensors a call updates in place (U, V, d): contiguous ones are used as they are, strided views are worked on
    as contiguous copies and written back when the call returns."""

    def __init__(self, *tensors):
        self.orig = tensors
        self.work = tuple(_c(t) for t in tensors)

    def writeback(self):
        for o, w in zip(self.orig, self.work):
            if w is not o:
                o.copy_(w)


def _workspace(kind, device, bytes_fn, *shape, limits=""):
    """Cached device workspace of `bytes_fn(*shape)` bytes, keyed by ([kind,] device index, *shape, current stream): a workspace
    carries the reduced vectors between the sweeps of one call, so calls issued on two streams must not share one (the C ABI itself
    is safe on several streams as long as each has its own workspace).  A shape the kernels do not support raises: most of the
    size functions answer with an error code, the sparse-LU one with 0 bytes (limits: what that message adds)."""
    key = kind + (device.index if device.index is not None else torch.cuda.current_device(), *map(int, shape),
                  torch.cuda.current_stream(device).cuda_stream)

    def make():
        nbytes = int(getattr(_lib.load(), bytes_fn)(*shape))
        if nbytes < 0:
            _lib.check(nbytes, bytes_fn)
        if nbytes == 0:
            raise _lib.PsgdHipError("%s: unsupported shape %r%s" % (bytes_fn, shape, limits))
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    return _ws_cache.get(key, make)


def uvd_workspace(device, N, r):
    """Cached workspace for a shard of N rows at rank r (psgd_uvd_workspace_bytes); its key has no kind: placement.UVdArena
    installs its own block under (device index, N, r, stream)."""
    return _workspace((), device, "psgd_uvd_workspace_bytes", N, r)


def uvd_bf16_workspace(device, N, r):
    """Cached workspace of the bf16-state kernels (psgd_uvd_bf16_workspace_bytes: a layout of its own)."""
    return _workspace(("uvd_bf16",), device, "psgd_uvd_bf16_workspace_bytes", N, r)


_ROUNDINGS = {"nearest": 0, "stochastic": 1}
_FP32_STATE = {}                                     # _require_hip(name, U, V, d, *vectors, **_BF16_STATE or **_FP32_STATE)
_BF16_STATE = {"dtypes": (torch.bfloat16,) * 3, "dtype_msg": "with a bfloat16 state the vectors v, h, g and out stay float32"}


def _bf16_state(name, U, V, d):
    """Classifies the state: True for a bf16-stored one (psgd_uvd_bf16.hip: U, V, d all bfloat16, rank <= 32), False for anything
    the fp32 entry points judge; raises for a float16 or mixed state and for a bfloat16 state of rank above 32."""
    state = (U, V, d)
    if not all(isinstance(t, torch.Tensor) for t in state):
        return False
    dts = {t.dtype for t in state}
    if dts == {torch.float32} or not (dts & {torch.bfloat16, torch.float16}):
        return False
    if torch.float16 in dts:
        raise TypeError("%s: a float16 state is not supported (the native narrow state is bfloat16 only)" % name)
    if dts != {torch.bfloat16}:
        raise TypeError("%s: mixed state dtypes %s; U, V and d must all be bfloat16 (or all float32)"
                        % (name, sorted(str(x) for x in dts)))
    if U.dim() == 2 and U.shape[1] > _lib.UVD_MAX_RANK:
        raise ValueError("%s: a bfloat16 state supports ranks up to %d, got %d" % (name, _lib.UVD_MAX_RANK, U.shape[1]))
    return True


def _rounding_mode(name, bf16, rounding, rounding_seed=None, row0=None):
    """The rounding arguments of an updating call, judged before a tensor is looked at, a workspace made or a number drawn:
    returns the mode.  An fp32 state (bf16 False) is not rounded: rounding arguments, row0 (row-sharded) among them, raise."""
    if rounding not in _ROUNDINGS:
        raise ValueError("%s: rounding must be 'nearest' or 'stochastic', got %r" % (name, rounding))
    mode = _ROUNDINGS[rounding]
    if not bf16 and (mode or rounding_seed is not None or row0 is not None):
        raise ValueError("%s: rounding / rounding_seed / row0 apply to a bfloat16 state only; an fp32 state is not rounded" % name)
    return mode


def _draw_branch(p, generator):
    gen = generator if generator is not None else _branch_rng
    return bool(torch.rand((), generator=gen).item() < p)


def _resolve_branches(balance, update_U, generator, mode, rounding_seed, synced=None):
    """The two branches (psgd.py:562, :588) and the rounding seed of one updating call, single-GPU or row-sharded, whose rounding
    arguments _rounding_mode has judged: (balance, update_U, seed).  Whatever is None is drawn, in the reference's order --
    balance (p = 0.01), update_U (p = 0.5), then the seed, the last only for rounding="stochastic" -- from `generator` (the
    module's branch generator when None), never from the global CUDA generator.  synced (row-sharded): () -> the
    sharded.BranchRng all ranks draw from in place of `generator`; it is synchronised by a collective the first time, so it is
    asked for only when something is drawn."""
    draw_seed = bool(mode) and rounding_seed is None
    rng = synced() if synced is not None and (balance is None or update_U is None or draw_seed) else None
    if balance is None:
        balance = _draw_branch(0.01, generator) if rng is None else rng.draw(0.01)
    if update_U is None:
        update_U = _draw_branch(0.5, generator) if rng is None else rng.draw(0.5)
    seed = 0 if rounding_seed is None else int(rounding_seed) & (2 ** 64 - 1)
    if draw_seed:
        gen = rng.gen if rng is not None else generator if generator is not None else _branch_rng
        seed = int(torch.randint(0, 2 ** 62, (), generator=gen).item())
    return bool(balance), bool(update_U), seed


def _mix64(z):
    """the splitmix64 finaliser (step seeds of class UVd)"""
    z &= 2 ** 64 - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return z ^ (z >> 31)


def uvd_step_rounding_seed(seed0, k):
    """rounding seed of step k (0, 1, ...) of a UVd optimizer whose construction seed is seed0: a hash of both, not a sum, and the
    kernels hash it again before the tensor id enters (psgd_uvd_bf16_rounding_key) -- no two (step, tensor) streams coincide"""
    return _mix64(_mix64(int(seed0)) + 0x9E3779B97F4A7C15 * (int(k) + 1))


# --------------------------------------------------------------------------- stochastic rounding of bf16 parameters
# param_rounding="stochastic" of class UVd and class Kron: the narrowing of the step-tail kernels psgd_uvd_param_update_multi_sr,
# psgd_multi_param_update_sr and psgd_multi_param_update_mixed_sr (bf16_state.h: narrow_param) restated with torch integer ops, bit
# for bit -- what step_tail="torch" runs and what the tests hold the kernels against.
_PARAM_TENSOR_ID = 16                                # the rounding stream "parameters" (bf16_state.h)
_PARAM_ROUNDINGS = ("nearest", "stochastic")
_M32 = 0xFFFFFFFF


def rounding_stream_key(seed, tensor):
    """(a, b): the two 32-bit halves of the key of one tensor's rounding stream, bf16s::make_key(seed, tensor) in Python"""
    z = _mix64(_mix64(int(seed) + 0x9E3779B97F4A7C15) ^ ((0xD1B54A32D192ED03 * (int(tensor) + 1)) & (2 ** 64 - 1)))
    return z & _M32, z >> 32


def param_rounding_addend(seed, index):
    """u of SR(x) = (bits(x) + u) >> 16 for the parameter elements whose flat indices are `index` (an int64 tensor, >= 0): the top
    16 bits of the counter hash of bf16s::narrow's mode 1 under the key of (seed, tensor id 16).  int64 arithmetic with 32-bit
    masks (a product of two 32-bit values may wrap in int64: its low 32 bits, all that is kept, are right)."""
    a, b = rounding_stream_key(seed, _PARAM_TENSOR_ID)
    index = index.to(torch.int64)
    z = ((index & _M32) * 0x9E3779B1 + a + ((index >> 32) & _M32) * 0x85EBCA77) & _M32
    z = z ^ (z >> 16)
    z = (z * 0x7FEB352D) & _M32
    z = z ^ b
    z = z ^ (z >> 15)
    z = (z * 0x846CA68B) & _M32
    z = z ^ (z >> 16)
    return z >> 16


def stochastic_narrow_bf16(x, seed, index0=0):
    """SR(x): the bfloat16 tensor the stochastic step-tail kernels store for the float32 values x, element j of x.reshape(-1)
    being the parameter element of flat index index0 + j.  (bits(x) + u) >> 16; a NaN becomes 0x7FC0, +-Inf stays, a value that
    is a bfloat16 value is unchanged, a finite value beyond the bfloat16 range may carry into +-Inf.  Any device."""
    if x.dtype != torch.float32:
        raise TypeError("stochastic_narrow_bf16: x must be float32, got %s" % (x.dtype,))
    flat = x.detach().contiguous().view(-1)
    index = torch.arange(flat.numel(), dtype=torch.int64, device=flat.device) + int(index0)
    bits = flat.view(torch.int32).to(torch.int64) & _M32
    code = ((bits + param_rounding_addend(seed, index)) >> 16) & 0xFFFF
    code = torch.where(torch.isnan(flat), torch.full_like(code, 0x7FC0), code)
    code = torch.where(code >= 2 ** 15, code - 2 ** 16, code).to(torch.int16)      # the 16 bits as they are: nothing converts
    return code.view(torch.bfloat16).view(x.shape)


def param_update_stochastic_(p, g, v, lr_eff, c, seed, index0):
    """One bfloat16 parameter tensor of the stochastic step tail, in place, as the kernels compute it: w = float(p),
    d = fl32(lr_eff * float(g)); v given: d = fl32(d + float(v)); c given: d = fl32(d + fl32(c * w)); p <- SR(fl32(w - d)) with the
    flat indices index0, index0 + 1, ...  lr_eff and c: Python floats that hold float32 values, or 0-dim float32 tensors."""
    w = p.detach().float()
    d = g.reshape(p.shape).float() * lr_eff
    if v is not None:
        d = d + v.float()
    if c is not None:
        d = d + w * c
    p.detach().copy_(stochastic_narrow_bf16(w - d, seed, index0))
    return p


def _param_rounding(name, param_rounding, dtype):
    """the param_rounding argument of a constructor, judged before anything touches a device: True for "stochastic".  dtype: the
    parameters' dtype, or (mixed_dtypes=True) the collection of the dtypes present: "stochastic" then rounds the bfloat16
    tensors, and needs one of them and no float16 tensor"""
    if param_rounding not in _PARAM_ROUNDINGS:
        raise ValueError("%s: param_rounding must be 'nearest' or 'stochastic', got %r" % (name, param_rounding))
    if param_rounding == "stochastic" and isinstance(dtype, (set, frozenset, list, tuple)):
        if torch.float16 in dtype or torch.bfloat16 not in dtype:
            raise ValueError("%s: param_rounding='stochastic' rounds the bfloat16 parameters of a mixed list: it needs at least one "
                             "and no float16 parameter (float16 stochastic rounding is not supported), got %s"
                             % (name, sorted(str(d) for d in set(dtype))))
    elif param_rounding == "stochastic" and dtype != torch.bfloat16:
        raise ValueError("%s: param_rounding='stochastic' needs bfloat16 parameters, got %s (float32 parameters are not rounded; "
                         "float16 stochastic rounding is not supported)" % (name, dtype))
    return param_rounding == "stochastic"


def _param_rounding_encode(sd, stochastic, seed0, step):
    """the checkpoint keys of the parameters' rounding stream, added to sd when the switch is on (both classes); returns sd"""
    if stochastic:
        sd["param_round_seed0"], sd["param_round_step"] = int(seed0), int(step)
    return sd


def _param_rounding_decode(name, sd, stochastic, seed0):
    """(seed0, step) after loading sd into an optimizer whose own seed is seed0: the dict's pair where it has one; the
    optimizer's seed with the counter at 0 where it has none; a nearest optimizer ignores the keys and gets (seed0, 0)"""
    if not stochastic or "param_round_seed0" not in sd:
        return seed0, 0
    if "param_round_step" not in sd:
        raise ValueError("%s: the state dict has 'param_round_seed0' but no 'param_round_step'" % name)
    return int(sd["param_round_seed0"]), int(sd["param_round_step"])


# --------------------------------------------------------------------------- counter-based probe vectors
# The draws of psgd_multi_randn_f32 (class Kron(preconditioner_fit="whitening"), multi_tail.multi_randn) restated in numpy: the
# hash in integer arithmetic, Box-Muller in float64.  The kernel evaluates the same expressions in float32, so the two agree to a
# few float32 ulps, not bit for bit (profiles/kron_whitening.txt has the measured distance).
_PROBE_TENSOR_ID = 17                                # the stream "probe vectors" (bf16_state.h)
_GOLDEN64 = 0x9E3779B97F4A7C15


def counter_randn(seed, index0, n, scale=1.0):
    """The n float32 values psgd_multi_randn_f32 defines for the flat indices index0 .. index0 + n - 1 under `seed`, as a numpy
    array, evaluated in float64 and rounded to float32 once: element i is float32(scale) * float32(z_i) with, for the pair
    j = i >> 1 and K = the 64-bit key of (seed, tensor id 17),
        h = mix64(K + 0x9E3779B97F4A7C15 * (j + 1));  u1 = ((h >> 32) + 1) * 2^-32;  theta = 2 pi (h & 0xFFFFFFFF) * 2^-32
        z_{2j} = sqrt(-2 ln u1) cos(theta),  z_{2j+1} = sqrt(-2 ln u1) sin(theta).
    The draw of an element depends on (seed, i) alone: counter_randn(s, i0, n)[a:b] == counter_randn(s, i0 + a, b - a).  The
    per-step seed of class Kron is uvd_step_rounding_seed(probe_seed0, probe_step)."""
    import numpy as np
    index0, n = int(index0), int(n)
    if index0 < 0 or n < 0:
        raise ValueError("counter_randn: index0 and n must be >= 0, got %r and %r" % (index0, n))
    if not math.isfinite(float(scale)):
        raise ValueError("counter_randn: scale must be finite, got %r" % (scale,))
    a, b = rounding_stream_key(seed, _PROBE_TENSOR_ID)
    K = a | (b << 32)
    j0, j1 = index0 >> 1, (index0 + n + 1) >> 1                       # the pairs that cover the range
    # Python integers in an object array: _mix64 itself, element by element, with no width to overflow
    j = np.arange(j1 - j0, dtype=np.int64).astype(object) + j0
    h = _mix64(K + _GOLDEN64 * (j + 1))
    hi = (h >> 32).astype(np.float64)
    lo = (h & _M32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log((hi + 1.0) * 2.0 ** -32))
    theta = (2.0 * np.pi) * (lo * 2.0 ** -32)
    z = np.stack([r * np.cos(theta), r * np.sin(theta)], axis=1).reshape(-1)
    z = z[index0 - 2 * j0: index0 - 2 * j0 + n].astype(np.float32)
    return np.float32(scale) * z


_PRECONDITIONER_FITS = ("hessian", "whitening")


def _probe_encode(sd, whitening, seed0, step):
    """the checkpoint keys of the probe stream, added to sd when the optimizer fits by gradient whitening (both classes); returns sd"""
    if whitening:
        sd["probe_seed0"], sd["probe_step"] = int(seed0), int(step)
    return sd


def _probe_decode(sd, whitening, seed0, name="load_state_dict"):
    """(seed0, step) after loading sd into an optimizer whose own probe seed is seed0: the dict's pair where it has one; the
    optimizer's seed with the counter at 0 where it has none (a dict of a hessian-fit optimizer); a hessian-fit optimizer ignores
    the keys and gets (seed0, 0)"""
    if not whitening or "probe_seed0" not in sd:
        return seed0, 0
    if "probe_step" not in sd:
        raise ValueError("%s: the state dict has 'probe_seed0' but no 'probe_step'" % name)
    return int(sd["probe_seed0"]), int(sd["probe_step"])


_UVD_TENSOR_IDS = {"U": 0, "V": 1, "d": 2}           # the tensor ids of psgd_uvd_bf16_rounding_key
_NARROW_STAGING_BYTES = 64 << 20                     # UVd.load_state_dict: the fp32 staging buffer of an fp32 -> native bf16 load


def uvd_bf16_narrow_(dst, src, *, tensor, index0=0, rounding="nearest", rounding_seed=0):
    """dst <- the bf16 codes of the fp32 values src, narrowed as the bf16-state kernels narrow what they write
    (psgd_uvd_bf16_narrow_f32): dst bfloat16 and src float32 on one ROCm device, contiguous, of one size.  tensor: "U", "V" or "d"
    (the rounding stream of that state tensor under rounding_seed); index0: the flat GLOBAL element index of src[0] in it --
    (row0 + first row) * r for a factor, row0 + first row for d -- so the codes depend on neither the chunks nor the row split.
    Returns dst."""
    name = "uvd_bf16_narrow_"
    if tensor not in _UVD_TENSOR_IDS:
        raise ValueError("%s: tensor must be 'U', 'V' or 'd', got %r" % (name, tensor))
    mode = _rounding_mode(name, True, rounding)
    _require_hip(name, dst, src, dtypes=(torch.bfloat16,), dtype_msg="dst must be bfloat16 and src float32")
    if dst.numel() != src.numel():
        raise ValueError("%s: dst and src must be of one size" % name)
    if int(index0) < 0:
        raise ValueError("%s: index0 must be >= 0, got %r" % (name, index0))
    if dst.numel():
        rc = _lib.load().psgd_uvd_bf16_narrow_f32(src.data_ptr(), dst.data_ptr(), dst.numel(), int(index0), _UVD_TENSOR_IDS[tensor],
                                                  mode, int(rounding_seed) & (2 ** 64 - 1), _stream_ptr(dst.device))
        _lib.check(rc, "psgd_uvd_bf16_narrow_f32")
    return dst


def _uvd_shapes(name, U, V, *cols):
    if U.dim() != 2 or V.shape != U.shape:
        raise ValueError("%s: U and V must both be [N, r]" % name)
    N, r = U.shape
    for c in cols:
        if c.numel() != N or (c.dim() == 2 and c.shape[1] != 1) or c.dim() > 2:
            raise ValueError("%s: column vectors must be [N] or [N, 1] with N = %d" % (name, N))
    return N, r


# --------------------------------------------------------------------------- dense
_dense_route = "native"


def set_dense_route(route):
    """"native" (default): fp32 operands on one ROCm device run the HIP kernels of psgd_dense.hip; "torch": the torch-op
    plumbing below for every operand (A/B runs).  CPU, fp64 and bf16 operands take the torch ops under either route."""
    global _dense_route
    if route not in ("native", "torch"):
        raise ValueError("set_dense_route: route must be 'native' or 'torch', got %r" % (route,))
    _dense_route = route


def _dense_native(Q, *lists):
    """True when the call goes to the kernels: route "native", Q and every list entry fp32 tensors on one ROCm device."""
    if _dense_route != "native" or not isinstance(Q, torch.Tensor) or not Q.is_cuda or Q.dtype != torch.float32:
        return False
    return all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == Q.device for xs in lists for t in xs)


def _dense_workspace(device, N):
    return _workspace(("dense",), device, "psgd_dense_workspace_bytes", N)


def _dense_n(name, Q):
    if Q.dim() != 2 or Q.shape[0] != Q.shape[1]:
        raise ValueError("%s: Q must be N x N, got %s" % (name, tuple(Q.shape)))
    return Q.shape[0]


def _update_dense_native(Q, dxs, dgs, step):
    Q = _c(Q)
    N = _dense_n("update_precond_dense", Q)
    dx, dg = _tall("update_precond_dense", dxs, N), _tall("update_precond_dense", dgs, N)
    dev = _require_hip("update_precond_dense", Q, dx, dg)
    out = torch.empty((N, N), dtype=Q.dtype, device=dev)
    ws = _dense_workspace(dev, N)
    rc = _lib.load().psgd_dense_update_f32(Q.data_ptr(), dx.data_ptr(), dg.data_ptr(), out.data_ptr(), N, float(step),
                                           float(_tiny), ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    _lib.check(rc, "psgd_dense_update_f32")
    return out


def _precond_grad_dense_native(Q, grads):
    Q = _c(Q)
    N = _dense_n("precond_grad_dense", Q)
    g = _tall("precond_grad_dense", grads, N)
    dev = _require_hip("precond_grad_dense", Q, g)
    out = torch.empty(N, dtype=Q.dtype, device=dev)
    ws = _dense_workspace(dev, N)
    rc = _lib.load().psgd_dense_apply_f32(Q.data_ptr(), g.data_ptr(), out.data_ptr(), N, ws.data_ptr(), ws.numel(),
                                          _stream_ptr(dev))
    _lib.check(rc, "psgd_dense_apply_f32")
    pre_grads, idx = [], 0
    for x in grads:
        n = x.numel()
        pre_grads.append(torch.reshape(out[idx:idx + n], x.shape))
        idx = idx + n
    return pre_grads


def update_precond_dense(Q, dxs, dgs, step=0.01):
    """psgd.py:26-42.  fp32 on a ROCm device: psgd_dense_update_f32 (O(N^2), never forms G; Q is not modified).  Anything else
    (hello_psgd's 2x2 on the CPU, fp64, bf16), or set_dense_route("torch"): the torch ops below."""
    if _dense_native(Q, dxs, dgs):
        return _update_dense_native(Q, dxs, dgs, step)
    dx = torch.cat([torch.reshape(x, [-1, 1]) for x in dxs], 0)
    dg = torch.cat([torch.reshape(g, [-1, 1]) for g in dgs], 0)
    a = Q @ dg
    b = torch.linalg.solve_triangular(Q.t(), dx, upper=False)      # Q^T b = dx  (:39, adjoint=True)
    grad = torch.triu(a @ a.t() - b @ b.t())
    step0 = step / (torch.max(torch.abs(grad)) + torch.finfo(Q.dtype).tiny)
    return Q - (step0 * grad) @ Q


def precond_grad_dense(Q, grads):
    """psgd.py:45-63: list in, list out with the original shapes.  Routes as update_precond_dense (psgd_dense_apply_f32)."""
    if _dense_native(Q, grads):
        return _precond_grad_dense_native(Q, grads)
    cols = [torch.reshape(g, [-1, 1]) for g in grads]
    lens = [c.shape[0] for c in cols]
    grad = torch.cat(cols, 0)
    pre_grad = Q.t() @ (Q @ grad)
    pre_grads, idx = [], 0
    for g, n in zip(grads, lens):
        pre_grads.append(torch.reshape(pre_grad[idx:idx + n], g.shape))
        idx = idx + n
    return pre_grads


# --------------------------------------------------------------------------- Kron
def update_precond_kron(Ql, Qr, dX, dG, step=0.01):
    """psgd.py:72-110 (shape dispatch of SURVEY Appendix B); returns (Ql_new, Qr_new)."""
    return _kron.update_precond_kron(Ql, Qr, dX, dG, step)


def precond_grad_kron(Ql, Qr, Grad):
    """psgd.py:116-152; returns the preconditioned gradient, same shape as Grad."""
    return _kron.precond_grad_kron(Ql, Qr, Grad)


def update_precond_kron_batched(Qls, Qrs, dXs, dGs, step=0.01):
    """Extension: the list comprehension of mnist_with_lenet5.py:51 as one batched call."""
    return _kron.update_precond_kron_batched(Qls, Qrs, dXs, dGs, step)


def precond_grad_kron_batched(Qls, Qrs, Grads):
    """Extension: the list comprehension of mnist_with_lenet5.py:53 as one batched call."""
    return _kron.precond_grad_kron_batched(Qls, Qrs, Grads)


# --------------------------------------------------------------------------- sparse LU
_SPLU_LIMITS = " (1 <= r <= %d, N >= r)" % _lib.SPLU_MAX_RANK


def _splu_workspace(device, N, r):
    return _workspace(("splu",), device, "psgd_splu_workspace_bytes", N, r, limits=_SPLU_LIMITS)


def _splu_shapes(name, L12, l3, U12, u3):
    if L12.dim() != 2 or U12.dim() != 2 or U12.shape != (L12.shape[1], L12.shape[0]):
        raise ValueError("%s: L12 must be [N, r] and U12 [r, N]" % name)
    N, r = L12.shape
    for c in (l3, u3):
        if c.numel() != N - r or c.dim() > 2 or (c.dim() == 2 and c.shape[1] != 1):
            raise ValueError("%s: l3 and u3 must be [N - r, 1] with N - r = %d" % (name, N - r))
    return N, r


def _tall(name, xs, N):
    """psgd.py:426-427 / :495-497: the list as one tall column vector (device-side cat; plumbing)."""
    flat = torch.cat([torch.reshape(x, [-1]) for x in xs], 0) if len(xs) != 1 else torch.reshape(xs[0], [-1])
    if flat.numel() != N:
        raise ValueError("%s: the list holds %d elements, the preconditioner is for %d" % (name, flat.numel(), N))
    return flat.contiguous()


def _splu_chunked(r):
    """ranks above PSGD_SPLU_MAX_RANK (64) run on column chunks (splu_wide.py); PSGD_SPLU_CHUNKS=1 sends ranks 33 .. 64 there too
    (the route of rounds 3-4: A/B runs of tools/r05_wide_rank.py)."""
    return r > _lib.SPLU_MAX_RANK or (r > _lib.UVD_MAX_RANK and os.environ.get("PSGD_SPLU_CHUNKS") == "1")


_SPLU_BF16_STATE = {"dtypes": (torch.bfloat16,) * 4,
                    "dtype_msg": "with a bfloat16 state the vectors dx, dg, g stay float32"}


def _splu_bf16_workspace(device, N, r):
    """Cached workspace of the bf16-state sparse-LU kernels (psgd_splu_bf16_workspace_bytes: a layout of its own)."""
    return _workspace(("splu_bf16",), device, "psgd_splu_bf16_workspace_bytes", N, r)


def _splu_bf16_state(name, L12, l3, U12, u3):
    """Classifies the sparse-LU state, as _bf16_state does for UVd: True for a bf16-stored one (psgd_splu_bf16.hip: all four
    factors bfloat16, rank <= 32), False for anything the fp32 entry points judge; raises for a float16 or mixed state and for a
    bfloat16 state of rank above 32 (the wider native kernels and the chunked route of splu_wide.py are fp32 only)."""
    state = (L12, l3, U12, u3)
    if not all(isinstance(t, torch.Tensor) for t in state):
        return False
    dts = {t.dtype for t in state}
    if dts == {torch.float32} or not (dts & {torch.bfloat16, torch.float16}):
        return False
    if torch.float16 in dts:
        raise TypeError("%s: a float16 state is not supported (the native narrow state is bfloat16 only)" % name)
    if dts != {torch.bfloat16}:
        raise TypeError("%s: mixed state dtypes %s; L12, l3, U12 and u3 must all be bfloat16 (or all float32)"
                        % (name, sorted(str(x) for x in dts)))
    if L12.dim() == 2 and L12.shape[1] > _lib.UVD_MAX_RANK:
        raise ValueError("%s: a bfloat16 state supports ranks up to %d, got %d" % (name, _lib.UVD_MAX_RANK, L12.shape[1]))
    return True


def _unflatten(out, grads):
    """psgd.py:518-522: the flat result as a list shaped like grads."""
    pre_grads, idx = [], 0
    for x in grads:
        n = x.numel()
        pre_grads.append(torch.reshape(out[idx:idx + n], x.shape))
        idx += n
    return pre_grads


def update_precond_splu(L12, l3, U12, u3, dxs, dgs, step=0.01, *, rounding="nearest", rounding_seed=None):
    """psgd.py:396-480: returns (L12_new, l3_new, U12_new, u3_new); inputs are not modified.

    A bfloat16 L12, l3, U12, u3 (all four; fp32 dxs, dgs; r <= 32) is updated by the bf16-state kernels (psgd_splu_bf16.hip) and
    four bfloat16 tensors come back: fp64 arithmetic on the widened codes, each written element narrowed once --
    rounding="nearest" or "stochastic" (seeded by rounding_seed; None draws one from the module's branch generator).  The
    balance of :411-417 rescales every element, so every element of the state is re-rounded by every call.  An fp32 state is
    not rounded: any rounding other than the default, or a rounding_seed, raises ValueError there."""
    name = "update_precond_splu"
    L12, l3, U12, u3 = _c(L12), _c(l3), _c(U12), _c(u3)
    bf16 = _splu_bf16_state(name, L12, l3, U12, u3)
    mode = _rounding_mode(name, bf16, rounding, rounding_seed)
    dev = _require_hip(name, L12, l3, U12, u3, **(_SPLU_BF16_STATE if bf16 else _FP32_STATE))
    N, r = _splu_shapes(name, L12, l3, U12, u3)
    dx, dg = _tall(name, dxs, N), _tall(name, dgs, N)
    _require_hip(name, dx, dg)
    if dx.device != dev or dg.device != dev:
        raise ValueError("%s: all tensors must be on one device" % name)
    if bf16:
        seed = 0 if rounding_seed is None else int(rounding_seed) & (2 ** 64 - 1)
        if mode and rounding_seed is None:
            seed = int(torch.randint(0, 2 ** 62, (), generator=_branch_rng).item())
        out = [torch.empty_like(t) for t in (L12, l3, U12, u3)]
        ws = _splu_bf16_workspace(dev, N, r)
        rc = _lib.load().psgd_splu_update_bf16(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(), dx.data_ptr(),
                                               dg.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                               out[3].data_ptr(), N, r, float(step), float(_tiny), mode, seed, ws.data_ptr(),
                                               ws.numel(), _stream_ptr(dev))
        _lib.check(rc, "psgd_splu_update_bf16")
        return tuple(out)
    if _splu_chunked(r):                           # wide rank: column chunks of L2 and U2' (splu_wide.py)
        return _splu_wide.update(L12, l3, U12, u3, dx, dg, float(step), float(_tiny), uvd_workspace)
    out = [torch.empty_like(t) for t in (L12, l3, U12, u3)]
    ws = _splu_workspace(dev, N, r)
    rc = _lib.load().psgd_splu_update_f32(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(), dx.data_ptr(),
                                          dg.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                          out[3].data_ptr(), N, r, float(step), float(_tiny), ws.data_ptr(), ws.numel(),
                                          _stream_ptr(dev))
    _lib.check(rc, "psgd_splu_update_f32")
    return tuple(out)


def precond_grad_splu(L12, l3, U12, u3, grads):
    """psgd.py:483-524: list of gradients in, list of preconditioned gradients (same shapes) out.
    A bfloat16 L12, l3, U12, u3 (all four, r <= 32; psgd_splu_bf16.hip): fp32 gradients in, fp32 preconditioned gradients out."""
    name = "precond_grad_splu"
    L12, l3, U12, u3 = _c(L12), _c(l3), _c(U12), _c(u3)
    bf16 = _splu_bf16_state(name, L12, l3, U12, u3)
    dev = _require_hip(name, L12, l3, U12, u3, **(_SPLU_BF16_STATE if bf16 else _FP32_STATE))
    N, r = _splu_shapes(name, L12, l3, U12, u3)
    g = _tall(name, grads, N)
    _require_hip(name, g)
    if g.device != dev:
        raise ValueError("%s: all tensors must be on one device" % name)
    if not bf16 and _splu_chunked(r):
        return _unflatten(_splu_wide.precond_grad(L12, l3, U12, u3, g, uvd_workspace), grads)
    out = torch.empty_like(g)
    ws = (_splu_bf16_workspace if bf16 else _splu_workspace)(dev, N, r)
    fn = "psgd_splu_apply_bf16" if bf16 else "psgd_splu_apply_f32"
    rc = getattr(_lib.load(), fn)(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(), g.data_ptr(), out.data_ptr(),
                                  N, r, ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    _lib.check(rc, fn)
    return _unflatten(out, grads)


# --------------------------------------------------------------------------- UVd math
def IpUVtmatvec(U, V, x):
    """psgd.py:540-544: (I + U V') x for a column vector x ([N] or [N,1]) or [N,k] matrix."""
    U, V = _c(U), _c(V)
    if not (isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] > 1):
        x = _c(x)
    if U.dim() == 2 and U.shape[1] > _lib.UVD_MAX_RANK:
        _require_hip("IpUVtmatvec", U, V, x)
        return _wide.ipuvt_matvec(U, V, x, uvd_workspace)
    if x.dim() == 2 and x.shape[1] > 1:
        # a matrix x: its columns go through as contiguous vectors (two small transposes, N k floats each), U and V are
        # swept once per group of four columns
        dev = _require_hip("IpUVtmatvec", U, V)
        if not x.is_cuda or x.dtype != torch.float32:
            _require_hip("IpUVtmatvec", x)
        N, r = _uvd_shapes("IpUVtmatvec", U, V)
        if x.shape[0] != N:
            raise ValueError("IpUVtmatvec: x must have N = %d rows" % N)
        k = x.shape[1]
        xt = x.t().contiguous()
        ot = torch.empty_like(xt)
        ws = uvd_workspace(dev, N, r)
        xs = (ctypes.c_void_p * k)(*[xt[j].data_ptr() for j in range(k)])
        os_ = (ctypes.c_void_p * k)(*[ot[j].data_ptr() for j in range(k)])
        rc = _lib.load().psgd_uvd_ipuvt_matvec_cols_f32(U.data_ptr(), V.data_ptr(), xs, os_, k, N, r, ws.data_ptr(),
                                                         ws.numel(), _stream_ptr(dev))
        _lib.check(rc, "psgd_uvd_ipuvt_matvec_cols_f32")
        return ot.t().contiguous()
    dev = _require_hip("IpUVtmatvec", U, V, x)
    N, r = _uvd_shapes("IpUVtmatvec", U, V, x)
    out = torch.empty_like(x)
    ws = uvd_workspace(dev, N, r)
    rc = _lib.load().psgd_uvd_ipuvt_matvec_f32(U.data_ptr(), V.data_ptr(), x.data_ptr(), out.data_ptr(), N, r,
                                                ws.data_ptr(), ws.numel(), _stream_ptr(dev))
    _lib.check(rc, "psgd_uvd_ipuvt_matvec_f32")
    return out


def _cols_of(name, x, N):
    """A matrix operand [N, k] as k contiguous columns: its transpose, materialised once ([k, N] row-major; a transposed view of a
    [k, N] tensor is used as it is)."""
    if x.shape[0] != N:
        raise ValueError("%s: the matrix must have N = %d rows" % (name, N))
    xt = x.t()
    return xt if xt.is_contiguous() else xt.contiguous()


def _vector_call(name, bf16, U, V, d, cols, out=None):
    """what the vector forms of the three UVd calls share once the state is classified: the tensor check (a bf16 state keeps
    fp32 vectors), the shapes and the (workspace pointer, bytes, stream) tail of the kernels' argument lists -- the bf16-state
    kernels have a workspace layout of their own; None above rank 32, where uvd_wide.py brings its own and `out` is ignored.
    Returns (N, r, tail)."""
    dev = _require_hip(name, U, V, d, *cols, **(_BF16_STATE if bf16 else _FP32_STATE))
    N, r = _uvd_shapes(name, U, V, d, *cols)
    if r > _lib.UVD_MAX_RANK:
        return N, r, None
    if out is not None:
        _require_hip(name, out, cols[-1])
        if out.shape != cols[-1].shape:
            raise ValueError("%s: out must be shaped like g" % name)
    ws = (uvd_bf16_workspace if bf16 else uvd_workspace)(dev, N, r)
    return N, r, (ws.data_ptr(), ws.numel(), _stream_ptr(dev))


def precond_grad_UVd_math(U, V, d, g, *, out=None):
    """psgd.py:619-627: d .* (I + V U')(I + U V')(d .* g); returns a new tensor shaped like g.
    g is a column vector ([N] or [N, 1]) or, as the reference's docstring allows (:623), a matrix [N, k]: d broadcasts over
    the columns and U, V are swept once per group of four columns (psgd_uvd_apply_cols_f32).
    out (extension; column-vector g, r <= 32): a contiguous fp32 tensor shaped like g to write the result to (placement.UVdArena.out).
    A bfloat16 U, V, d (psgd_uvd_bf16.hip): fp32 column vector g, r <= 32."""
    name = "precond_grad_UVd_math"
    U, V, d = _c(U), _c(V), _c(d)
    bf16 = _bf16_state(name, U, V, d)
    if isinstance(g, torch.Tensor) and g.dim() == 2 and g.shape[1] > 1:
        if bf16:
            raise ValueError("%s: a matrix g is not supported with a bfloat16 state (column vectors only)" % name)
        dev = _require_hip(name, U, V, d)
        if not g.is_cuda or g.dtype != torch.float32 or g.device != dev:
            _require_hip(name, U, g)
        N, r = _uvd_shapes(name, U, V, d)
        gt = _cols_of(name, g, N)
        k = gt.shape[0]
        if r > _lib.UVD_MAX_RANK:
            return _wide.precond_grad(U, V, d, [gt[j] for j in range(k)], uvd_workspace).t().contiguous()
        ot = torch.empty_like(gt)
        ws = uvd_workspace(dev, N, r)
        gs = (ctypes.c_void_p * k)(*[gt[j].data_ptr() for j in range(k)])
        os_ = (ctypes.c_void_p * k)(*[ot[j].data_ptr() for j in range(k)])
        rc = _lib.load().psgd_uvd_apply_cols_f32(U.data_ptr(), V.data_ptr(), d.data_ptr(), gs, os_, k, N, r, ws.data_ptr(),
                                                  ws.numel(), _stream_ptr(dev))
        _lib.check(rc, "psgd_uvd_apply_cols_f32")
        return ot.t().contiguous()
    g = _c(g)
    N, r, tail = _vector_call(name, bf16, U, V, d, (g,), out)
    if tail is None:                               # wide rank: column chunks through the same kernels (uvd_wide.py)
        return _wide.precond_grad(U, V, d, g, uvd_workspace)
    out = torch.empty_like(g) if out is None else out
    lib = _lib.load()
    rc = (lib.psgd_uvd_apply_bf16 if bf16 else lib.psgd_uvd_apply_f32)(
        U.data_ptr(), V.data_ptr(), d.data_ptr(), g.data_ptr(), out.data_ptr(), N, r, *tail)
    _lib.check(rc, "psgd_uvd_apply_bf16" if bf16 else "psgd_uvd_apply_f32")
    return out


def update_precond_UVd_math_(U, V, d, v, h, step, tiny, *, balance=None, update_U=None, generator=None,
                             rounding="nearest", rounding_seed=None):
    """psgd.py:554-617.  Updates U or V, and d, IN PLACE; returns None.

    balance / update_U fix the two random branches of the reference (:562 p=0.01, :588 p=0.5);
    left at None they are drawn from `generator` (a CPU torch.Generator; module default otherwise),
    in the reference's order.

    A bfloat16 U, V, d (all three; fp32 v, h; r <= 32) is updated by the bf16-state kernels: fp32 arithmetic, each written
    element narrowed once -- rounding="nearest" or "stochastic" (seeded by rounding_seed; None draws one from `generator` /
    the module's branch generator after the branch draws).  An fp32 state is not rounded: any rounding other than the default, or
    a rounding_seed, raises ValueError there."""
    name = "update_precond_UVd_math_"
    state = _InPlace(U, V, d)
    (U, V, d), v, h = state.work, _c(v), _c(h)
    bf16 = _bf16_state(name, U, V, d)
    mode = _rounding_mode(name, bf16, rounding, rounding_seed)
    N, r, tail = _vector_call(name, bf16, U, V, d, (v, h))
    balance, update_U, seed = _resolve_branches(balance, update_U, generator, mode, rounding_seed)
    if tail is None:
        _wide.update(U, V, d, v, h, float(step), float(tiny), balance, update_U, uvd_workspace)
    elif bf16:
        rc = _lib.load().psgd_uvd_update_bf16(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(), h.data_ptr(), N, r,
                                               float(step), float(tiny), balance, update_U, mode, seed, *tail)
        _lib.check(rc, "psgd_uvd_update_bf16")
    else:
        rc = _lib.load().psgd_uvd_update_f32(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(), h.data_ptr(), N, r,
                                              float(step), float(tiny), balance, update_U, *tail)
        _lib.check(rc, "psgd_uvd_update_f32")
    state.writeback()
    return None


def update_precond_UVd_math_and_precond_grad(U, V, d, v, h, g, step, tiny, *, balance=None, update_U=None,
                                             generator=None, out=None, rounding="nearest", rounding_seed=None):
    """Extension: update_precond_UVd_math_(U, V, d, v, h, step, tiny) followed by
    precond_grad_UVd_math(U, V, d, g) on the updated state -- the UVd.step pattern (psgd.py:732 -> :748) --
    as one fused call that saves a pass over V.  U or V, and d, are updated in place; returns the
    preconditioned gradient.  out (optional): a contiguous fp32 tensor shaped like g to write it to (placement.UVdArena.out:
    where the output stream lives is worth 4 % of the last sweep); ranks above 32 ignore it.
    A bfloat16 state: rounding / rounding_seed as in update_precond_UVd_math_; the gradient is preconditioned with the state as
    it was stored (rounded)."""
    name = "update_precond_UVd_math_and_precond_grad"
    state = _InPlace(U, V, d)
    (U, V, d), v, h, g = state.work, _c(v), _c(h), _c(g)
    bf16 = _bf16_state(name, U, V, d)
    mode = _rounding_mode(name, bf16, rounding, rounding_seed)
    N, r, tail = _vector_call(name, bf16, U, V, d, (v, h, g), out)
    balance, update_U, seed = _resolve_branches(balance, update_U, generator, mode, rounding_seed)
    if tail is None:                               # ranks 33 .. 64: the fused sequence of uvd_wide.update_apply; above: update, then apply
        out = _wide.update_apply(U, V, d, v, h, g, float(step), float(tiny), balance, update_U, uvd_workspace)
        state.writeback()
        return out
    out = torch.empty_like(g) if out is None else out
    if bf16:
        rc = _lib.load().psgd_uvd_update_apply_bf16(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(), h.data_ptr(),
                                                     g.data_ptr(), out.data_ptr(), N, r, float(step), float(tiny), balance,
                                                     update_U, mode, seed, *tail)
        _lib.check(rc, "psgd_uvd_update_apply_bf16")
    else:
        rc = _lib.load().psgd_uvd_update_apply_f32(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(), h.data_ptr(),
                                                    g.data_ptr(), out.data_ptr(), N, r, float(step), float(tiny), balance,
                                                    update_U, *tail)
        _lib.check(rc, "psgd_uvd_update_apply_f32")
    state.writeback()
    return out


# --------------------------------------------------------------------------- UVd step tail (psgd_uvd_tail.hip)
# What class UVd does around the preconditioner call -- psgd.py:729-730 / :747 (lists of tensors -> flat vectors), :753-754 (clip norm)
# and :757-762 (parameter update) -- in a number of launches that does not depend on how many parameter tensors there are.
_TAIL_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def uvd_tail_chunks(sizes):
    """The chunk table of the step-tail kernels for tensors of these element counts (include/psgd_hip.h): an int64 numpy array
    [nchunks, 2] of (segment, offset inside the segment), one row per piece of at most _lib.UVD_TAIL_CHUNK elements, segments in
    order.  Every element of every segment is in exactly one chunk; a segment of 0 elements has none."""
    import numpy as np
    sizes = np.asarray(list(sizes), dtype=np.int64).reshape(-1)
    if (sizes < 0).any():
        raise ValueError("uvd_tail_chunks: negative size")
    per = (sizes + (_lib.UVD_TAIL_CHUNK - 1)) // _lib.UVD_TAIL_CHUNK
    seg = np.repeat(np.arange(len(sizes), dtype=np.int64), per)
    first = np.cumsum(per) - per
    off = (np.arange(int(per.sum()), dtype=np.int64) - np.repeat(first, per)) * _lib.UVD_TAIL_CHUNK
    return np.stack([seg, off], axis=1)


class _SegTable:
    """The device segment table {pointer, start, count} of one list of tensors.  The host copy lives in pinned memory; the table is
    uploaded (one asynchronous copy on the current stream) only when a pointer differs from the last upload."""

    def __init__(self, starts, sizes, device):
        k = len(sizes)
        self.host = torch.zeros((k, 3), dtype=torch.int64).pin_memory()
        self.rows = self.host.numpy()
        self.rows[:, 1] = starts
        self.rows[:, 2] = sizes
        self.dev = torch.zeros((k, 3), dtype=torch.int64, device=device)
        self.ptrs, self.uploaded = None, None

    def refresh(self, ptrs):
        if ptrs != self.ptrs:
            if self.uploaded is not None:
                self.uploaded.synchronize()                     # the previous upload has read the pinned rows (long ago, normally)
            self.rows[:, 0] = ptrs
            self.dev.copy_(self.host, non_blocking=True)
            self.uploaded = torch.cuda.Event()
            self.uploaded.record()
            self.ptrs = ptrs
        return self.dev.data_ptr()


class UVdTailPlan:
    """Everything about a list of parameter tensors that the step-tail kernels need and that does not change from step to step:
    sizes, start offsets, the chunk table on the device, one segment table per role ("params", "vs", "v", "h", "g", ...), the
    device double of the clip norm and the workspace of its reduction.  Calls that share a plan must run on one stream.

    dtype: one dtype for all tensors, or a list with one per tensor (a MIXED plan when more than one is present: mixed is True,
    dtype and code are None).  The kernels take the element type per launch, so a mixed list is served by the typed entry points
    launched once per dtype present over that dtype's rows of the chunk table (by_dtype, dtype_chunks); the segment tables are
    the one-dtype ones -- a table holds nothing typed -- and a launch never follows the pointer of a tensor of another dtype,
    because no chunk of its sub-plan names that segment.  tiny: the largest finfo(T).tiny over the dtypes present."""

    def __init__(self, sizes, dtype, device):
        self.sizes = tuple(int(n) for n in sizes)
        dtypes = tuple(dtype) if isinstance(dtype, (list, tuple)) else (dtype,) * len(self.sizes)
        if len(dtypes) != len(self.sizes):
            raise ValueError("UVd step tail: %d dtypes for %d tensors" % (len(dtypes), len(self.sizes)))
        for dt in dtypes if dtypes else (dtype,):
            if dt not in _TAIL_DTYPES:
                raise TypeError("UVd step tail: tensors must be float32, bfloat16 or float16, got %s" % (dt,))
        self.dtypes = dtypes
        self.present = tuple(dt for dt in _TAIL_DTYPES if dt in set(dtypes)) or (dtype,)     # in the order float32, bfloat16, float16
        self.mixed = len(self.present) > 1
        self.dtype = None if self.mixed else self.present[0]
        self.code, self.device = None if self.mixed else _TAIL_DTYPES[self.dtype], torch.device(device)
        self.tiny = max(torch.finfo(dt).tiny for dt in self.present)
        self.starts, acc = [], 0
        for n in self.sizes:
            self.starts.append(acc)
            acc += n
        self.total = acc
        chunks = self._host_chunks = uvd_tail_chunks(self.sizes)
        self.nchunks = int(chunks.shape[0])
        self.chunks = torch.from_numpy(chunks).to(self.device) if self.nchunks else None
        self._group_chunks, self._dtype_chunks = {}, {}
        # what a typed launch over the whole list walks: (dtype code, device chunk table, rows), one entry per dtype present
        self.by_dtype = self.dtype_chunks(None)
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.ws = torch.empty(_lib.UVD_SUMSQ_WS_BYTES, dtype=torch.uint8, device=self.device)
        # the flag words of the guarded step (uvd_pack(flag=, stamp=), uvd_check): slots v, h, g and one spare.  Zero ONCE, here:
        # the kernels store a stamp the caller has not used before, so nothing ever clears them again
        self.flags = torch.zeros(4, dtype=torch.int32, device=self.device)
        self._tables = {}

    def table(self, role, tensors, what, dtype=None):
        """device pointer of the segment table of `tensors` in this role (uploaded when a pointer changed).  Every tensor is
        checked against its own dtype: the plan's for its position, or `dtype` (one for all, or a list with one per tensor)"""
        if len(tensors) != len(self.sizes):
            raise ValueError("%s: %d tensors, the plan has %d" % (what, len(tensors), len(self.sizes)))
        dev = self.device
        dts = self.dtypes if dtype is None else dtype if isinstance(dtype, (list, tuple)) else (dtype,) * len(self.sizes)
        for t, n, dt in zip(tensors, self.sizes, dts):
            if t.dtype != dt or t.device != dev or t.numel() != n or not t.is_contiguous():
                raise ValueError("%s: every tensor must be a contiguous %s tensor on %s with the plan's element count (%d), got %s %s "
                                 "%s%s" % (what, dt, dev, n, t.dtype, t.device, tuple(t.shape), "" if t.is_contiguous() else " strided"))
        tab = self._tables.get(role)
        if tab is None:
            tab = self._tables[role] = _SegTable(self.starts, self.sizes, dev)
        return tab.refresh([t.data_ptr() for t in tensors])

    def group_chunks(self, indices):
        """(device chunk table, its row count) of the SUB-PLAN of the tensors at `indices` (a tuple, ascending): the rows of the
        plan's chunk table whose segment is one of them, in the plan's order.  A launch over it walks these tensors only and reads
        the plan's own segment tables, all k rows of them: a segment keeps its row, its pointer and its `start` (the offset in the
        flat order that the flat gradient and the stochastic-rounding index are taken from), so nothing about an element depends
        on the grouping, and a table whose pointers change from step to step (vs, a gradient list) is still uploaded once, not
        once per group.  Made at the first call for these indices and kept: an upload of 16 bytes per chunk, nothing N-sized."""
        got = self._group_chunks.get(indices)
        if got is None:
            rows = self._host_chunks[np.isin(self._host_chunks[:, 0], np.asarray(indices, dtype=np.int64))]
            while len(self._group_chunks) >= 64:
                self._group_chunks.pop(next(iter(self._group_chunks)))
            got = self._group_chunks[indices] = (torch.from_numpy(np.ascontiguousarray(rows)).to(self.device) if len(rows) else None,
                                                 int(rows.shape[0]))
        return got

    def dtype_chunks(self, indices=None):
        """[(PSGD_DTYPE_* code, device chunk table, its row count)]: the SUB-PLAN per dtype present, in the order float32,
        bfloat16, float16, of the whole list (indices None: what by_dtype holds, made at construction) or of the tensors at
        `indices`, the (group, dtype) pairs of a group.  Each is group_chunks of the tensors of that dtype among them: the sub-plans
        partition the chunk table (the group's rows of it), keep its order and leave every segment its row, pointer and `start`.
        A pair without a chunk is left out: it is not launched.  A one-dtype plan answers with its own table (the group's) under
        its one code.  Kept per `indices`, like group_chunks."""
        got = self._dtype_chunks.get(indices)
        if got is None:
            if not self.mixed:
                one = (self.chunks, self.nchunks) if indices is None else self.group_chunks(indices)
                got = [(self.code,) + one] if one[1] else []
            else:
                among = range(len(self.sizes)) if indices is None else indices
                got = []
                for dt in self.present:
                    chunks, nchunks = self.group_chunks(tuple(i for i in among if self.dtypes[i] == dt))
                    if nchunks:
                        got.append((_TAIL_DTYPES[dt], chunks, nchunks))
            while len(self._dtype_chunks) >= 64:
                self._dtype_chunks.pop(next(iter(self._dtype_chunks)))
            self._dtype_chunks[indices] = got
        return got


def tail_launch_count(dtypes, sizes, groups=None, *, packs=1, sums=1):
    """The launches of one fused step tail over tensors of these dtypes and element counts, counted on the host:
        (packs x D) + sums + (number of (group, dtype) pairs that hold an element)
    packs: the typed roles launched over the whole list (pack, pack-blend, pack-check, check, widen-check, the perturbation of
    psgd.py:723), each once per dtype present that holds an element, D <= 3; sums: the float32-only launches, which stay single
    (the sum of squares of class UVd is one, that of class Kron two); groups: a partition of range(len(sizes)) into index
    tuples (None: one group), each launched once per dtype it holds elements of."""
    dtypes, sizes = list(dtypes), [int(n) for n in sizes]
    if len(dtypes) != len(sizes):
        raise ValueError("tail_launch_count: %d dtypes for %d sizes" % (len(dtypes), len(sizes)))
    groups = [tuple(range(len(sizes)))] if groups is None else [tuple(g) for g in groups]
    D = len({dt for dt, n in zip(dtypes, sizes) if n})
    pairs = sum(len({dtypes[i] for i in g if sizes[i]}) for g in groups)
    return int(packs) * D + int(sums) + pairs


def mixed_dtype_constants(dtypes):
    """(tiny, delta_param_scale) that an optimizer with mixed_dtypes=True shares among tensors of these dtypes: the LARGEST
    finfo(T).tiny (psgd.py:682, the floor of the clip norm) and the LARGEST finfo(T).eps ** 0.5 (:683; one perturbation scale for
    the whole vector, since the finite difference of :716-727 perturbs all parameters jointly).  Neither depends on the order;
    with one dtype both are that dtype's values."""
    present = set(dtypes)
    return max(torch.finfo(dt).tiny for dt in present), max(torch.finfo(dt).eps ** 0.5 for dt in present)


def _tensor_groups(what, tensor_groups, k, weight_decay, pre):
    """The tensor_groups argument of a functional step tail, checked: a list of (indices, lr_scale, weight_decay) -- sorted index
    tuples that partition range(k), lr_scale a finite float >= 0, weight_decay a float >= 0.  None stays None."""
    if tensor_groups is None:
        return None
    if float(weight_decay) != 0.0:
        raise ValueError("%s: with tensor_groups every group brings its own weight_decay; leave the weight_decay argument at 0" % what)
    if not pre:
        raise ValueError("%s: tensor_groups apply to the update; the perturbation p + v is one launch over all tensors" % what)
    out, seen = [], set()
    for j, group in enumerate(tensor_groups):
        try:
            indices, scale, wd = group
            indices, scale, wd = tuple(sorted(int(i) for i in indices)), float(scale), float(wd)
        except (TypeError, ValueError):
            raise ValueError("%s: tensor_groups[%d] must be (indices, lr_scale, weight_decay), got %r" % (what, j, group))
        if not indices:
            raise ValueError("%s: tensor_groups[%d] has no indices" % (what, j))
        if not (scale >= 0.0 and math.isfinite(scale)):
            raise ValueError("%s: tensor_groups[%d]: lr_scale must be finite and >= 0, got %r" % (what, j, scale))
        if not wd >= 0.0:
            raise ValueError("%s: tensor_groups[%d]: weight_decay must be >= 0, got %r" % (what, j, wd))
        for i in indices:
            if not 0 <= i < k or i in seen:
                raise ValueError("%s: tensor_groups must partition range(%d); index %d of tensor_groups[%d] is %s"
                                 % (what, k, i, j, "listed twice" if i in seen else "out of range"))
            seen.add(i)
        out.append((indices, scale, wd))
    if len(seen) != k:
        raise ValueError("%s: tensor_groups must partition range(%d); %r are in no group" % (what, k, sorted(set(range(k)) - seen)))
    return out


_tail_plans = {}    # (device, dtype, sizes) -> UVdTailPlan of the calls that bring none (a model has one or two such keys)


def _tail_plan(tensors, what):
    if not tensors:
        raise ValueError("%s: empty tensor list" % what)
    t0 = tensors[0]
    if not isinstance(t0, torch.Tensor) or not t0.is_cuda:
        raise _lib.PsgdHipError("%s runs on the HIP device only; no CPU fallback" % what)
    key = (t0.device, t0.dtype, tuple(int(t.numel()) for t in tensors))
    plan = _tail_plans.get(key)
    if plan is None:
        while len(_tail_plans) >= 16:
            _tail_plans.pop(next(iter(_tail_plans)))
        plan = _tail_plans[key] = UVdTailPlan(key[2], t0.dtype, t0.device)
    return plan


def _flag_word(what, flag, stamp, dev):
    """the device pointer of a guard flag (one int32 word on dev) after the checks the host can make"""
    if not isinstance(flag, torch.Tensor) or flag.dtype != torch.int32 or flag.device != dev or flag.numel() < 1:
        raise ValueError("%s: flag must be an int32 tensor of at least one element on %s" % (what, dev))
    if int(stamp) != stamp:
        raise ValueError("%s: stamp must be an integer, got %r" % (what, stamp))
    return flag.data_ptr()


def uvd_pack(tensors, out, scale=1.0, *, plan=None, role="pack", flag=None, stamp=None):
    """out[:n] = torch.cat([t.reshape(-1) for t in tensors]).float() * scale in ONE launch whatever len(tensors) (psgd.py:729-730, :747;
    scale: the 1 / delta_param_scale of :734-736).  tensors: contiguous device tensors of one dtype (float32, bfloat16 or float16;
    with a plan built for a mixed list each of its own, one launch per dtype present, sharing the flag word), empty ones allowed; out: a contiguous fp32 device tensor of at least n elements.  Returns out's first n elements, flat.
    flag and stamp (both or neither): the same bits from psgd_uvd_pack_check_f32, which also stores stamp (1 .. 2^31 - 1, one the
    caller has not used on this word before) to flag[0], an int32 device word, when a value it writes is not finite; the caller
    reads flag[0] == stamp after the launch.  Nothing zeroes the word."""
    tensors = list(tensors)
    if (flag is None) != (stamp is None):
        raise ValueError("uvd_pack: flag and stamp go together (got flag=%s, stamp=%r)" % ("None" if flag is None else "given", stamp))
    plan = plan if plan is not None else _tail_plan(tensors, "uvd_pack")
    dev = _require_hip("uvd_pack", out)
    if out.numel() < plan.total:
        raise ValueError("uvd_pack: out has %d elements, the tensors have %d" % (out.numel(), plan.total))
    segs = plan.table(role, tensors, "uvd_pack")
    word = None if flag is None else _flag_word("uvd_pack", flag, stamp, plan.device)
    for code, chunks, nchunks in plan.by_dtype:                  # one launch; a mixed plan: one per dtype present, one flag word
        if flag is not None:
            rc = _lib.load().psgd_uvd_pack_check_f32(segs, len(tensors), chunks.data_ptr(), nchunks, code, float(scale),
                                                     out.data_ptr(), word, int(stamp), _stream_ptr(dev))
            _lib.check(rc, "psgd_uvd_pack_check_f32")
        else:
            rc = _lib.load().psgd_uvd_pack_f32(segs, len(tensors), chunks.data_ptr(), nchunks, code, float(scale),
                                               out.data_ptr(), _stream_ptr(dev))
            _lib.check(rc, "psgd_uvd_pack_f32")
    return out.view(-1)[:plan.total]


def uvd_check(tensors, scale=1.0, *, plan=None, role="check", flag, stamp):
    """The predicate of uvd_pack(..., flag=, stamp=) without the pack (psgd_uvd_check_multi): stamp is stored to flag[0] when
    float32(t) * scale is not finite for an element t of any tensor.  Every element is read once in its own dtype and nothing else is
    written.  For the gradients of a momentum step, which must be judged BEFORE uvd_pack_blend overwrites the buffer."""
    tensors = list(tensors)
    plan = plan if plan is not None else _tail_plan(tensors, "uvd_check")
    dev = plan.device
    if dev.type != "cuda":
        raise _lib.PsgdHipError("uvd_check runs on the HIP device only; no CPU fallback")
    segs = plan.table(role, tensors, "uvd_check")
    word = _flag_word("uvd_check", flag, stamp, dev)
    for code, chunks, nchunks in plan.by_dtype:
        rc = _lib.load().psgd_uvd_check_multi(segs, len(tensors), chunks.data_ptr(), nchunks, code, float(scale), word,
                                              int(stamp), _stream_ptr(dev))
        _lib.check(rc, "psgd_uvd_check_multi")


def uvd_loss_scale_next(scale, good_steps, skipped, *, growth_interval, growth=2.0, backoff=0.5, min_scale=1.0, max_scale=2.0 ** 24):
    """The dynamic loss-scale schedule of class UVd as a pure function: (scale, good_steps) after one more step.  A skipped step
    multiplies the scale by backoff and sets the counter to 0; growth_interval good steps in a row multiply it by growth and set the
    counter to 0; the scale stays in [min_scale, max_scale].  With the defaults every scale is a power of two."""
    scale, good_steps = float(scale), int(good_steps)
    if skipped:
        return max(scale * backoff, float(min_scale)), 0
    good_steps += 1
    if good_steps >= int(growth_interval):
        return min(scale * growth, float(max_scale)), 0
    return scale, good_steps


def uvd_momentum_coefficients(k, momentum):
    """(beta_k, 1 - beta_k) of step k (counted from 0) as Python floats that hold float32 values: beta_k = float32(min(k / (k + 1),
    momentum)), the warm-up of the PyTorch PSGD optimizers (the first step has beta = 0), and float32(1) - beta_k rounded once --
    the pair every tail of class UVd and the kernel receive, so that host and device cannot disagree"""
    import numpy as np
    beta = np.float32(min(k / (k + 1.0), float(momentum)))
    return float(beta), float(np.float32(1.0) - beta)


def uvd_pack_blend(tensors, out, beta, scale=1.0, *, plan=None, role="pack"):
    """uvd_pack BLENDED into out, the momentum buffer, in ONE launch: with x = torch.cat([...]).float() * scale,
        out[:n] = beta * out[:n] + (float32(1) - float32(beta)) * x
    every product and the sum rounded to float32 on its own (out.mul_(beta); out.add_(x.mul(1 - beta)) in torch).  beta == 0 does
    not read out: whatever it held, NaN included, is replaced by x.  Arguments as uvd_pack; 0 <= beta < 1."""
    import numpy as np
    tensors = list(tensors)
    beta = float(np.float32(beta))
    if not 0.0 <= beta < 1.0:
        raise ValueError("uvd_pack_blend: beta must be in [0, 1), got %r" % (beta,))
    omb = float(np.float32(1.0) - np.float32(beta))
    plan = plan if plan is not None else _tail_plan(tensors, "uvd_pack_blend")
    dev = _require_hip("uvd_pack_blend", out)
    if out.numel() < plan.total:
        raise ValueError("uvd_pack_blend: out has %d elements, the tensors have %d" % (out.numel(), plan.total))
    segs = plan.table(role, tensors, "uvd_pack_blend")
    for code, chunks, nchunks in plan.by_dtype:
        rc = _lib.load().psgd_uvd_pack_blend_f32(segs, len(tensors), chunks.data_ptr(), nchunks, code, float(scale),
                                                 beta, omb, out.data_ptr(), _stream_ptr(dev))
        _lib.check(rc, "psgd_uvd_pack_blend_f32")
    return out.view(-1)[:plan.total]


def uvd_sumsq(x, *, plan):
    """plan.sumsq[0] = sum of fl32(x * x) in fp64, fixed order (the square of the clip norm of psgd.py:753); returns that tensor"""
    dev = _require_hip("uvd_sumsq", x)
    rc = _lib.load().psgd_uvd_sumsq_f32(x.data_ptr(), x.numel(), plan.sumsq.data_ptr(), plan.ws.data_ptr(), plan.ws.numel(),
                                        _stream_ptr(dev))
    _lib.check(rc, "psgd_uvd_sumsq_f32")
    return plan.sumsq


def uvd_step_tail(params, pre_grad, lr, max_norm=None, tiny=None, vs=None, group=None, *, plan=None, weight_decay=0.0,
                  rounding="nearest", rounding_seed=None, index0=0, tensor_groups=None):
    """psgd.py:750-762 on all parameters in place, in launches that do not depend on len(params):
        lr_eff = lr                                                         (max_norm None or inf, :750-751)
                 lr * min(max_norm / (||pre_grad|| + tiny), 1)              (:753-754; the norm never reaches the host)
        p <- T(p - delta),  delta = T(fl32(lr_eff * pre_grad slice)),  with vs: delta = T(delta + v)        (:757-762)
    with T the parameters' dtype: the roundings of the torch expressions of class UVd.  params (and vs): contiguous device tensors
    of one dtype; pre_grad: the flat fp32 preconditioned gradient of their concatenation.  tiny defaults to the dtype's smallest
    normal (:682).  With a plan built for a MIXED list (UVdTailPlan(sizes, [one dtype per tensor], device)) every tensor has its
    own T: each launch below runs once per dtype present over that dtype's sub-plan, rounding="stochastic" applies to the
    bfloat16 tensors (the float32 ones: as under "nearest"; a float16 one is refused) and tiny defaults to the largest present.
    group: pre_grad holds this rank's rows of a row-sharded vector -- the sum of squares is all-reduced (one fp64
    scalar, the collective sharded.global_norm uses).  pre_grad None (vs required): p <- T(p + v), the perturbation of :723.
    weight_decay (extension, decoupled): with c = fl32(lr_eff * weight_decay), delta = T(delta + T(fl32(c * p))) after the vs term;
    0 (default) adds no rounding step.
    rounding="stochastic" (bfloat16 parameters, pre_grad required; psgd_uvd_param_update_multi_sr): the update is formed once in
    float32 and narrowed once, with w = float(p): d = fl32(lr_eff * g); d = fl32(d + float(v)); d = fl32(d + fl32(c * w));
    p <- SR(fl32(w - d)), SR the stochastic narrowing of stochastic_narrow_bf16 under rounding_seed (None: drawn from the module's
    branch generator) on the flat index index0 + the element's place in the concatenation of params (index0: this rank's first
    row on a row-sharded vector).  With "nearest" (default) nothing changes, and rounding_seed / index0 must be left alone.
    tensor_groups (extension; None: nothing changes): a sequence of (indices, lr_scale, weight_decay) that partitions
    range(len(params)); weight_decay itself must then be left at 0.  The sum of squares -- of the WHOLE pre_grad, before any scale
    -- is taken once (and all-reduced once), then the update entry point is launched once per group over the group's chunks
    (UVdTailPlan.group_chunks) with lr_j = fl32(float(lr) * lr_scale_j), the product formed in double and rounded once, and the
    group's weight_decay: lr_eff_j = fl32(double(lr_j) * the clip factor), c_j = fl32(lr_eff_j * fl32(wd_j)), and a group whose
    weight_decay is 0 takes the form without the decay term.  The stochastic-rounding index of an element does not depend on
    the grouping.
    The parameters are written through their pointers: autograd's version counters do not move."""
    params = list(params)
    if rounding not in _PARAM_ROUNDINGS:
        raise ValueError("uvd_step_tail: rounding must be 'nearest' or 'stochastic', got %r" % (rounding,))
    sr = rounding == "stochastic"
    if not sr and (rounding_seed is not None or index0 != 0):
        raise ValueError("uvd_step_tail: rounding_seed and index0 apply to rounding='stochastic' only")
    if sr and (pre_grad is None or int(index0) < 0):
        raise ValueError("uvd_step_tail: rounding='stochastic' needs pre_grad (the perturbation p + v rounds to nearest) and index0 >= 0")
    plan = plan if plan is not None else _tail_plan(params, "uvd_step_tail")
    if sr and plan.mixed:
        _param_rounding("uvd_step_tail", rounding, plan.present)
    elif sr and plan.dtype != torch.bfloat16:
        raise ValueError("uvd_step_tail: rounding='stochastic' needs bfloat16 parameters, got %s" % (plan.dtype,))
    dev = plan.device
    psegs = plan.table("params", params, "uvd_step_tail")
    vsegs = plan.table("vs", list(vs), "uvd_step_tail (vs)") if vs is not None else None
    clip = max_norm is not None and not math.isinf(float(max_norm))
    sumsq = None
    wd = float(weight_decay)
    if not wd >= 0.0:
        raise ValueError("uvd_step_tail: weight_decay must be >= 0, got %r" % (weight_decay,))
    groups = _tensor_groups("uvd_step_tail", tensor_groups, len(params), wd, pre_grad is not None)
    if pre_grad is None:
        if vsegs is None or clip or wd != 0.0:
            raise ValueError("uvd_step_tail: pre_grad=None adds vs to the parameters; it needs vs and takes no max_norm and no "
                             "weight_decay")
    else:
        _require_hip("uvd_step_tail", pre_grad)
        if pre_grad.device != dev or pre_grad.numel() != plan.total:
            raise ValueError("uvd_step_tail: pre_grad must hold the %d elements of the parameters on %s" % (plan.total, dev))
        if clip:
            sumsq = uvd_sumsq(pre_grad, plan=plan)
            if group is not None:
                from . import sharded as _sharded
                _sharded.all_reduce_sum_f64_(sumsq, group)
    if not plan.nchunks:
        return
    tiny = plan.tiny if tiny is None else tiny
    if sr and rounding_seed is None:
        rounding_seed = int(torch.randint(0, 2 ** 62, (), generator=_branch_rng).item())
    # one launch over the plan's chunks, or one per group over the group's: the same tables, the same sum of squares.  A mixed
    # plan: each of these once per dtype present, with that dtype's code, over that dtype's rows
    launches = [sub + (float(lr), wd) for sub in plan.by_dtype] if groups is None else \
        [sub + (float(lr) * scale, wd_j) for indices, scale, wd_j in groups for sub in plan.dtype_chunks(indices)]
    for code, chunks, nchunks, lr_j, wd_j in launches:
        args = (psegs, vsegs, len(params), chunks.data_ptr(), nchunks, code,
                None if pre_grad is None else pre_grad.data_ptr(), lr_j, None if sumsq is None else sumsq.data_ptr(),
                float(max_norm) if clip else 0.0, float(tiny))
        if sr and code == _lib.DTYPE_BF16:                      # (the float32 tensors of a mixed list: as under "nearest")
            rc = _lib.load().psgd_uvd_param_update_multi_sr(*args, wd_j, int(rounding_seed) & (2 ** 64 - 1), int(index0),
                                                            _stream_ptr(dev))
            _lib.check(rc, "psgd_uvd_param_update_multi_sr")
        elif wd_j == 0.0:
            rc = _lib.load().psgd_uvd_param_update_multi(*args, _stream_ptr(dev))
            _lib.check(rc, "psgd_uvd_param_update_multi")
        else:
            rc = _lib.load().psgd_uvd_param_update_multi_wd(*args, wd_j, _stream_ptr(dev))
            _lib.check(rc, "psgd_uvd_param_update_multi_wd")


# --------------------------------------------------------------------------- UVd optimizer wrapper
class _Hyper:
    """Stand-in for the non-trainable tf.Variable hyper-parameters of psgd.py:673-680:
    change them with .assign(value), read them with float()/bool()."""

    def __init__(self, value):
        self.value = value

    def assign(self, value):
        self.value = value.value if isinstance(value, _Hyper) else value
        return self

    def numpy(self):
        return self.value

    def __float__(self):
        return float(self.value)

    def __bool__(self):
        return bool(self.value)

    def __repr__(self):
        return "_Hyper(%r)" % (self.value,)


class _ParamGroup:
    """One entry of opt.param_groups: indices, a tuple of positions in the optimizer's parameter order (ascending), and the two
    _Hyper objects lr_scale and weight_decay (None: the group follows opt.weight_decay).  A schedule changes them with .assign();
    every step reads and checks them again."""

    def __init__(self, indices, lr_scale, weight_decay):
        self.indices = tuple(int(i) for i in indices)
        self.lr_scale, self.weight_decay = _Hyper(lr_scale), _Hyper(weight_decay)

    def __repr__(self):
        return "_ParamGroup(indices=%r, lr_scale=%r, weight_decay=%r)" % (self.indices, self.lr_scale.value, self.weight_decay.value)


def _group_values(name, which, lr_scale, weight_decay):
    """(lr_scale, weight_decay) of one parameter group as floats, checked: lr_scale finite and >= 0, weight_decay None or >= 0"""
    try:
        scale = float(lr_scale)
        wd = None if weight_decay is None else float(weight_decay)
    except (TypeError, ValueError):
        raise ValueError("%s: %s: lr_scale must be a float and weight_decay a float or None, got %r and %r"
                         % (name, which, lr_scale, weight_decay))
    if not (scale >= 0.0 and math.isfinite(scale)):
        raise ValueError("%s: %s: lr_scale must be finite and >= 0, got %r" % (name, which, lr_scale))
    if wd is not None and not wd >= 0.0:
        raise ValueError("%s: %s: weight_decay must be >= 0 (or None: the optimizer's), got %r" % (name, which, weight_decay))
    return scale, wd


class _StepFeatures:
    """What the flat classes (_FlatStep: UVd, SPLU, Dense) and class Kron share, written once.  The switches: momentum, weight
    decay, nonfinite="skip", the loss scale, parameter groups (param_groups: a learning-rate scale and a weight decay per group of
    tensors; _init_groups, _step_groups), the seeds drawn at construction, the stream of param_rounding="stochastic", the
    preconditioner_fit switch with the state of its probe stream (probe_seed0 / probe_step) and the guard's checkpoint keys.  The
    parts of a step that no preconditioner shapes: the reference's five hyper-parameters (_HYPER_KEYS, _init_step_hypers), the
    route and the closure front (_step_route; _closure_gradients, the one place that calls the closure), the coefficients of the
    torch tail (_tail_coefficients) and the keywords of the fused one (_fused_tail_kwargs).
    The class that inherits this provides self._params (the parameters, in order), self._generator and, where param_rounding is
    on, _param_round_seed0 / _param_round_step.  Messages carry the name of that class.  The schedules (uvd_loss_scale_next,
    uvd_momentum_coefficients, uvd_step_rounding_seed) are looked up in this module at the call."""

    _HYPER_KEYS = ("lr_params", "lr_preconditioner", "grad_clip_max_norm", "preconditioner_update_probability",
                   "exact_hessian_vector_product")

    def _init_step_hypers(self, lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                          exact_hessian_vector_product):
        """psgd.py:673-680: the five _Hyper objects of _HYPER_KEYS; grad_clip_max_norm=None means no clipping (inf)"""
        self.lr_params = _Hyper(lr_params)                                                   # :673
        self.lr_preconditioner = _Hyper(lr_preconditioner)                                   # :674
        self.grad_clip_max_norm = _Hyper(math.inf if grad_clip_max_norm is None else grad_clip_max_norm)  # :675-678
        self.preconditioner_update_probability = _Hyper(preconditioner_update_probability)  # :679
        self.exact_hessian_vector_product = _Hyper(bool(exact_hessian_vector_product))       # :680

    # ------------------------------------------------------------------------------------------------- the front of a step
    def _step_route(self, update_Q):
        """how this step feeds the preconditioner update, from its coin: None leaves the preconditioner alone; "whitening" (that
        fit, whatever exact_hessian_vector_product says), "exact" (Hessian-vector products) or "fd" (finite differences)"""
        if not update_Q:
            return None
        return "whitening" if self._whiten else "exact" if bool(self.exact_hessian_vector_product) else "fd"

    def _closure_gradients(self, closure, route, scaled, randn, delta, perturb=None):
        """The closure front of a step (psgd.py:706-727, :737-744): (closure_returns, grads, second, vs).  The ORDER is a contract:
        it fixes which draws a step consumes, and tools/class_step_digest.py replays it on the CPU.
        1. closure() under enable_grad; what it returns is passed through untouched (the loss is _loss_of it).
        2. grads = autograd.grad(scaled(loss), params), create_graph=True only for "exact"; they come back without a graph.
        3. "exact" and "fd": vs = one randn(p) per parameter, in parameter order; "fd": times delta (a Python float), in p's dtype.
        4. "exact": second = the Hessian-vector products autograd.grad(grads, params, vs), which carry no graph.
        5. "fd": the perturbation of :723 under no_grad -- perturb(vs), the class's list kernel, or with perturb=None (the torch
           tail) p.add_(v) per tensor; the caller takes it back -- then closure() again: second = the perturbed gradients.
        6. "whitening" and None: no draw, second = vs = None.
        scaled: _step_scales's.  randn and perturb are hooks: there the classes differ (_randn_like; Kron's generator=)."""
        params = self._params
        second = vs = None
        with torch.enable_grad():
            closure_returns = closure()
            grads = torch.autograd.grad(scaled(self._loss_of(closure_returns)), params, create_graph=route == "exact")
            if route == "exact":
                vs = [randn(p) for p in params]
                second = list(torch.autograd.grad(grads, params, vs))
                grads = [g.detach() for g in grads]
        if route == "fd":
            vs = [randn(p) * delta for p in params]
            with torch.no_grad():
                if perturb is not None:
                    perturb(vs)
                else:
                    for p, v in zip(params, vs):
                        p.add_(v)
            with torch.enable_grad():
                second = torch.autograd.grad(scaled(self._loss_of(closure())), params)
        return closure_returns, grads, second, vs

    # ------------------------------------------------------------------------------------------------- the tail of a step
    @staticmethod
    def _tail_coefficients(lr, wd, groups, max_norm, sumsq, tiny, k):
        """[(lr_eff, c or None)] * k of the torch tail, one pair per parameter tensor for _torch_param_update_: the rule the
        step-tail kernels implement (fl32: rounded to float32; lr_scale_j = 1 and wd_j = wd without groups):
            lr_j = fl32(lr lr_scale_j), the product in double
            lr_eff_j = lr_j without a clip, else fl32(double(lr_j) min(fl32(max_norm) / (sqrt(sumsq) + fl32(tiny)), 1)) in double
            c_j = fl32(lr_eff_j fl32(wd_j)); None where fl32(wd_j) == 0: no decay term is formed
        groups: _step_groups's.  sumsq: None for no clip, else the caller's fp64 0-dim device tensor, the sum of squares of the whole
        preconditioned gradient.  No host read: with a clip 0-dim float32 device tensors (NaN from a NaN sumsq), else Python floats."""
        f32 = lambda x: float(np.float32(x))
        ratio = None
        if sumsq is not None:
            ratio = torch.clamp(torch.full_like(sumsq, f32(max_norm)) / (torch.sqrt(sumsq) + f32(tiny)), max=1.0)

        def pair(lr_j, wd_j):
            lr_j, wd_j = f32(lr_j), f32(wd_j)
            if ratio is None:
                return lr_j, None if wd_j == 0.0 else float(np.float32(lr_j) * np.float32(wd_j))
            lr_j = (lr_j * ratio).float()
            return lr_j, None if wd_j == 0.0 else lr_j * wd_j
        if groups is None:
            return [pair(lr, wd)] * k
        out = [None] * k
        for indices, scale, wd_j in groups:
            out_j = pair(lr * scale, wd_j)
            for i in indices:
                out[i] = out_j
        return out

    @staticmethod
    def _fused_tail_kwargs(groups, wd, sr, sr_seed, index0=0):
        """what weight decay, the groups (in its place: one launch of the update per group) and param_rounding (sr: this step's
        seed and the GLOBAL flat index of the first element) add to the call of uvd_step_tail / multi_param_update"""
        kw = dict(weight_decay=wd) if groups is None else dict(tensor_groups=groups)
        return dict(kw, rounding="stochastic", rounding_seed=sr_seed, index0=index0) if sr else kw

    def _init_features(self, momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval):
        """momentum, weight_decay (off by default; _Hyper objects like the others), nonfinite, loss_scale,
        loss_scale_growth_interval of a constructor, checked in this order before anything touches a device.  nonfinite="propagate"
        is the code path from before the guard; "skip": a step with a non-finite input changes nothing.  loss_scale: None, a power
        of two, or "dynamic" (starts at 2^16, uvd_loss_scale_next); a _Hyper that holds the CURRENT scale."""
        name = type(self).__name__
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError("%s: momentum must be in [0, 1), got %r" % (name, momentum))
        if not float(weight_decay) >= 0.0:
            raise ValueError("%s: weight_decay must be >= 0, got %r" % (name, weight_decay))
        if nonfinite not in ("propagate", "skip"):
            raise ValueError("%s: nonfinite must be 'propagate' or 'skip', got %r" % (name, nonfinite))
        self._guard = nonfinite == "skip"
        if loss_scale is not None and not self._guard:
            raise ValueError("%s: loss_scale needs nonfinite='skip' (a scaled gradient that overflows must not reach the state)" % name)
        self._dynamic_scale = isinstance(loss_scale, str)
        if self._dynamic_scale and loss_scale != "dynamic":
            raise ValueError("%s: loss_scale must be None, a power of two or 'dynamic', got %r" % (name, loss_scale))
        self.momentum = _Hyper(momentum)
        self.weight_decay = _Hyper(weight_decay)
        self.loss_scale = _Hyper(2.0 ** 16 if self._dynamic_scale else loss_scale)
        self._loss_scale_value()
        self.loss_scale_growth_interval = int(loss_scale_growth_interval)
        if self.loss_scale_growth_interval < 1:
            raise ValueError("%s: loss_scale_growth_interval must be >= 1, got %r" % (name, loss_scale_growth_interval))
        self._m, self._m_step, self._good_steps = None, 0, 0
        self.skipped_steps, self.last_step_skipped = 0, False

    def _loss_scale_value(self):
        """the current loss scale S as a float (1.0 without loss scaling), checked: a power of two"""
        S = self.loss_scale.value
        if S is None:
            return 1.0
        S = float(S)
        if not (S > 0.0 and math.isfinite(S) and math.frexp(S)[0] == 0.5):
            raise ValueError("%s: loss_scale must be a power of two (1 / loss_scale must be exact), got %r"
                             % (type(self).__name__, self.loss_scale.value))
        return S

    def _hyper_momentum(self):
        mom, wd = float(self.momentum), float(self.weight_decay)
        if not 0.0 <= mom < 1.0:
            raise ValueError("%s: momentum must be in [0, 1), got %r" % (type(self).__name__, mom))
        if not wd >= 0.0:
            raise ValueError("%s: weight_decay must be >= 0, got %r" % (type(self).__name__, wd))
        return mom, wd

    def _step_scales(self):
        """(mom, wd, S, inv, scaled) of one step: the checked momentum and weight decay, the loss scale S (1.0 unguarded),
        inv = 1 / S and the function that scales the loss"""
        mom, wd = self._hyper_momentum()
        S = self._loss_scale_value() if self._guard else 1.0
        inv = 1.0 / S                                           # exact: S is a power of two
        return mom, wd, S, inv, (lambda loss: loss) if S == 1.0 else (lambda loss: loss * S)

    # ------------------------------------------------------------------------------------------------- parameter groups
    param_groups = None                  # _init_groups makes it a list of _ParamGroup where the constructor was given groups

    def _init_groups(self, param_groups):
        """the param_groups argument of a constructor, judged against self._params before anything touches a device: None, or a
        sequence of dicts {"params": [tensors], "lr_scale": 1.0, "weight_decay": None}.  Tensors are matched by identity; the
        parameters named in no group form an implicit last group (lr_scale 1.0, weight_decay None: it follows opt.weight_decay).
        Sets self.param_groups (None without groups)."""
        name = type(self).__name__
        if param_groups is None:
            return
        place = {id(p): i for i, p in enumerate(self._params)}
        groups, seen = [], set()
        for j, g in enumerate(param_groups):
            if not isinstance(g, dict):
                raise ValueError("%s: param_groups[%d] must be a dict with 'params', got %r" % (name, j, type(g)))
            unknown = sorted(set(g) - {"params", "lr_scale", "weight_decay"}, key=str)
            if unknown:
                raise ValueError("%s: param_groups[%d] has unknown key%s %s (a group holds 'params', 'lr_scale' and 'weight_decay')"
                                 % (name, j, "" if len(unknown) == 1 else "s", ", ".join(repr(k) for k in unknown)))
            tensors = g.get("params")
            tensors = [tensors] if isinstance(tensors, torch.Tensor) else list(tensors if tensors is not None else ())
            if not tensors:
                raise ValueError("%s: param_groups[%d] has no 'params'" % (name, j))
            indices = []
            for t in tensors:
                i = place.get(id(t))
                if i is None:
                    raise ValueError("%s: param_groups[%d] names a tensor%s that is not one of this optimizer's parameters (they are "
                                     "matched by identity, and only those that require grad count)"
                                     % (name, j, " of shape %s" % (tuple(t.shape),) if isinstance(t, torch.Tensor) else ""))
                if i in seen:
                    raise ValueError("%s: parameter %d (shape %s) is listed twice in param_groups (again in group %d)"
                                     % (name, i, tuple(t.shape), j))
                seen.add(i)
                indices.append(i)
            scale, wd = _group_values(name, "param_groups[%d]" % j, g.get("lr_scale", 1.0), g.get("weight_decay"))
            groups.append(_ParamGroup(sorted(indices), scale, wd))
        rest = [i for i in range(len(self._params)) if i not in seen]
        if rest:
            groups.append(_ParamGroup(rest, 1.0, None))
        self.param_groups = groups

    def _step_groups(self, wd):
        """None without groups; else [(indices, lr_scale, weight_decay)] of this step, the values read from the groups' _Hyper
        objects and checked again (a schedule may have assigned anything); a weight_decay of None follows wd, opt.weight_decay"""
        if self.param_groups is None:
            return None
        name = type(self).__name__
        out = []
        for j, g in enumerate(self.param_groups):
            scale, gwd = _group_values(name, "param_groups[%d]" % j, g.lr_scale.value, g.weight_decay.value)
            out.append((g.indices, scale, wd if gwd is None else gwd))
        return out

    def _groups_encode(self, sd):
        """the checkpoint key of the groups, added to sd when the constructor was given groups (all classes); returns sd"""
        if self.param_groups is not None:
            sd["param_groups"] = [{"indices": [int(i) for i in g.indices], "lr_scale": float(g.lr_scale.value),
                                   "weight_decay": None if g.weight_decay.value is None else float(g.weight_decay.value)}
                                  for g in self.param_groups]
        return sd

    def _groups_judge(self, sd, name):
        """what _groups_commit takes, from a state dict: None where the dict has no 'param_groups' (this object keeps its values),
        else the checked (lr_scale, weight_decay) of every group.  The dict's groups must be this object's, index for index and
        in this order (ValueError; an object without groups refuses a dict that has them).  Changes nothing."""
        if "param_groups" not in sd:
            return None
        theirs = sd["param_groups"]
        try:
            got = [tuple(int(i) for i in g["indices"]) for g in theirs]
        except (TypeError, KeyError, ValueError):
            raise ValueError("%s: 'param_groups' must be a list of dicts with 'indices', 'lr_scale' and 'weight_decay'" % name)
        mine = None if self.param_groups is None else [g.indices for g in self.param_groups]
        if got != mine:
            raise ValueError("%s: 'param_groups' partitions the parameters as %r in the state dict, %r in this optimizer"
                             % (name, got, mine))
        return [_group_values(name, "'param_groups'[%d]" % j, g.get("lr_scale", 1.0), g.get("weight_decay"))
                for j, g in enumerate(theirs)]

    def _groups_commit(self, values):
        for g, (scale, wd) in zip(self.param_groups or (), values or ()):
            g.lr_scale.assign(scale)
            g.weight_decay.assign(wd)

    def _guard_outcome(self, skipped, undo_vs=None):
        """book-keeping of a guarded step once its decision is known; a skipped finite-difference step takes the perturbation of
        psgd.py:723 back, p <- T(p - v): the reference's own undo, within one rounding of T of the parameters before the step"""
        if undo_vs is not None:
            with torch.no_grad():
                for p, v in zip(self._params, undo_vs):
                    p.sub_(v)
        self.last_step_skipped = bool(skipped)
        self.skipped_steps += int(bool(skipped))
        if self._dynamic_scale:
            S, self._good_steps = uvd_loss_scale_next(self._loss_scale_value(), self._good_steps, skipped,
                                                      growth_interval=self.loss_scale_growth_interval)
            self.loss_scale.assign(S)

    @staticmethod
    def _loss_of(closure_returns):
        return closure_returns if isinstance(closure_returns, torch.Tensor) else closure_returns[0]

    _group = None                        # class UVd(group=...) sets it, and _coins: the generator all ranks share

    def _coin_generator(self):
        """the generator behind the coins (psgd.py:703, :562, :588) and the construction seeds: the generator= argument, else the
        module's branch generator; row-sharded, the synchronised generator all ranks draw from"""
        if self._group is not None:
            return self._coins.gen
        return self._generator if self._generator is not None else _branch_rng

    def _draw_seed(self, explicit):
        """a construction seed (native state, param_rounding, probe): the low 64 bits of `explicit`, or, for None, one draw from
        the generator behind the coin.  The order of these draws is part of the checkpoint contract."""
        if explicit is not None:
            return int(explicit) & (2 ** 64 - 1)
        gen = self._coin_generator()
        return int(torch.randint(0, 2 ** 62, (), generator=gen, device=gen.device).item())

    def _init_fit(self, preconditioner_fit):
        """the preconditioner_fit argument of a constructor, judged before anything touches a device: sets preconditioner_fit,
        _whiten (True for "whitening") and the probe stream's state -- no seed yet (the constructor draws it with _draw_seed, after
        every seed it drew before this switch existed) and the counter at 0"""
        if preconditioner_fit not in _PRECONDITIONER_FITS:
            raise ValueError("%s: preconditioner_fit must be 'hessian' or 'whitening', got %r" % (type(self).__name__, preconditioner_fit))
        self.preconditioner_fit = preconditioner_fit
        self._whiten = preconditioner_fit == "whitening"
        self._probe_seed0, self._probe_step = None, 0

    @property
    def probe_seed0(self):
        """the construction seed of the probe stream (None with preconditioner_fit="hessian")"""
        return self._probe_seed0

    @property
    def probe_step(self):
        """the number of steps that drew a probe so far: the k of uvd_step_rounding_seed(probe_seed0, k) of the next draw"""
        return self._probe_step

    def _next_probe_seed(self):
        """the seed of the probe of an updating whitening step; advances probe_step"""
        seed = uvd_step_rounding_seed(self._probe_seed0, self._probe_step)
        self._probe_step += 1
        return seed

    def _next_param_round_seed(self):
        """the seed of the rounding stream of a step that writes the parameters (param_rounding="stochastic"); advances the counter"""
        seed = uvd_step_rounding_seed(self._param_round_seed0, self._param_round_step)
        self._param_round_step += 1
        return seed

    def _guard_decode(self, sd):
        """restores what _guard_encode saved into a guarded optimizer.  A dict of an unguarded optimizer has none of the keys: the
        guard starts fresh; loss_scale is taken only when both sides scale the loss.  An unguarded optimizer ignores the keys."""
        if not self._guard:
            return
        self.skipped_steps, self.last_step_skipped = int(sd.get("skipped_steps", 0)), False
        self._good_steps = int(sd.get("loss_scale_good_steps", 0))
        if sd.get("loss_scale") is not None and self.loss_scale.value is not None:
            self.loss_scale.assign(float(sd["loss_scale"]))
            self._loss_scale_value()


def _guard_encode(sd, guard, skipped_steps, loss_scale, good_steps):
    """the checkpoint keys of the guard, added to sd when the optimizer is guarded (both classes): nonfinite, skipped_steps,
    loss_scale (the current one; None without loss scaling) and loss_scale_good_steps; returns sd"""
    if guard:
        sd["nonfinite"], sd["skipped_steps"] = "skip", int(skipped_steps)
        sd["loss_scale"] = None if loss_scale is None else float(loss_scale)
        sd["loss_scale_good_steps"] = int(good_steps)
    return sd


def _torch_param_update_(p, g, v, lr, decay, sr_seed, index0):
    """One parameter tensor of the torch tail of either class, in place, one torch op per rounding: delta = T(lr g); v given (the
    undo of the finite-difference perturbation): delta = T(delta + v); decay given (c = fl32(lr_eff wd)): delta = T(delta +
    T(c float(p))); p <- T(p - delta).  For float32 .to(T) and .float() do nothing.  g: float32, in p's shape; lr and decay:
    a pair of _StepFeatures._tail_coefficients (Python floats that hold float32 values, or 0-dim float32 tensors).
    sr_seed not None (param_rounding="stochastic"): param_update_stochastic_ on the flat indices index0, index0 + 1, ..."""
    if sr_seed is not None:                                     # formed once in fp32, narrowed once
        param_update_stochastic_(p, g, v, lr, decay, sr_seed, index0)
        return
    delta = (lr * g).to(p.dtype)
    if v is not None:
        delta = delta + v
    if decay is not None:
        delta = delta + (decay * p.float()).to(p.dtype)
    p.sub_(delta)


def _randn_like(p):
    """The draw of psgd.py:713 / :721 (one place, so that a test can supply the global vector's slices)."""
    return torch.randn_like(p)


def uvd_param_index(params):
    """psgd.py:684-686: sizes and cumulative sizes of the parameters, in list order."""
    sizes = [int(p.numel()) for p in params]
    cumsizes, acc = [], 0
    for s in sizes:
        acc += s
        cumsizes.append(acc)
    return sizes, cumsizes


def _flatten_params(params_with_grad):
    """tf.nest.flatten order (psgd.py:668-669): depth-first through lists/tuples/dicts (dict keys sorted)."""
    if isinstance(params_with_grad, torch.Tensor):
        return [params_with_grad]
    out = []
    if isinstance(params_with_grad, dict):
        for k in sorted(params_with_grad):
            out.extend(_flatten_params(params_with_grad[k]))
    else:
        for p in params_with_grad:
            out.extend(_flatten_params(p))
    return out


def _mixed_dtypes_switch(name, mixed_dtypes):
    """the mixed_dtypes argument of a constructor, judged before anything else: a bool, nothing that merely converts to one"""
    if not isinstance(mixed_dtypes, bool):
        raise ValueError("%s: mixed_dtypes must be True or False, got %r" % (name, mixed_dtypes))
    return mixed_dtypes


def _state_dtype_param(name, mixed, dtype):
    """what state_dtype="param" means: the parameters' dtype; with more than one dtype present it names none (ValueError)"""
    if mixed:
        raise ValueError("%s: state_dtype='param' is ambiguous with parameters of more than one dtype (mixed_dtypes=True); "
                         "name the dtype of the state" % name)
    return dtype


class _FlatStep(_StepFeatures):
    """An optimizer that preconditions ONE flat float32 vector (psgd.py:692-764): everything of its three subclasses -- class UVd,
    class SPLU (splu_optimizer.py) and class Dense (dense_optimizer.py) -- but the preconditioner itself: step(), the flat-vector
    plumbing behind it, the stages of the constructor and the checkpoint pair.
    A row-sharded flat vector (group=) is part of this class: its branches read _group, _coins and _sharded.
    step() stands on what class Kron uses too (_StepFeatures: _step_route, _closure_gradients, _tail_coefficients,
    _fused_tail_kwargs; _init_step_hypers in the constructor); its own are the flat vectors and the guard sequence (_step_grad).

    A subclass's __init__ calls _init_params, _init_hypers, _init_tail and _draw_seeds in this order, its own checks between
    them and every check before _init_tail (the first stage that touches a device), sets _rank, _store_dtype and _state_rounding,
    and provides

        _precondition(v, h, grad)      the flat preconditioned gradient; v and h are None on a step that leaves the state alone
        _flat_region(name, narrow)     where the flat vector `name` lives: "v", "h", "g" of psgd.py:729-730 / :747, "m" the
                                       momentum buffer, "probe" the probe of the whitening fit.  None: it has no home there -- a
                                       step vector is then a fresh tensor, "m" and "probe" are made once by this class (_m, _probe).
                                       narrow: the torch tail asks, for parts that are not float32 yet.  Never None for a step
                                       vector on the fused tail.  Asked at every call, never cached.
        _state_encode(sd, host)        state_dict(): adds the subclass's keys to sd
        _state_judge(sd, name, need, same, **how)    load_state_dict(): judges those keys against this object, changes nothing,
                                       returns what _state_commit takes
        _state_commit(judged)          writes the state; it cannot refuse any more"""

    # ------------------------------------------------------------------------------------------- the stages of a constructor
    def _init_params(self, params_with_grad, generator, param_rounding, preconditioner_fit, mixed_dtypes=False):
        """psgd.py:668-671, :684-686 and the keyword-only switches, judged in this order: mixed_dtypes, the parameters with
        requires_grad (the reference's .trainable) in tf.nest.flatten order, their dtype and device, their index, param_rounding,
        preconditioner_fit.  Returns the number of elements.
        mixed_dtypes=False: params[0].dtype is THE dtype, as in the reference (:671).  True: every tensor is float32, bfloat16 or
        float16 on its own (TypeError otherwise) and _dtypes holds them; _mixed says that more than one is present -- a list of
        one dtype is the optimizer it is with the switch off."""
        name = type(self).__name__
        _mixed_dtypes_switch(name, mixed_dtypes)
        self._params = self._params_with_grad = [p for p in _flatten_params(params_with_grad) if p.requires_grad]   # one list, two names
        self._dtype, self._device, self._generator = self._params[0].dtype, self._params[0].device, generator
        self._dtypes = [p.dtype for p in self._params] if mixed_dtypes else [self._dtype] * len(self._params)
        for dt in self._dtypes:
            if dt not in (torch.float32, torch.float16, torch.bfloat16):
                raise TypeError("%s: parameters must be float32, float16 or bfloat16, got %s" % (name, dt))
        self._mixed = len(set(self._dtypes)) > 1
        self._param_sr = _param_rounding(name, param_rounding, set(self._dtypes) if self._mixed else self._dtype)
        self._param_round_seed0, self._param_round_step = None, 0
        self._round_seed0, self._round_step = None, None        # the stream of a state the kernels round (_draw_seeds)
        self._init_fit(preconditioner_fit)
        self._probe, self._probe_plan = None, None
        self._param_sizes, self._param_cumsizes = uvd_param_index(self._params)
        return self._param_cumsizes[-1]

    def _init_hypers(self, lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                     exact_hessian_vector_product, *features):
        """psgd.py:673-683: the five _Hyper objects (_init_step_hypers); momentum, weight_decay, nonfinite, loss_scale and
        loss_scale_growth_interval (_init_features, which checks them); the tiny of the clip and the finite-difference scale,
        which follow the parameters' dtype"""
        self._init_step_hypers(lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                               exact_hessian_vector_product)
        self._init_features(*features)
        self._stamp = 0
        self._tiny = torch.finfo(self._dtype).tiny                                           # :682
        self._delta_param_scale = torch.finfo(self._dtype).eps ** 0.5                        # :683
        if self._mixed:                                   # the largest of each over the dtypes present, whatever the order
            self._tiny, self._delta_param_scale = mixed_dtype_constants(self._dtypes)
        self._fd_inv_scale = float(np.float32(1.0) / np.float32(self._delta_param_scale))    # what torch's `/ scale` multiplies by

    def _init_tail(self, step_tail):
        """step_tail: "torch" = the tail of step() as torch expressions, a handful of launches per parameter tensor; "fused" =
        the step-tail kernels (uvd_pack, uvd_step_tail) on flat vectors, in a number of launches that does not depend on the
        number of tensors -- the same roundings, so without clipping the same bits.  Parameters that are not contiguous, or not
        of one dtype, keep the torch tail for the life of the object (one warning).  The plan is the first thing a constructor
        puts on the device."""
        if step_tail not in ("torch", "fused"):
            raise ValueError("%s: step_tail must be 'torch' or 'fused', got %r" % (type(self).__name__, step_tail))
        self._tail = None
        if step_tail == "fused":
            if all(p.is_contiguous() and p.dtype == dt for p, dt in zip(self._params, self._dtypes)):
                self._tail = UVdTailPlan(self._param_sizes, self._dtypes if self._mixed else self._dtype, self._device)
                for g in self.param_groups or ():               # the groups' chunk tables: made here, once
                    self._tail.group_chunks(g.indices)
                    if self._mixed:                             # ... and those of the (group, dtype) pairs
                        self._tail.dtype_chunks(g.indices)
            else:
                import warnings
                warnings.warn("%s: step_tail='fused' needs contiguous parameters of one dtype; this optimizer keeps the torch tail"
                              % type(self).__name__)

    def _draw_seeds(self, rounded_state, param_rounding_seed, probe_seed):
        """the construction seeds, from the generator behind the coins, in the order of the checkpoint contract: the state's
        (rounded_state: the kernels round what they store), the parameters', the probe's.  Row-sharded, that generator is the
        synchronised one (_coins is set before this): every rank holds the same seeds."""
        if rounded_state:
            self._round_seed0, self._round_step = self._draw_seed(None), 0
        if self._param_sr:
            self._param_round_seed0 = self._draw_seed(param_rounding_seed)
        if self._whiten:
            self._probe_seed0 = self._draw_seed(probe_seed)

    # ------------------------------------------------------------------------------------------------ the flat vectors of a step

    def _pack_scale(self, fd_scaled, inv):
        """the scale of a pack: 1 / delta_param_scale (:734-736) where fd_scaled, times inv = 1 / loss_scale, rounded once to fp32"""
        base = self._fd_inv_scale if fd_scaled else 1.0
        if inv == 1.0:
            return base
        return float(np.float32(base) * np.float32(inv))

    def _flat(self, tensors, name, fd_scaled=False, inv=1.0, slot=None):
        """psgd.py:729-730, :747: the per-parameter tensors as one flat float32 vector, written where _flat_region says it lives
        (no second copy, and the vector sits where the sweeps read it) -- by one uvd_pack launch on the fused tail, by one
        torch.cat on the torch tail, which makes a fresh tensor where the vector has no home.  fd_scaled (fused tail only): the
        division of :734-736 rides on the pack.  inv: 1 / loss_scale, a power of two, folded into the pack (torch tail: one exact
        multiplication).  slot (guarded step, fused tail): the pack checks what it writes and stamps that word of the plan's
        flags."""
        if self._tail is not None:
            kw = {} if slot is None else dict(flag=self._tail.flags[slot:slot + 1], stamp=self._stamp)
            return uvd_pack([_c(x) for x in tensors], self._flat_region(name), self._pack_scale(fd_scaled, inv), plan=self._tail,
                            role=name, **kw)
        parts = [torch.reshape(x, [-1]) for x in tensors]
        narrow = not all(x.dtype == torch.float32 for x in parts)
        out = self._flat_region(name, narrow)
        if out is None:
            flat = torch.cat(parts, 0).to(torch.float32)
        elif narrow:
            flat = out.copy_(torch.cat(parts, 0))
        else:
            flat = torch.cat(parts, 0, out=out)
        return flat if inv == 1.0 else flat.mul_(inv)

    def _momentum_buffer(self):
        """this rank's flat fp32 momentum vector: where _flat_region places it, else one zero-initialised tensor created on
        first use"""
        m = self._flat_region("m")
        if m is not None:
            return m
        if self._m is None:
            self._m = torch.zeros(self._param_cumsizes[-1], dtype=torch.float32, device=self._device)
        return self._m

    def _grad_flat(self, grads, mom, inv=1.0, flat=None):
        """psgd.py:747; with momentum the gradients blended into the momentum buffer, which is returned in their place.  inv:
        1 / loss_scale, folded into the pack; flat: the flat fp32 gradient where the guarded step has formed it already"""
        if mom == 0.0:
            self._m_step = 0                                  # the buffer is not kept up: a later momentum warms up again
            return flat if flat is not None else self._flat(grads, "g", inv=inv)
        beta, omb = uvd_momentum_coefficients(self._m_step, mom)
        self._m_step += 1
        m = self._momentum_buffer()
        if self._tail is not None:
            return uvd_pack_blend([_c(x) for x in grads], m, beta, self._pack_scale(False, inv), plan=self._tail, role="g")
        g = flat if flat is not None else self._grad_cat(grads, inv)
        with torch.no_grad():
            if beta == 0.0:
                m.copy_(g.mul(omb))                           # the buffer is not read (as in the kernel): NaN in it does not leak
            else:
                m.mul_(beta)
                m.add_(g.mul(omb))
        return m

    def _grad_cat(self, grads, inv):
        g = torch.cat([torch.reshape(x, [-1]) for x in grads], 0).to(torch.float32)
        return g if inv == 1.0 else g * inv

    def _guarded_grad(self, grads, mom, inv, others):
        """The decision of a guarded step, then _grad_flat: the flat gradient (the momentum buffer with momentum), or None when v,
        h (others: checked already by their packs on the fused tail) or the gradient holds a non-finite value -- in which case
        nothing has been written but flat scratch vectors: the momentum blend runs only after the decision.  Row-sharded: every
        rank's verdict crosses the ranks in ONE collective (sharded.all_reduce_max_i32_), issued here on every rank whatever it
        saw, so that all ranks skip or none does.  The single host read of the step is here."""
        flat = None
        if self._tail is not None:
            flags = self._tail.flags
            if mom == 0.0:
                flat = self._flat(grads, "g", inv=inv, slot=2)
            else:               # the blend overwrites the buffer: judge the gradients where they are, blend on a good step only
                uvd_check([_c(x) for x in grads], self._pack_scale(False, inv), plan=self._tail, role="g", flag=flags[2:3],
                          stamp=self._stamp)
            if self._group is None:
                bad = self._stamp in flags.tolist()                                          # the 16 flag bytes: the host read
            else:
                bad = (flags == self._stamp).any()
        else:
            flat = self._flat(grads, "g", inv=inv) if mom == 0.0 else self._grad_cat(grads, inv)
            ok = torch.isfinite(flat).all()
            for x in others:
                ok = ok & torch.isfinite(x).all()
            bad = ~ok
        if self._group is not None:
            bad = self._sharded.all_reduce_max_i32_(bad.to(torch.int32).reshape(1), self._group)
        if not isinstance(bad, bool):
            bad = bool(bad.item())                                                           # ... or this one
        if bad:
            return None
        return self._grad_flat(grads, mom, inv, flat)

    def _step_grad(self, grads, mom, inv, others=(), undo_vs=None):
        """The flat gradient of a step on every route: _grad_flat; guarded, _guarded_grad and the book-keeping of its decision --
        None: the step is skipped (the perturbation undo_vs of a finite-difference step taken back) and the caller returns."""
        if not self._guard:
            return self._grad_flat(grads, mom)                                                # :747
        grad = self._guarded_grad(grads, mom, inv, others)
        self._guard_outcome(grad is None, undo_vs if grad is None else None)
        return grad

    # ------------------------------------------------------------------------------------- preconditioner_fit="whitening"
    def _whitening_inputs(self, grads, mom, inv):
        """(h, g) of an updating whitening step, or (None, None) where the guard skips it: h the raw flat fp32 gradient of this
        step (1 / loss_scale folded into the pack; never the momentum buffer), g what _grad_flat returns.  Without momentum,
        where _flat_region gives the momentum buffer no place, the two hold the same bits: ONE pack, ONE buffer passed for both
        -- every preconditioner call takes v, h and g as const pointers and only reads them.  With momentum, or where the
        momentum buffer has its place (a placed state: its layout was measured with distinct streams), h gets its own region.
        Guarded: the packs judge what they write (h in slot 1, g in slot 2 of the plan's flags); with momentum uvd_check judges
        the gradients before the blend, as on every guarded step.  The decision and its book-keeping are _step_grad's: the one
        host read of the step."""
        if mom == 0.0 and self._flat_region("m") is None:
            g = self._step_grad(grads, mom, inv)
            return g, g
        h = self._flat(grads, "h", inv=inv, slot=1 if self._guard and self._tail is not None else None)
        g = self._step_grad(grads, mom, inv, (h,))
        return (None, None) if g is None else (h, g)

    def _draw_probe(self):
        """v ~ N(0, I) of an updating whitening step, drawn straight into this rank's flat fp32 vector -- where _flat_region places
        it, else a buffer made once; _probe is the vector of the latest draw -- by ONE multi_randn launch over one segment, on
        either step tail: seed uvd_step_rounding_seed(probe_seed0, probe_step), index0 = this rank's first global row, scale 1.
        Advances probe_step."""
        n = self._param_cumsizes[-1]
        if self._probe_plan is None:
            from .multi_tail import MultiTailPlan
            self._probe_plan = MultiTailPlan([n], self._device)
        v = self._flat_region("probe")
        if v is None:
            v = self._probe if self._probe is not None else torch.empty(n, dtype=torch.float32, device=self._device)
        self._probe = v
        multi_randn([v], self._next_probe_seed(), self._row0(), plan=self._probe_plan)
        return v

    def _row0(self):
        """the global index of this rank's first row (row-sharded: one set-up collective the first time)"""
        if self._group is None:
            return 0
        return self._sharded.global_row0(self._param_cumsizes[-1], self._device, self._group)

    def step(self, closure):
        """psgd.py:692-764.

        Guarded (nonfinite="skip"; with the default "propagate" none of this runs: the same launches, the same bits, no host read):
        a step whose flat v, h or g -- as written, scales included -- holds +-Inf or NaN is SKIPPED.  It never reaches the
        preconditioner, the momentum blend or the parameter update: the bits of U, V, d, the parameters and the momentum buffer
        and the counters behind momentum warm-up and stochastic rounding stay as they were; it has consumed the coin of :703 and
        the probe vectors and nothing else.  skipped_steps counts such steps, last_step_skipped tells about the latest, and the
        closure's return value is passed through as always.  On the finite-difference route the perturbation of :723 is taken
        back by p <- T(p - v), the reference's own undo: the parameters are then within one rounding of T of their old values, not
        bit-equal.  A step that leaves the preconditioner alone checks g only.
        With the fused tail the check rides on the packs of h and g (and of v on the finite-difference route:
        psgd_uvd_pack_check_f32 moves the bytes of the plain pack); with momentum the gradients are judged where they are
        (uvd_check) and blended only on a good step.  The decision costs ONE device-to-host read, of the plan's 16 flag bytes: the
        only host read a guarded step adds.  The torch tail decides by torch.isfinite(...).all() on the flat vectors (one read of
        one bool).  Row-sharded, the ranks' verdicts cross in one extra collective per guarded step (a MAX over one int), issued at
        the same point on every rank: all ranks skip or none does.

        loss_scale=S: every gradient this step takes is that of loss * S (the closure is unchanged and returns the unscaled
        loss), so the gradients, the Hessian-vector products and the perturbed gradients are S times larger where they are
        formed, in the parameters' type; 1 / S, exact because S is a power of two, is folded into the pack scale of h and g (on
        the finite-difference route into the product with 1 / delta_param_scale, rounded once on the host), v is not scaled.
        "dynamic": S starts at 2^16, halves on a skipped step and doubles after loss_scale_growth_interval good steps in a row
        (uvd_loss_scale_next).
        Out of scope: a non-finite value that the state itself produces from finite inputs propagates as before, and the
        functional preconditioner calls (update_precond_UVd_math_ and the others) are unchanged.

        preconditioner_fit="whitening" (nothing of this runs with "hessian"): an updating step takes the "whitening" route -- ONE
        closure call and ONE ordinary backward -- and forms h and g from the gradients (_whitening_inputs); the guard, where on,
        sees the gradients only and a skipped step returns before the probe is drawn: probe_step, U, V, d, the parameters, the
        momentum buffer and every counter keep their bits.  Then ONE multi_randn launch fills the flat probe (_draw_probe),
        probe_step advances, and :732-733, :748 run on (v, h, g) = (probe, raw gradient, gradient or momentum buffer).  Nothing is
        undone in the tail: the parameters were never perturbed.  A step whose coin says no update is the path it always was.
        The order of closure calls, backward passes and draws on every route is written down in _StepFeatures._closure_gradients,
        the coefficients (lr_eff, c) of the torch tail with an extension on in _StepFeatures._tail_coefficients."""
        params = self._params_with_grad
        if self._group is None:
            update_Q = _draw_branch(float(self.preconditioner_update_probability), self._generator)   # :703
        else:
            update_Q = self._coins.draw(float(self.preconditioner_update_probability))       # the same coin on every rank
        mom, wd, S, inv, scaled = self._step_scales()
        groups = self._step_groups(wd)                              # None without param_groups: nothing below changes
        guard, fused = self._guard, self._tail is not None
        if guard:
            self._stamp = self._stamp % (2 ** 31 - 1) + 1       # 1 .. 2^31 - 1, then 1 again: the flags are never zeroed
        route = self._step_route(update_Q)
        fd = route == "fd"                                          # the step carries the perturbation of :723 and takes it back
        closure_returns, grads, second, vs = self._closure_gradients(       # :706-727, :737-744; _randn_like: looked up at the call
            closure, route, scaled, lambda p: _randn_like(p), self._delta_param_scale,
            (lambda vs: uvd_step_tail(params, None, 0.0, vs=vs, plan=self._tail)) if fused else None)
        # per route (v, h) and the flat gradient; grad None: the guard skips the step (_step_grad has done the book-keeping)
        if route == "whitening":                                    # (v, h) = (counter-based probe, gradient)
            (h, grad), v = self._whitening_inputs(grads, mom, inv), None        # v: drawn after the decision, below
        elif route is None:                                                                   # :737-744
            v, h, grad = None, None, self._step_grad(grads, mom, inv)
        else:
            Hvs = [pg - g for pg, g in zip(second, grads)] if fd else second                  # :726, in the parameters' dtype
            v = self._flat(vs, "v", fd, slot=0 if guard and fused and fd else None)           # :729
            h = self._flat(Hvs, "h", fd, inv, slot=1 if guard and fused else None)            # :730
            if fd and not fused:                                                              # :734-736
                v = v / self._delta_param_scale
                h = h / self._delta_param_scale
            grad = self._step_grad(grads, mom, inv, (v, h), vs if fd else None)
        if grad is None:
            return closure_returns
        pre_grad = self._precondition(self._draw_probe() if route == "whitening" else v, h, grad)      # :732-733, :747-748
        max_norm = float(self.grad_clip_max_norm)
        sr, sr_seed, sr_index0 = self._param_sr, None, 0
        if sr:                           # this step writes the parameters: the seed of its rounding stream, the GLOBAL first index
            sr_seed = self._next_param_round_seed()
            sr_index0 = int(self._row0()) if self._group is not None else 0
        if fused:                                                                             # :750-762 in the step-tail kernels
            uvd_step_tail(params, pre_grad, float(self.lr_params), max_norm, self._tiny, vs if fd else None,
                          self._group, plan=self._tail, **self._fused_tail_kwargs(groups, wd, sr, sr_seed, sr_index0))
            return closure_returns
        if mom != 0.0 or wd != 0.0 or sr or groups is not None or self._mixed:      # the torch tail of the extensions: the kernels' rule
            sumsq = None
            if not math.isinf(max_norm):
                sq = torch.sum((pre_grad * pre_grad).double()).reshape(1)
                if self._group is not None:
                    self._sharded.all_reduce_sum_f64_(sq, self._group)
                sumsq = sq[0]
            coef = self._tail_coefficients(float(self.lr_params), wd, groups, max_norm, sumsq, self._tiny, len(params))
        else:
            # every extension off: the reference's own expressions, NOT _tail_coefficients -- psgd.py:750-754 forms the norm and the
            # learning rate in float32, which gives other bits than the kernels' rule (fp64 sum, one rounding), by design
            if math.isinf(max_norm):                                                          # :750-751
                lr = float(self.lr_params)
            else:                                                                             # :753-754
                if self._group is None:
                    grad_norm = torch.sqrt(torch.sum(pre_grad * pre_grad)) + self._tiny
                else:                              # the norm of the GLOBAL vector: one scalar all-reduce, no host read
                    grad_norm = self._sharded.global_norm(pre_grad, self._group) + self._tiny
                lr = float(self.lr_params) * torch.clamp(max_norm / grad_norm, max=1.0)
            coef = [(lr, None)] * len(params)
        with torch.no_grad():                                                                 # :757-762
            for k, (p, i, j) in enumerate(zip(params, self._param_sizes, self._param_cumsizes)):
                _torch_param_update_(p, torch.reshape(pre_grad[j - i:j], p.shape), vs[k] if fd else None, *coef[k],
                                     sr_seed if p.dtype == torch.bfloat16 else None, sr_index0 + j - i)
        return closure_returns                                                              # :764

    # ------------------------------------------------------------------------------------------------- checkpoint / resume
    def state_dict(self):
        """Everything a bit-faithful resume needs, as a flat dict of CPU tensors and plain Python values (safe for torch.save /
        torch.load(weights_only=True)); the subclass documents its own keys and adds them in _state_encode:

            format                   1
            rank, num_params         the rank r and this rank's row count
            param_sizes              the element counts of this rank's parameter tensors
            state_dtype, state_rounding    strings ("torch.bfloat16"; "stochastic" / "nearest" / "none")
            round_seed0, round_step  a state the kernels round only: together they fix every stored code of every later step
            param_round_seed0, param_round_step    param_rounding="stochastic" only: the seed and the step counter of the
                                     parameters' rounding stream (param_rounding itself is a constructor choice and is not saved)
            probe_seed0, probe_step  preconditioner_fit="whitening" only: the seed and the step counter of the probe stream, the
                                     same on every rank (preconditioner_fit itself is a constructor choice and is not saved)
            hyper                    lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability (floats),
                                     exact_hessian_vector_product (bool)
                                     and, optional when loading, momentum and weight_decay (floats)
            momentum_buffer, momentum_step    only when momentum > 0: this rank's rows of the momentum buffer (fp32) and the number of
                                     steps blended into it
            nonfinite, skipped_steps, loss_scale, loss_scale_good_steps    only when nonfinite="skip": "skip", the number of
                                     skipped steps, the current loss scale (None without loss scaling) and the good steps
                                     counted towards the next growth of a dynamic scale
            branch_rng               get_state() of the generator behind the coin flips: the generator= argument, else the
                                     module's branch generator; row-sharded, the synchronised generator all ranks draw from
            param_groups             only when the constructor was given param_groups: [{"indices": [...], "lr_scale": float,
                                     "weight_decay": float or None}, ...], the groups of opt.param_groups in order

        NOT saved: the parameters (they are the caller's), and the global CUDA generator that draws the probe vectors of
        :713 / :721 -- it belongs to the caller; save torch.cuda.get_rng_state() next to this dict and restore it with
        torch.cuda.set_rng_state() where the resumed run must draw the same vectors."""
        def host(t):
            return t.detach().to("cpu", copy=True).contiguous()
        sd = {"format": 1, "rank": self._rank, "num_params": self._param_cumsizes[-1],
              "param_sizes": [int(s) for s in self._param_sizes], "state_dtype": str(self._store_dtype),
              "state_rounding": self._state_rounding if self._state_rounding is not None else "none",
              "hyper": {k: (bool if k == "exact_hessian_vector_product" else float)(getattr(self, k)) for k in self._HYPER_KEYS},
              "branch_rng": self._coin_generator().get_state().clone()}
        self._state_encode(sd, host)
        sd["hyper"]["momentum"], sd["hyper"]["weight_decay"] = float(self.momentum), float(self.weight_decay)
        if float(self.momentum) > 0.0:
            sd["momentum_buffer"], sd["momentum_step"] = host(self._momentum_buffer()), int(self._m_step)
        if self._round_seed0 is not None:
            sd["round_seed0"], sd["round_step"] = int(self._round_seed0), int(self._round_step)
        _param_rounding_encode(sd, self._param_sr, self._param_round_seed0, self._param_round_step)
        _probe_encode(sd, self._whiten, self._probe_seed0, self._probe_step)
        self._groups_encode(sd)
        return _guard_encode(sd, self._guard, self.skipped_steps, self.loss_scale.value, self._good_steps)

    def load_state_dict(self, sd, **how):
        """Restore what state_dict() saved, IN PLACE: the state is written into the tensors this object already holds, the
        hyper-parameters are assigned (momentum and weight_decay when the dict has them; momentum_buffer / momentum_step are
        restored, and a dict without them zeroes the buffer of a momentum optimizer and restarts its warm-up), the generator
        behind the coins gets the saved state (row-sharded: every rank loads the same bytes into the synchronised generator;
        nothing is broadcast again) and so do, where this object has the switch on and the dict has the keys, round_seed0 /
        round_step, param_round_seed0 / param_round_step and probe_seed0 / probe_step; a dict without the keys of a switch this
        object has on leaves its seed and starts the counter at 0, and an object with the switch off ignores them.  A guarded
        optimizer (nonfinite="skip") restores skipped_steps, loss_scale_good_steps and, when both sides scale the loss,
        loss_scale where the dict has them and starts them fresh where it has not; an unguarded one ignores them.
        param_groups: a dict without the key leaves the groups' lr_scale and weight_decay as they are; with the key, the dict's
        groups must be this object's index for index (ValueError otherwise, also for an object built without groups) and their
        values are assigned.

        Checked against this object (ValueError naming the key): format, rank, num_params, param_sizes (skipped when the dict
        holds None, as a resharded one does), then the subclass's keys (_state_judge; **how are its keywords).  Everything that can
        refuse the dict is judged before anything of this object changes: a dict that is refused leaves this object as it was.
        The parameters and the global CUDA generator are the caller's."""
        name = type(self).__name__ + ".load_state_dict"

        def need(key):
            if key not in sd:
                raise ValueError("%s: the state dict has no %r" % (name, key))
            return sd[key]

        def same(key, mine):
            got = need(key)
            if got != mine:
                raise ValueError("%s: %r is %r in the state dict, %r in this optimizer" % (name, key, got, mine))
        if need("format") != 1:
            raise ValueError("%s: 'format' is %r; this version reads format 1" % (name, sd["format"]))
        n = self._param_cumsizes[-1]
        same("rank", self._rank)
        same("num_params", n)
        if need("param_sizes") is not None and [int(s) for s in sd["param_sizes"]] != [int(s) for s in self._param_sizes]:
            raise ValueError("%s: 'param_sizes' is %r in the state dict, %r in this optimizer"
                             % (name, list(sd["param_sizes"]), list(self._param_sizes)))
        judged = self._state_judge(sd, name, need, same, **how)
        hyper = need("hyper")
        for k in self._HYPER_KEYS:
            if k not in hyper:
                raise ValueError("%s: 'hyper' has no %r" % (name, k))
        mbuf = sd.get("momentum_buffer")
        if mbuf is not None and (not isinstance(mbuf, torch.Tensor) or mbuf.dtype != torch.float32 or mbuf.numel() != n):
            raise ValueError("%s: 'momentum_buffer' must be a float32 tensor of %d elements" % (name, n))
        if mbuf is not None:
            need("momentum_step")
        gen = self._coin_generator()
        try:                                                     # tried on a scratch generator: this object's is not touched yet
            torch.Generator(device=gen.device).set_state(need("branch_rng"))
        except (RuntimeError, TypeError) as e:
            raise ValueError("%s: 'branch_rng' does not fit this optimizer's generator: %s" % (name, e))
        rounded = self._round_seed0 is not None and "round_seed0" in sd
        if rounded:
            need("round_step")
        param_round = _param_rounding_decode(name, sd, self._param_sr, self._param_round_seed0)
        probe = _probe_decode(sd, self._whiten, self._probe_seed0, name)
        if self._guard and sd.get("loss_scale") is not None and self.loss_scale.value is not None:
            S = float(sd["loss_scale"])
            if not (S > 0.0 and math.isfinite(S) and math.frexp(S)[0] == 0.5):
                raise ValueError("%s: 'loss_scale' must be a power of two, got %r" % (name, sd["loss_scale"]))
        group_values = self._groups_judge(sd, name)
        # ---- nothing below refuses the dict
        gen.set_state(sd["branch_rng"])
        self._groups_commit(group_values)
        for k in self._HYPER_KEYS + tuple(k for k in ("momentum", "weight_decay") if k in hyper):   # (the two: optional in a dict)
            getattr(self, k).assign(hyper[k])
        with torch.no_grad():
            if mbuf is not None:
                self._momentum_buffer().copy_(mbuf.reshape(-1))
                self._m_step = int(sd["momentum_step"])
            else:                                                # no buffer saved: a momentum optimizer starts its warm-up again
                self._m_step = 0
                if float(self.momentum) > 0.0:
                    self._momentum_buffer().zero_()
        if rounded:
            self._round_seed0, self._round_step = int(sd["round_seed0"]), int(sd["round_step"])
        (self._param_round_seed0, self._param_round_step), (self._probe_seed0, self._probe_step) = param_round, probe
        self._guard_decode(sd)
        with torch.no_grad():
            self._state_commit(judged)


class UVd(_FlatStep):
    """Low-rank modification (UVd) preconditioner as an optimizer, psgd.py:630-764: _FlatStep (step(), the flat vectors, the
    checkpoint skeleton) with the state U, V, d -- plain tensors, a bfloat16 state the kernels read and write, regions of a
    placement.UVdArena, or this rank's rows of a row-sharded state.

    Same constructor arguments and defaults as the reference (psgd.py:663-666).  Parameters are
    torch tensors with requires_grad=True on a ROCm device (the reference's `.trainable` filter,
    :670, maps to requires_grad).  `step(closure)` returns whatever closure returns (:764).

    param_rounding="stochastic" (extension, keyword-only; "nearest" by default: nothing changes; bfloat16 parameters only, anything
    else is a ValueError before a device is touched).  There is no float32 master copy: the parameter is the bfloat16 tensor, and
    under round to nearest a weight ignores every update below half its spacing.  With "stochastic" the update of :757-762 is
    formed once in float32 and narrowed once with the stochastic rounding of the bf16-stored states -- w = float(p),
    d = fl32(lr_eff g), d = fl32(d + float(v)), d = fl32(d + fl32(c w)), p <- SR(fl32(w - d)) -- on a stream keyed by
    uvd_step_rounding_seed(seed0, k) and the element's global flat index (psgd_uvd_param_update_multi_sr on the fused tail,
    param_update_stochastic_ on the torch tail: the same bits).  seed0: param_rounding_seed, or a draw from the generator behind
    the coins; k counts the steps that wrote the parameters.  The perturbation of :723 and its undo stay round-to-nearest.
    state_dict() carries param_round_seed0 / param_round_step; param_rounding itself is a constructor choice, like step_tail.

    preconditioner_fit="whitening" (extension, keyword-only; "hessian" by default: nothing changes, no new function is called, no
    new number is drawn; any other value is a ValueError before a device is touched) fits the preconditioner to the GRADIENTS
    instead of to Hessian-vector products: the update of :732-733 is fed the pair (v, h) = (probe, g), v ~ N(0, I) drawn fresh on
    every updating step and g the raw flat float32 gradient of this step (1 / loss_scale folded into its pack; never the momentum
    buffer).  The criterion E[h' P h + v' P^-1 v] is then minimised by P = Q'Q = (E[g g'])^(-1/2) within the UVd form: the
    preconditioner whitens the gradient (the gradient-whitening fit of the PSGD papers).  A step needs ONE ordinary
    backward pass: no create_graph, no second closure call, no perturbation of the parameters -- so closures whose backward cannot
    be differentiated again (fused attention kernels, custom Functions marked once_differentiable) train, and the step no longer
    pays the second backward.  exact_hessian_vector_product is ignored on this route (nothing is rejected).  The probe is this
    rank's flat float32 vector -- the arena's v region on a placed state, else a buffer made once -- filled by ONE multi_randn
    launch over one segment on BOTH step tails (there is no torch.randn on this route, no per-tensor probe, and v is never
    packed): the stream of updating step k is keyed by uvd_step_rounding_seed(probe_seed0, k) and the element's GLOBAL flat index
    (index0 = this rank's first row), whatever `generator` is, so a row-sharded run draws the rows of the one-process probe;
    probe_seed0 = probe_seed, or a draw from the generator behind the coins (after the draws of the native state's and the
    parameters' seeds where those happen; row-sharded, from the synchronised generator: the same on every rank); k = probe_step
    counts the steps that drew a probe.  Without momentum, on a state that is not placed, h and g are one buffer, packed once (the
    kernels only read them); with momentum or a placed state each has its own.  The probe is finite by construction and is not
    judged by the guard; a skipped step returns before it is drawn and leaves probe_step alone.  state_dict() carries probe_seed0
    / probe_step; preconditioner_fit itself is a constructor choice, like step_tail.  The whitened gradient has roughly unit scale
    per element, as Adam's update has: lr_params and grad_clip_max_norm tuned for the Hessian fit do NOT carry over.

    mixed_dtypes=True (extension, keyword-only; False by default: nothing changes, params[0].dtype is THE dtype; anything but a
    bool is a ValueError before a device is touched) takes parameter tensors that are float32, bfloat16 or float16 each, on both
    step tails; a list of one dtype behaves bit for bit as with False.  Each tensor is treated exactly as in a one-dtype optimizer
    of its own dtype given the same float32 preconditioned gradient: the packs widen it from its own dtype, its update is rounded
    once in its dtype, the undo of a skipped finite-difference step too.  tiny (:682) and delta_param_scale (:683) are the LARGEST
    finfo(T).tiny and finfo(T).eps ** 0.5 over the dtypes present (mixed_dtype_constants; one perturbation scale, since :716-727
    perturbs all parameters jointly), whatever the order of the list.  param_rounding="stochastic" rounds the bfloat16 tensors,
    on the stream keyed by the index in the FULL flat order, and updates the float32 ones as under "nearest"; a float16 tensor or
    no bfloat16 tensor is a ValueError.  state_dtype="param" is then ambiguous: ValueError.  Fused tail: every typed launch runs
    once per dtype present over that dtype's sub-plan of the chunk table (UVdTailPlan.dtype_chunks), crossed with param_groups
    once per (group, dtype) pair that has tensors -- (typed roles x D) + sums + pairs launches, D <= 3 (tail_launch_count) --
    with the one-dtype segment tables and uploads; the guard's flag word is shared by the launches of a role.  A constructor
    choice like step_tail: not in state_dict(), which carries no parameter dtype."""

    def __init__(self, params_with_grad, rank_of_modification: int = 10, preconditioner_init_scale=1.0,
                 lr_params=0.01, lr_preconditioner=0.01,
                 grad_clip_max_norm=None, preconditioner_update_probability=1.0,
                 exact_hessian_vector_product: bool = True, generator=None, state_dtype=None, group=None,
                 stage_backend=None, placement="auto", state_route="widen", state_rounding=None, step_tail="torch",
                 momentum=0.0, weight_decay=0.0, nonfinite="propagate", loss_scale=None, loss_scale_growth_interval=2000,
                 *, param_rounding="nearest", param_rounding_seed=None, preconditioner_fit="hessian", probe_seed=None,
                 param_groups=None, mixed_dtypes=False):
        # group (extension): a torch.distributed process group (dist.group.WORLD for the default one) makes this a
        # ROW-SHARDED optimizer: `params_with_grad` are THIS rank's parameters, the global flat vector of psgd.py:729-730 is the
        # concatenation of the ranks' vectors in rank order, and U, V, d hold this rank's rows only.  A step then costs three
        # collectives: the two exchanges of sharded.update_precond_UVd_math_and_precond_grad (r-dimensional sums, never N-sized
        # data) and one scalar all-reduce for the clip norm of :753 (none without clipping); the coins of :703, :562, :588 come
        # from one generator whose state rank 0 broadcasts once.  The closure returns this rank's loss; its gradient and
        # Hessian-vector product with respect to this rank's parameters are what a model-parallel closure computes.
        # Every check comes before anything is drawn from a generator or touches a device (_FlatStep._init_tail is the first that
        # does).  param_rounding and preconditioner_fit: the class docstring.
        num_params = self._init_params(params_with_grad, generator, param_rounding, preconditioner_fit, mixed_dtypes)  # :668-671, :684-686
        # psgd.py:657-658 allows half-precision parameters.  The preconditioner state U, V, d and all of its arithmetic
        # stay fp32 here (mixed precision: the HIP kernels compute in fp32; v, Hv and the gradient are widened on the
        # way in, the preconditioned gradient is narrowed on the way out).  _tiny and the finite-difference scale follow
        # the parameter dtype as in the reference (:682-683).
        # state_dtype (extension; default None = fp32): "param" or a torch dtype STORES U, V, d in that type, as the reference does
        # for half-precision parameters (psgd.py:688-690) -- every step widens them, runs the fp32 kernels and rounds the updated
        # state back, so the memory held between steps and the rounding of the state once per step are the reference's; its
        # arithmetic (every TF op in the parameters' type) is not reproduced.
        self._store_dtype = torch.float32 if state_dtype is None else \
            _state_dtype_param("UVd", self._mixed, self._dtype) if state_dtype == "param" else state_dtype
        if self._store_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError("UVd: state_dtype must be None, 'param', float32, float16 or bfloat16, got %r" % (state_dtype,))
        r = self._rank = int(rank_of_modification)
        if r < 1:
            raise ValueError("UVd: rank_of_modification must be >= 1, got %d" % r)
        # state_route (extension): "widen" (default) = the behaviour above for a narrow state_dtype; "native" = a bfloat16 state is
        # read and written by the bf16-state kernels themselves (psgd_uvd_bf16.hip): no fp32 copies of U, V, d exist at any time.
        # state_rounding: how those kernels narrow what they write, "stochastic" (default of the native route: under round to
        # nearest a bf16 d practically stops learning, its increments are below half a spacing) or "nearest".  The seed of step k
        # is a hash of one seed fixed here (drawn from `generator` when given, the module's branch generator otherwise) and k
        # (uvd_step_rounding_seed).
        if state_route not in ("widen", "native"):
            raise ValueError("UVd: state_route must be 'widen' or 'native', got %r" % (state_route,))
        self._native = state_route == "native"
        if self._native:
            if self._store_dtype != torch.bfloat16:
                raise ValueError("UVd: state_route='native' needs a bfloat16 state (state_dtype=torch.bfloat16, or 'param' with "
                                 "bfloat16 parameters), got %s" % (self._store_dtype,))
            if r > _lib.UVD_MAX_RANK:
                raise ValueError("UVd: state_route='native' supports ranks up to %d, got %d" % (_lib.UVD_MAX_RANK, r))
            # row-sharded (group=): this rank's rows in bf16, the staged bf16 kernels of sharded.py -- 4 exchanges per step.  The
            # bf16 stages exist in the HIP backend only, and the group must be a real process group.
            if stage_backend is not None:
                raise ValueError("UVd: state_route='native' runs the HIP stages of its group= only (stage_backend= is not supported)")
            if group is not None:
                import torch.distributed as _dist
                if not (_dist.is_available() and isinstance(group, _dist.ProcessGroup)):
                    raise ValueError("UVd: state_route='native' needs group= to be a torch.distributed process group, got %r"
                                     % (type(group),))
            state_rounding = "stochastic" if state_rounding is None else state_rounding
            if state_rounding not in _ROUNDINGS:
                raise ValueError("UVd: state_rounding must be 'stochastic' or 'nearest', got %r" % (state_rounding,))
        elif state_rounding is not None:
            raise ValueError("UVd: state_rounding applies to state_route='native' only")
        self._state_rounding = state_rounding
        # momentum, weight_decay (extensions, off by default; _Hyper objects like the others).  momentum: the flat gradient of :747
        # is blended into a buffer m that this object keeps, m <- beta_k m + (1 - beta_k) g with beta_k = min(k / (k + 1), momentum)
        # (the warm-up of the PyTorch PSGD optimizers; k counts the steps blended so far, and a step taken with momentum == 0 sets
        # it back to 0), and m takes the place of g in :748 -- v, h, the finite-difference undo and the clip norm (now of P m) are
        # as before.  m is this rank's flat fp32 vector: the arena's g region when the state is placed, one tensor otherwise; with
        # the fused tail the blend rides on the pack of g (uvd_pack_blend: no flat g exists).  weight_decay (decoupled): the update
        # of :757-762 gains delta <- T(delta + T(fl32(fl32(lr_eff wd) p))).  Both tails round alike (every operation on its own);
        # with either one on, the torch tail forms the clipped lr as the kernel does (fp64 from the fp32 squares, one rounding).
        # nonfinite, loss_scale, loss_scale_growth_interval (extensions, off by default; see step()): "skip" = a step whose v, h or
        # g holds a non-finite value changes nothing.
        self._init_hypers(lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                          exact_hessian_vector_product, momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval)
        # placement (extension): "probe" / "packed" carve U, V, d, the workspace, the output and the flat v / h / g vectors of :729-730,
        # :747 out of allocations owned by this object (placement.UVdArena; "probe" times candidate layouts once and keeps the
        # fastest: where the WRITTEN streams sit relative to the read ones is worth 5 %); None = plain allocations; "auto" (default)
        # = "probe" when a factor is at least 1 GiB (the search costs ~0.6 s and allocates up to ~100 GiB while it runs; smaller
        # states are close to cache-resident and gain little), None below
        if placement not in (None, "auto", "probe", "packed"):
            raise ValueError("UVd: placement must be None, 'auto', 'probe' or 'packed', got %r" % (placement,))
        if placement == "auto":
            placement = "probe" if 4 * num_params * r >= (1 << 30) else None
        # param_groups (extension, keyword-only; None by default: nothing changes): a learning-rate scale and a weight decay per
        # group of parameter tensors (_StepFeatures._init_groups); row-sharded, of this rank's tensors
        self._init_groups(param_groups)
        self._init_tail(step_tail)                              # (on the fused tail the flat vectors are this object's, or the arena's)
        # group (extension): a torch.distributed process group (dist.group.WORLD for the default one) makes this a
        # ROW-SHARDED optimizer: `params_with_grad` are THIS rank's parameters, the global flat vector of psgd.py:729-730 is the
        # concatenation of the ranks' vectors in rank order, and U, V, d hold this rank's rows only.  A step then costs three
        # collectives: the two exchanges of sharded.update_precond_UVd_math_and_precond_grad (r-dimensional sums, never N-sized
        # data) and one scalar all-reduce for the clip norm of :753 (none without clipping); the coins of :703, :562, :588 come
        # from one generator whose state rank 0 broadcasts once.  The closure returns this rank's loss; its gradient and
        # Hessian-vector product with respect to this rank's parameters are what a model-parallel closure computes.
        self._group, self._stage_backend, self._num_params_global = group, stage_backend, num_params
        if group is not None:       # the generator whose state rank 0 broadcasts, once, here: the coins and one seed for all ranks
            from . import sharded as _sharded
            self._sharded = _sharded
            self._coins = _sharded.branch_rng_for(generator, group, self._device)
            self._num_params_global = _sharded.global_rows(num_params, self._device, group)  # :686 over all ranks (set-up time)
        self._draw_seeds(self._native, param_rounding_seed, probe_seed)
        uv_scale = (1.0 / (self._num_params_global * r)) ** 0.5                              # :687 (the GLOBAL N)
        self._arena, self._flat_bufs = None, {}
        if placement is not None and self._device.type == "cuda" and self._store_dtype == torch.float32 \
                and r <= _lib.UVD_MAX_RANK and stage_backend is None:
            from . import placement as _placement
            self._arena = (_placement.UVdArena.probe if placement == "probe" else _placement.UVdArena.packed)(
                num_params, r, self._device)
        # the keywords of the two calls of step() (_precondition) that never change
        out = None if self._arena is None else self._arena.out
        self._apply_kw = dict(group=group, backend=stage_backend) if group is not None else dict(out=out)
        self._update_kw = dict(self._apply_kw, out=out, generator=generator, rounding=state_rounding or "nearest")
        if self._arena is not None:
            self._arena.install_workspace()
            self._U, self._V, self._d = self._arena.U, self._arena.V, self._arena.d
            self._U.normal_().mul_(uv_scale)                                                 # :688
            self._V.normal_().mul_(uv_scale)                                                 # :689
            self._d.fill_(float(preconditioner_init_scale))                                  # :690
            return
        self._U = torch.randn(num_params, r, dtype=torch.float32, device=self._device) * uv_scale       # :688
        self._V = torch.randn(num_params, r, dtype=torch.float32, device=self._device) * uv_scale       # :689
        self._d = torch.ones(num_params, 1, dtype=torch.float32, device=self._device) * preconditioner_init_scale  # :690
        if self._store_dtype != torch.float32:
            self._U, self._V, self._d = (x.to(self._store_dtype) for x in (self._U, self._V, self._d))

    def _state_fp32(self):
        """the state the kernels work on: the stored tensors themselves (fp32, or bf16 on the native route), or fp32 copies of a
        half-precision state"""
        if self._store_dtype == torch.float32 or self._native:
            return self._U, self._V, self._d
        return self._U.float(), self._V.float(), self._d.float()

    def _state_store(self, U, V, d):
        if self._store_dtype != torch.float32 and not self._native:
            self._U.copy_(U)
            self._V.copy_(V)
            self._d.copy_(d)

    def _flat_region(self, name, narrow=False):
        """_FlatStep's question.  A placed state: the arena's region ("m" is its g region, "probe" its v region) -- on the torch
        tail only for parts that are float32 already (narrow ones are concatenated and widened into a fresh tensor, as without an
        arena).  No arena: on the fused tail a buffer for v, h or g made on first use; nothing on the torch tail, and nothing for
        the momentum buffer and the probe, which _FlatStep then makes once."""
        if self._arena is not None:
            return None if narrow else getattr(self._arena, {"m": "g", "probe": "v"}.get(name, name)).view(-1)
        if self._tail is None or name in ("m", "probe"):
            return None
        if name not in self._flat_bufs:
            self._flat_bufs[name] = torch.empty(self._tail.total, dtype=torch.float32, device=self._device)
        return self._flat_bufs[name]

    # ------------------------------------------------------------------------------------------------- checkpoint / resume
    def _state_encode(self, sd, host):
        """state_dict() of _FlatStep with these keys besides:

            U, V, d                  this rank's rows in the STORED dtype (clones on the CPU, never views of an arena)
            row0, num_params_global  the global index of this rank's first row (unsharded: 0) and the rows of the global vector
            state_route              "native" / "widen"

        Row-sharded: every rank calls it (row0 is one set-up collective the first time, sharded.global_row0) and saves its own dict."""
        sd.update(U=host(self._U), V=host(self._V), d=host(self._d), num_params_global=int(self._num_params_global),
                  row0=int(self._row0()), state_route="native" if self._native else "widen")

    def load_state_dict(self, sd, *, strict=True, narrow_rounding=None, narrow_seed=None):
        """_FlatStep.load_state_dict: U, V, d are written into the tensors this object already holds (a placed state stays in
        its arena; every pointer the tail plan and the workspaces cache stays valid), and a dict that is refused, on whatever
        key, leaves this object as it was.

        Checked besides the common keys: with strict=True num_params_global and row0.  strict=False is for loading a slice of a
        global state into an object that does not know where its rows sit (rows of a resharded checkpoint).

        Dtypes: the same stored dtype is a bitwise copy; a bfloat16 checkpoint into a float32 state widens exactly; a float32
        checkpoint into a NATIVE bfloat16 state is streamed -- host -> pinned staging -> device staging (64 MiB at most, the only
        fp32 image of the state that ever exists on the device) -> psgd_uvd_bf16_narrow_f32 -- with narrow_rounding (default: this
        object's state_rounding) and narrow_seed (default: uvd_step_rounding_seed(round_seed0, 2**40 + round_step), a stream
        disjoint from every step's); the rounding index is the GLOBAL element index (from the dict's row0), so the codes depend
        on neither the chunking nor the row split.  Such a checkpoint carries no round_seed0 / round_step: the object keeps
        its own.  Any other pair of dtypes raises TypeError."""
        super().load_state_dict(sd, strict=strict, narrow_rounding=narrow_rounding, narrow_seed=narrow_seed)

    def _state_judge(self, sd, name, need, same, strict, narrow_rounding, narrow_seed):
        if narrow_rounding is not None and narrow_rounding not in _ROUNDINGS:
            raise ValueError("%s: narrow_rounding must be 'stochastic' or 'nearest', got %r" % (name, narrow_rounding))
        if strict:
            same("num_params_global", int(self._num_params_global))
            same("row0", int(self._row0()))
        row0 = int(need("row0"))
        src = {k: need(k) for k in ("U", "V", "d")}
        for k, mine in (("U", self._U), ("V", self._V), ("d", self._d)):
            if not isinstance(src[k], torch.Tensor) or tuple(src[k].shape) != tuple(mine.shape):
                raise ValueError("%s: %r must be a tensor of shape %s" % (name, k, tuple(mine.shape)))
        have = {src[k].dtype for k in src}
        if len(have) != 1:
            raise TypeError("%s: U, V and d of the state dict have different dtypes %s" % (name, sorted(str(x) for x in have)))
        have = have.pop()
        if have == self._store_dtype or (have == torch.bfloat16 and self._store_dtype == torch.float32):
            return src, None                               # a copy (exact: every bfloat16 value is a float32 value)
        if not (have == torch.float32 and self._native):
            raise TypeError("%s: a %s checkpoint cannot be loaded into a %s state (state_route=%r): the same dtype, bfloat16 into "
                            "float32 and float32 into a native bfloat16 state are supported"
                            % (name, have, self._store_dtype, "native" if self._native else "widen"))
        if not all(t.is_contiguous() for t in (self._U, self._V, self._d)):
            raise ValueError("UVd.load_state_dict: the native state must be contiguous")
        return src, (row0, narrow_rounding if narrow_rounding is not None else self._state_rounding,
                     None if narrow_seed is None else int(narrow_seed))

    def _state_commit(self, judged):
        src, narrow = judged
        if narrow is None:
            for k, mine in (("U", self._U), ("V", self._V), ("d", self._d)):
                mine.copy_(src[k])
            return
        row0, rounding, seed = narrow                      # (the default seed: from round_seed0 / round_step as just restored)
        if seed is None:
            seed = uvd_step_rounding_seed(self._round_seed0, 2 ** 40 + self._round_step)
        self._load_narrowed(src, row0, self._rank, rounding, seed)

    def _load_narrowed(self, src, row0, r, rounding, seed):
        """fp32 host tensors -> this object's native bf16 state, through ONE pinned and ONE device staging buffer of at most
        _NARROW_STAGING_BYTES (reused chunk after chunk: the stream is drained before a buffer is refilled)"""
        chunk = max(1, int(_NARROW_STAGING_BYTES) // 4)
        cap = min(chunk, max(int(t.numel()) for t in src.values()))
        pinned = torch.empty(cap, dtype=torch.float32, pin_memory=True)
        staged = torch.empty(cap, dtype=torch.float32, device=self._device)
        stream = torch.cuda.current_stream(self._device)
        for k, mine, index0 in (("U", self._U, row0 * r), ("V", self._V, row0 * r), ("d", self._d, row0)):
            flat, host = mine.view(-1), src[k].detach().contiguous().view(-1)
            for lo in range(0, int(host.numel()), chunk):
                m = min(chunk, int(host.numel()) - lo)
                pinned[:m].copy_(host[lo:lo + m])
                staged[:m].copy_(pinned[:m], non_blocking=True)
                uvd_bf16_narrow_(flat[lo:lo + m], staged[:m], tensor=k, index0=index0 + lo, rounding=rounding, rounding_seed=seed)
                stream.synchronize()

    def _precondition(self, v, h, grad):
        """psgd.py:748 on the flat gradient; with v and h (None on a step that leaves the preconditioner alone) after :732-733,
        as one fused call: the same results in three sweeps instead of six.  Row-sharded: this rank's rows, 2 exchanges (4 for
        a native bf16 state), :562 and :588 from the synchronised generator.  A native state gets the rounding seed of this step."""
        U, V, d = self._state_fp32()
        g = grad[:, None].contiguous()
        if self._group is not None:          # (looked up at the call, as a global is: a spy on the module attribute sees the call)
            apply, fused = self._sharded.precond_grad_UVd_math, self._sharded.update_precond_UVd_math_and_precond_grad
        else:
            apply, fused = precond_grad_UVd_math, update_precond_UVd_math_and_precond_grad
        if v is None:
            return apply(U, V, d, g, **self._apply_kw)
        seed = None
        if self._native:
            seed = uvd_step_rounding_seed(self._round_seed0, self._round_step)
            self._round_step += 1
        pre_grad = fused(U, V, d, v[:, None].contiguous(), h[:, None].contiguous(), g, step=float(self.lr_preconditioner),
                         tiny=self._tiny, rounding_seed=seed, **self._update_kw)
        self._state_store(U, V, d)
        return pre_grad


# --------------------------------------------------------------------------- Kron optimizer (kron_optimizer.py, multi_tail.py)
# (imported last: those modules build on the step-tail plan, _Hyper, _StepFeatures and the Kron entry points above; the multi_*
# functions live in multi_tail.py and come through kron_optimizer, which imports them by name)
from .kron_optimizer import Kron, multi_sumsq, multi_param_update, multi_diff_scale, kron_initial_factors  # noqa: E402,F401
from .kron_optimizer import multi_blend, multi_scale_check, multi_widen_check  # noqa: E402,F401
from .kron_optimizer import multi_vec_precond_update, multi_vec_precond_grad, kron_layers  # noqa: E402,F401
from .kron_optimizer import multi_narrow, kron_operand_layers  # noqa: E402,F401
from .kron_optimizer import multi_randn  # noqa: E402,F401

# --------------------------------------------------------------------------- sparse-LU optimizer (splu_optimizer.py)
# (after _FlatStep, its base class)
from .splu_optimizer import SPLU, splu_initial_factors  # noqa: E402,F401

# --------------------------------------------------------------------------- dense optimizer (dense_optimizer.py)
from .dense_optimizer import Dense, dense_initial_factor  # noqa: E402,F401
