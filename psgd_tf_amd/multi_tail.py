"""The multi-tensor ("list") kernels as functions: thin wrappers of csrc/psgd_multi_tail.hip, one launch for a whole list of tensors.

    MultiTailPlan                                         the tables and workspaces of lists of fixed sizes
    multi_sumsq, multi_param_update, multi_diff_scale,
    multi_blend, multi_scale_check, multi_widen_check,
    multi_narrow, multi_randn                             the step tail of class Kron (kron_optimizer.py), usable on their own
    multi_vec_precond_update, multi_vec_precond_grad      update_precond_kron / precond_grad_kron on k vector layers

Nothing here knows class Kron; kron_optimizer.py imports these names back and calls them as its own globals.
"""
import math

import numpy as np
import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd

_f32 = torch.float32
_TINY = float(np.finfo(np.float32).tiny)
_HALF = (torch.bfloat16, torch.float16)
_MIXED = (torch.float32, torch.bfloat16)            # the dtypes of a mixed list: a preconditioned gradient is one or the other
_DTYPE_NAMES = {torch.float32: "float32", torch.bfloat16: "bfloat16", torch.float16: "float16"}
_CODE_DTYPES = {code: dt for dt, code in _psgd._TAIL_DTYPES.items()}


# --------------------------------------------------------------------------- list kernels
class MultiTailPlan(_psgd.UVdTailPlan):
    """The chunk table, the segment tables (one per role), the device double of the clip norm and the workspace of its reduction for
    lists of tensors of fixed sizes.  The tables hold pointers and element counts only, so one plan serves the fp32 lists and
    the bfloat16 / float16 lists of the typed entry points alike.  Calls that share a plan must run on one stream.
    dtypes (None: nothing changes): one dtype per PARAMETER tensor, float32, bfloat16 or float16 each.  With more than one present
    the plan is MIXED (UVdTailPlan): the typed lists of a call (params, vs, the sources of a widening) are checked tensor by
    tensor against these, and every typed launch runs once per dtype present over that dtype's sub-plan (dtype_chunks)."""

    def __init__(self, sizes, device, dtypes=None):
        # (dtypes that are all one: the dtype-agnostic plan, whose typed calls take T from params[0] as they always did)
        super().__init__(sizes, list(dtypes) if dtypes is not None and len(set(dtypes)) > 1 else torch.float32, device)
        self.ws = torch.empty(_lib.MULTI_SUMSQ_WS_BYTES, dtype=torch.uint8, device=self.device)
        # the flag word of the guarded step (multi_scale_check) and the stamp last stored to it.  The word is zeroed ONCE, here: the
        # kernel stores a stamp that this word has not seen before, so nothing ever clears it again
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.stamp = 0

    def table(self, role, tensors, what, dtype=_f32):
        """device pointer of the segment table of `tensors` (contiguous tensors of `dtype` -- one for all, or a list with one per
        tensor -- with the plan's sizes) in this role"""
        return super().table(role, tensors, what, dtype)

    def mixed_table(self, role, tensors, what):
        """device pointer of the segment table of a MIXED list in this role: contiguous tensors with the plan's sizes, each float32
        or bfloat16; the `start` field of a segment holds its PSGD_DTYPE_* code (include/psgd_hip.h)"""
        if len(tensors) != len(self.sizes):
            raise ValueError("%s: %d tensors, the plan has %d" % (what, len(tensors), len(self.sizes)))
        for t, n in zip(tensors, self.sizes):
            if t.dtype not in _MIXED or t.device != self.device or t.numel() != n or not t.is_contiguous():
                raise ValueError("%s: every tensor must be a contiguous float32 or bfloat16 tensor on %s with the plan's element "
                                 "count (%d), got %s %s %s%s" % (what, self.device, n, t.dtype, t.device, tuple(t.shape),
                                                                 "" if t.is_contiguous() else " strided"))
        codes = [_psgd._TAIL_DTYPES[t.dtype] for t in tensors]
        tab = self._tables.get(role)
        if tab is None:
            tab = self._tables[role] = _psgd._SegTable(codes, self.sizes, self.device)
            tab.codes = codes
        elif tab.codes != codes:                               # another pattern of dtypes in this role: rewrite and upload again
            if tab.uploaded is not None:
                tab.uploaded.synchronize()
            tab.rows[:, 1] = codes
            tab.codes, tab.ptrs = codes, None
        return tab.refresh([t.data_ptr() for t in tensors])

    def next_stamp(self):
        """1 .. 2^31 - 1, then 1 again"""
        self.stamp = self.stamp % (2 ** 31 - 1) + 1
        return self.stamp


_multi_plans = {}


def _check_list(what, name, tensors, sizes=None, device=None, dtype=_f32):
    """one operand list of a list kernel: contiguous tensors of `dtype` (float32 unless the caller names another) on one HIP
    device, sizes[i] elements at position i"""
    tensors = list(tensors)
    if sizes is not None and len(tensors) != len(sizes):
        raise ValueError("%s: %s has %d tensors, the first list has %d" % (what, name, len(tensors), len(sizes)))
    each = dtype if isinstance(dtype, list) else None           # (a list: one dtype per position, a mixed plan's)
    if each is not None and len(each) != len(tensors):
        raise ValueError("%s: %s has %d tensors, the plan has %d" % (what, name, len(tensors), len(each)))
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s[%d] is not a torch tensor (%r)" % (what, name, i, type(t)))
        if each is not None:
            dtype = each[i]
        if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):          # (a tuple: a mixed list)
            raise TypeError("%s: %s[%d] must be %s, got %s" % (what, name, i, " or ".join(
                _DTYPE_NAMES[d] for d in (dtype if isinstance(dtype, tuple) else (dtype,))), t.dtype))
        if not t.is_cuda:
            raise _lib.PsgdHipError("%s runs on the HIP device only (%s[%d] is on %s); no CPU fallback" % (what, name, i, t.device))
        if device is None:
            device = t.device
        if t.device != device:
            raise ValueError("%s: all tensors must be on one device, %s[%d] is on %s, not %s" % (what, name, i, t.device, device))
        if not t.is_contiguous():
            raise ValueError("%s: %s[%d] (shape %s) is not contiguous" % (what, name, i, tuple(t.shape)))
        if sizes is not None and int(t.numel()) != sizes[i]:
            raise ValueError("%s: %s[%d] has %d elements, position %d of the first list has %d"
                             % (what, name, i, t.numel(), i, sizes[i]))
    return tensors, device


def _lists(what, first, *others, plan=None, dtypes=None):
    """checks every list against the first one; returns (lists, plan).  dtypes: {list name: dtype} of the lists that are not fp32"""
    dtypes = dtypes or {}
    name0, t0 = first
    t0, dev = _check_list(what, name0, t0, dtype=dtypes.get(name0, _f32))
    if not t0:
        raise ValueError("%s: empty tensor list" % what)
    sizes = tuple(int(t.numel()) for t in t0)
    out = [t0]
    for name, ts in others:
        out.append(None if ts is None else _check_list(what, name, ts, sizes, dev, dtypes.get(name, _f32))[0])
    if plan is None:
        key = (dev, sizes)
        plan = _multi_plans.get(key)
        if plan is None:
            while len(_multi_plans) >= 16:
                _multi_plans.pop(next(iter(_multi_plans)))
            plan = _multi_plans[key] = MultiTailPlan(sizes, dev)
    elif plan.sizes != sizes or plan.device != dev:
        raise ValueError("%s: the plan is for sizes %r on %s, the tensors have %r on %s" % (what, plan.sizes, plan.device, sizes, dev))
    return out, plan


def _has_bf16(tensors):
    """a list of gradients with a bfloat16 device tensor in it is a MIXED list (the preconditioned gradients of an optimizer with
    bf16-operand layers); anything else takes the checks and the entry points of the fp32 lists"""
    return any(isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 and t.is_cuda for t in tensors)


def multi_sumsq(tensors, *, plan=None, out=None, ws=None):
    """out[0] = sum of fl32(x * x) over every element of every tensor, in fp64 and in a fixed order (psgd_multi_sumsq_f32: two launches
    whatever len(tensors), the same bits on every call).  tensors: contiguous fp32 tensors on one HIP device, empty ones allowed.
    out: a float64 device tensor of one element (default: the plan's); ws: a uint8 device tensor of at least
    _lib.MULTI_SUMSQ_WS_BYTES bytes (default: the plan's).  Returns out.
    A MIXED list -- some tensors bfloat16, the others float32 -- goes to psgd_multi_sumsq_mixed: the squares are those of float(x),
    the structure and the fixed order are the same; a list without a bfloat16 tensor calls psgd_multi_sumsq_f32 as before."""
    tensors = list(tensors)
    mixed = _has_bf16(tensors)
    (tensors,), plan = _lists("multi_sumsq", ("tensors", tensors), plan=plan, dtypes={"tensors": _MIXED} if mixed else None)
    out = plan.sumsq if out is None else out
    ws = plan.ws if ws is None else ws
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != plan.device or out.numel() < 1:
        raise ValueError("multi_sumsq: out must be a float64 tensor of at least one element on %s" % (plan.device,))
    if not isinstance(ws, torch.Tensor) or ws.dtype != torch.uint8 or ws.device != plan.device or not ws.is_contiguous():
        raise ValueError("multi_sumsq: ws must be a contiguous uint8 tensor on %s" % (plan.device,))
    if not plan.nchunks:
        out[:1].zero_()                                              # the kernel launches nothing: the sum of nothing is 0
        return out
    if mixed:
        rc = _lib.load().psgd_multi_sumsq_mixed(plan.mixed_table("sumsq_mixed", tensors, "multi_sumsq"), len(tensors),
                                                plan.chunks.data_ptr(), plan.nchunks, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _psgd._stream_ptr(plan.device))
        _lib.check(rc, "psgd_multi_sumsq_mixed")
        return out
    rc = _lib.load().psgd_multi_sumsq_f32(plan.table("sumsq", tensors, "multi_sumsq"), len(tensors), plan.chunks.data_ptr(),
                                          plan.nchunks, out.data_ptr(), ws.data_ptr(), ws.numel(), _psgd._stream_ptr(plan.device))
    _lib.check(rc, "psgd_multi_sumsq_f32")
    return out


def multi_param_update(params, grads, vs=None, lr=0.0, sumsq=None, max_norm=None, tiny=None, *, plan=None, weight_decay=0.0,
                       rounding="nearest", rounding_seed=None, index0=0, tensor_groups=None):
    """For all parameters in ONE launch (psgd_multi_param_update_f32), every operation rounded to float32 on its own:
        p <- p - lr_eff * g                     vs None
        p <- p - (lr_eff * g + v)               vs given (the undo of the finite-difference perturbation, psgd.py:761)
        p <- p + v                              grads None (the perturbation itself, psgd.py:723; lr, sumsq are not used)
    lr_eff = float32(lr) when sumsq is None; with sumsq (a float64 device tensor of one element, what multi_sumsq left) and max_norm,
    lr_eff = float32(lr * min(max_norm / (sqrt(sumsq) + tiny), 1)) formed on the device in fp64: no host read; a NaN sumsq makes
    every parameter NaN, as torch.minimum does.  tiny defaults to the smallest normal float32.
    weight_decay (decoupled; psgd_multi_param_update_wd_f32): with c = float32(lr_eff * weight_decay), the subtracted term gains
    float32(c * p) after the vs term; 0 (default) adds no rounding step and calls the entry point without decay.
    The parameters are written through their pointers: autograd's version counters do not move.
    Half precision: when params[0] is a bfloat16 or float16 tensor on the HIP device, params and vs have that type T, grads stay
    float32, and the call goes to psgd_multi_param_update_t: delta = T(float32(lr_eff * g)), then T(delta + v), then
    T(delta + T(float32(c * float(p)))), p <- T(p - delta); p <- T(p + v) without grads.  tiny then defaults to finfo(T).tiny.
    (A half-precision tensor that is not on the device is refused as before: params must be float32.)
    A plan built for a MIXED list (MultiTailPlan(sizes, device, dtypes)): params and vs have the plan's dtype at every position, and
    the entry point a one-dtype list of that dtype would take is launched once per dtype present over that dtype's sub-plan
    (crossed with tensor_groups: per (group, dtype) pair that has tensors); rounding="stochastic" applies to the bfloat16 tensors
    and needs one and no float16 tensor; tiny defaults to the largest finfo(T).tiny present.
    MIXED gradients: when some tensors of grads are bfloat16 device tensors and the others float32 (the preconditioned gradients
    of bf16-operand layers), the call goes to psgd_multi_param_update_mixed, which reads every gradient as float(g) and rounds as
    above for the parameters' dtype, float32 included.  A list without a bfloat16 tensor calls the entry points of before.
    rounding="stochastic" (bfloat16 parameters, grads required; psgd_multi_param_update_sr, with mixed gradients
    psgd_multi_param_update_mixed_sr): the update is formed once in float32 and narrowed once -- w = float(p),
    d = fl32(lr_eff * float(g)), d = fl32(d + float(v)), d = fl32(d + fl32(c * w)), p <- SR(fl32(w - d)) -- with the stochastic
    narrowing of stochastic_narrow_bf16 under rounding_seed (None: drawn from the module's branch generator) on the flat index
    index0 + the element's place in the concatenation of params.  "nearest" (default): nothing changes, and rounding_seed / index0
    must be left alone.
    tensor_groups (None: nothing changes): a sequence of (indices, lr_scale, weight_decay) that partitions range(len(params));
    weight_decay itself must then be left at 0.  The entry point the call would take anyway is launched once per group over the
    group's chunks (plan.group_chunks: the plan's segment tables, uploaded once) with lr_j = fl32(float(lr) * lr_scale_j), the
    product formed in double and rounded once, and the group's weight_decay, so lr_eff_j = fl32(double(lr_j) * the clip factor)
    and c_j = fl32(lr_eff_j * fl32(wd_j)); a group whose weight_decay is 0 takes the form without the decay term.  sumsq is the
    caller's, of all gradients and before any scale; the stochastic-rounding index of an element does not depend on the grouping."""
    what = "multi_param_update"
    wd = float(weight_decay)
    if not wd >= 0.0:
        raise ValueError("%s: weight_decay must be >= 0, got %r" % (what, weight_decay))
    if rounding not in _psgd._PARAM_ROUNDINGS:
        raise ValueError("%s: rounding must be 'nearest' or 'stochastic', got %r" % (what, rounding))
    sr = rounding == "stochastic"
    if not sr and (rounding_seed is not None or index0 != 0):
        raise ValueError("%s: rounding_seed and index0 apply to rounding='stochastic' only" % what)
    if sr and (grads is None or int(index0) < 0):
        raise ValueError("%s: rounding='stochastic' needs grads (the perturbation p + v rounds to nearest) and index0 >= 0" % what)
    params = list(params)
    T = _f32
    if plan is not None and plan.mixed:                         # a plan built for a mixed list: one dtype per position
        T = list(plan.dtypes)
    elif params and isinstance(params[0], torch.Tensor) and params[0].is_cuda and params[0].dtype in _HALF:
        T = params[0].dtype
    grads = None if grads is None else list(grads)
    mixed = grads is not None and _has_bf16(grads)
    dtypes = {"params": T, "vs": T}
    if mixed:
        dtypes["grads"] = _MIXED
    (params, grads, vs), plan = _lists(what, ("params", params), ("grads", grads), ("vs", vs), plan=plan, dtypes=dtypes)
    groups = _psgd._tensor_groups(what, tensor_groups, len(params), wd, grads is not None)
    if grads is None and (vs is None or sumsq is not None or wd != 0.0):
        raise ValueError("%s: grads=None adds vs to the parameters; it needs vs and takes no sumsq and no weight_decay" % what)
    if (sumsq is None) != (max_norm is None):
        raise ValueError("%s: sumsq and max_norm go together" % what)
    if sumsq is not None and (not isinstance(sumsq, torch.Tensor) or sumsq.dtype != torch.float64 or sumsq.device != plan.device
                              or sumsq.numel() < 1):
        raise ValueError("%s: sumsq must be a float64 tensor of at least one element on %s" % (what, plan.device))
    if sr and isinstance(T, list):
        _psgd._param_rounding(what, rounding, set(T))
    elif sr and T != torch.bfloat16:
        raise ValueError("%s: rounding='stochastic' needs bfloat16 parameters on the HIP device, got %s" % (what, params[0].dtype))
    if not plan.nchunks:
        return
    if sr and rounding_seed is None:
        rounding_seed = int(torch.randint(0, 2 ** 62, (), generator=_psgd._branch_rng).item())
    # the segment tables: made (and uploaded where a pointer moved) once, whatever the number of launches
    ptab = plan.table("params", params, what, T)
    gtab = None if grads is None else plan.mixed_table("grads_mixed", grads, what) if mixed else plan.table("grads", grads, what)
    vtab = None if vs is None else plan.table("vs", vs, what, T)
    clip = (None if sumsq is None else sumsq.data_ptr(), 0.0 if max_norm is None else float(max_norm),
            float((plan.tiny if isinstance(T, list) else torch.finfo(T).tiny) if tiny is None else tiny))
    # one launch over the plan's chunks, or one per group over the group's: the same tables, the same sum of squares.  A mixed
    # plan: each of these once per dtype present, as the call of a one-dtype list of that dtype, over that dtype's rows
    if isinstance(T, list):
        launches = [(_CODE_DTYPES[code], chunks, n, float(lr) * scale, wd_j)
                    for indices, scale, wd_j in (groups if groups is not None else [(None, 1.0, wd)])
                    for code, chunks, n in plan.dtype_chunks(indices)]
    else:
        launches = [(T, plan.chunks, plan.nchunks, float(lr), wd)] if groups is None else \
            [(T,) + plan.group_chunks(indices) + (float(lr) * scale, wd_j) for indices, scale, wd_j in groups]
    for T, chunks, nchunks, lr_j, wd_j in launches:
        if not nchunks:
            continue
        tabs = (ptab, gtab, vtab, len(params), chunks.data_ptr(), nchunks)
        if sr and T == torch.bfloat16:                          # (the float32 tensors of a mixed list: as under "nearest")
            name = "psgd_multi_param_update_mixed_sr" if mixed else "psgd_multi_param_update_sr"
            rc = getattr(_lib.load(), name)(*tabs, _psgd._TAIL_DTYPES[T], lr_j, *clip, wd_j, int(rounding_seed) & (2 ** 64 - 1),
                                            int(index0), _psgd._stream_ptr(plan.device))
        elif mixed:
            name = "psgd_multi_param_update_mixed"
            rc = _lib.load().psgd_multi_param_update_mixed(*tabs, _psgd._TAIL_DTYPES[T], lr_j, *clip, wd_j,
                                                           _psgd._stream_ptr(plan.device))
        elif T != _f32:
            name = "psgd_multi_param_update_t"
            rc = _lib.load().psgd_multi_param_update_t(*tabs, _psgd._TAIL_DTYPES[T], lr_j, *clip, wd_j, _psgd._stream_ptr(plan.device))
        elif wd_j == 0.0:
            name = "psgd_multi_param_update_f32"
            rc = _lib.load().psgd_multi_param_update_f32(*tabs, lr_j, *clip, _psgd._stream_ptr(plan.device))
        else:
            name = "psgd_multi_param_update_wd_f32"
            rc = _lib.load().psgd_multi_param_update_wd_f32(*tabs, lr_j, *clip, wd_j, _psgd._stream_ptr(plan.device))
        _lib.check(rc, name)


def multi_diff_scale(a, b, h, v=None, x=None, s=1.0, *, plan=None):
    """h <- (a - b) * s and, with v and x (both or neither), x <- v * s for all tensors of the lists in ONE launch
    (psgd_multi_diff_scale_f32), the difference and each product rounded to float32 on its own: the finite-difference
    dG = (g' - g) / delta, dX = v / delta of psgd.py:727, :734-736 with s = 1 / delta."""
    what = "multi_diff_scale"
    if (v is None) != (x is None):
        raise ValueError("%s: v and x go together" % what)
    (a, b, h, v, x), plan = _lists(what, ("a", a), ("b", b), ("h", h), ("v", v), ("x", x), plan=plan)
    if not plan.nchunks:
        return
    rc = _lib.load().psgd_multi_diff_scale_f32(
        plan.table("a", a, what), plan.table("b", b, what), plan.table("h", h, what),
        None if v is None else plan.table("v", v, what), None if x is None else plan.table("x", x, what),
        len(a), plan.chunks.data_ptr(), plan.nchunks, float(s), _psgd._stream_ptr(plan.device))
    _lib.check(rc, "psgd_multi_diff_scale_f32")


def multi_blend(ms, gs, beta, omb, *, plan=None):
    """m <- beta * m + omb * g for all tensors of the lists in ONE launch (psgd_multi_blend_f32), both products and the sum rounded
    to float32 on their own: the momentum of class Kron.  beta and omb are the pair of uvd_momentum_coefficients (omb = float32(1) -
    beta, rounded once); beta == 0 does not read m: whatever it held, NaN included, is replaced by omb * g."""
    what = "multi_blend"
    beta, omb = float(np.float32(beta)), float(np.float32(omb))
    if not 0.0 <= beta < 1.0:
        raise ValueError("%s: beta must be in [0, 1), got %r" % (what, beta))
    (ms, gs), plan = _lists(what, ("ms", ms), ("gs", gs), plan=plan)
    if gs is None:
        raise ValueError("%s: gs is required" % what)
    if not plan.nchunks:
        return
    rc = _lib.load().psgd_multi_blend_f32(plan.table("m", ms, what), plan.table("g", gs, what), len(ms), plan.chunks.data_ptr(),
                                          plan.nchunks, beta, omb, _psgd._stream_ptr(plan.device))
    _lib.check(rc, "psgd_multi_blend_f32")


def multi_scale_check(lists, scales, *, flag=None, stamp=None, plan=None):
    """One to three lists of tensors in ONE launch (psgd_multi_scale_check_f32): every element x of list j becomes float32(x *
    scales[j]) in place where scales[j] != 1 (a list with scale 1 is only read), and with flag and stamp (both or neither) stamp is
    stored to flag[0], an int32 device word, when any of these products -- of a scaled list or not -- is +-Inf or NaN.  The caller
    passes a stamp it has not used on this word before (1 .. 2^31 - 1; plan.next_stamp() for plan.flag) and reads flag[0] == stamp
    after the launch; nothing zeroes the word.  Without a flag the call only rescales, and all scales equal to 1 is an error."""
    what = "multi_scale_check"
    lists, scales = list(lists), [float(np.float32(s)) for s in scales]
    if not 1 <= len(lists) <= 3 or len(scales) != len(lists):
        raise ValueError("%s: one to three lists and one scale for each, got %d lists and %d scales" % (what, len(lists), len(scales)))
    if (flag is None) != (stamp is None):
        raise ValueError("%s: flag and stamp go together (got flag=%s, stamp=%r)" % (what, "None" if flag is None else "given", stamp))
    if flag is None and all(s == 1.0 for s in scales):
        raise ValueError("%s: no flag and every scale is 1: nothing to do" % what)
    # a mixed plan: only its float32 tensors are walked; the positions of the other dtypes hold tensors of those dtypes, untouched
    own = list(plan.dtypes) if plan is not None and plan.mixed else None
    lists, plan = _lists(what, *[("lists[%d]" % j, ts) for j, ts in enumerate(lists)], plan=plan,
                         dtypes=None if own is None else {"lists[%d]" % j: own for j in range(len(lists))})
    if any(ts is None for ts in lists):
        raise ValueError("%s: a list is None" % what)
    word = None
    if flag is not None:
        word = _psgd._flag_word(what, flag, stamp, plan.device)
        if not 1 <= int(stamp) <= 2 ** 31 - 1:
            raise ValueError("%s: stamp must be in 1 .. 2^31 - 1, got %r" % (what, stamp))
    if not plan.nchunks:
        return
    tabs = [plan.table("check%d" % j, ts, what, _f32 if own is None else own) for j, ts in enumerate(lists)] + \
        [None] * (3 - len(lists))
    for code, chunks, nchunks in plan.by_dtype:
        if code != _lib.DTYPE_F32:
            continue
        rc = _lib.load().psgd_multi_scale_check_f32(*tabs, *(scales + [1.0] * (3 - len(scales))), len(lists[0]), chunks.data_ptr(),
                                                    nchunks, word, 0 if stamp is None else int(stamp),
                                                    _psgd._stream_ptr(plan.device))
        _lib.check(rc, "psgd_multi_scale_check_f32")


def multi_widen_check(srcs, dsts, scales, *, flag=None, stamp=None, plan=None):
    """One to three lists of bfloat16 or float16 tensors widened into as many lists of float32 tensors in ONE launch
    (psgd_multi_widen_check): dsts[j][i] <- float32(float(srcs[j][i]) * scales[j]).  All source tensors have the dtype of
    srcs[0][0]; every destination is written whole.  With flag and stamp (both or neither) stamp is stored to flag[0], an int32
    device word, when any value written is +-Inf or NaN -- the flag of multi_scale_check: the caller passes a stamp it has not
    used on this word before (1 .. 2^31 - 1; plan.next_stamp() for plan.flag) and reads flag[0] == stamp after the launch;
    nothing zeroes the word.  Without a flag the call only widens.
    A plan built for a MIXED list: srcs have the plan's dtype at every position, one launch per half-precision dtype present over
    its sub-plan, all under the one stamp and flag; the float32 positions are skipped (neither read nor written: their dsts may
    be the sources themselves) and are left to multi_scale_check with the same plan, which walks the float32 sub-plan only."""
    what = "multi_widen_check"
    srcs, dsts, scales = list(srcs), list(dsts), [float(np.float32(s)) for s in scales]
    if not 1 <= len(srcs) <= 3 or len(dsts) != len(srcs) or len(scales) != len(srcs):
        raise ValueError("%s: one to three source lists, a destination list and a scale for each, got %d, %d and %d"
                         % (what, len(srcs), len(dsts), len(scales)))
    if (flag is None) != (stamp is None):
        raise ValueError("%s: flag and stamp go together (got flag=%s, stamp=%r)" % (what, "None" if flag is None else "given", stamp))
    srcs = [None if ts is None else list(ts) for ts in srcs]
    if any(ts is None for ts in srcs) or any(ts is None for ts in dsts):
        raise ValueError("%s: a list is None" % what)
    own = list(plan.dtypes) if plan is not None and plan.mixed else None
    first = srcs[0][0] if srcs[0] else None
    T = own if own is not None else first.dtype if isinstance(first, torch.Tensor) else None
    if own is None and isinstance(first, torch.Tensor) and T not in _HALF:
        raise TypeError("%s: srcs[0][0] must be bfloat16 or float16, got %s (float32 lists are scaled in place by multi_scale_check)"
                        % (what, T))
    names = ["srcs[%d]" % j for j in range(len(srcs))]
    lists, plan = _lists(what, *(list(zip(names, srcs)) + [("dsts[%d]" % j, ts) for j, ts in enumerate(dsts)]), plan=plan,
                         dtypes={n: T for n in names})
    srcs, dsts = lists[:len(srcs)], lists[len(srcs):]
    word = None
    if flag is not None:
        word = _psgd._flag_word(what, flag, stamp, plan.device)
        if not 1 <= int(stamp) <= 2 ** 31 - 1:
            raise ValueError("%s: stamp must be in 1 .. 2^31 - 1, got %r" % (what, stamp))
    if not plan.nchunks:
        return
    pad = [None] * (3 - len(srcs))
    tabs = [plan.table("widen_src%d" % j, ts, what, T) for j, ts in enumerate(srcs)] + pad + \
        [plan.table("widen_dst%d" % j, ts, what) for j, ts in enumerate(dsts)] + pad
    for code, chunks, nchunks in plan.by_dtype if own is not None else [(_psgd._TAIL_DTYPES[T], plan.chunks, plan.nchunks)]:
        if code == _lib.DTYPE_F32:                              # (a mixed plan: its float32 tensors skip the widening pass)
            continue
        rc = _lib.load().psgd_multi_widen_check(*tabs, *(scales + [1.0] * len(pad)), len(srcs[0]), chunks.data_ptr(), nchunks,
                                                code, word, 0 if stamp is None else int(stamp), _psgd._stream_ptr(plan.device))
        _lib.check(rc, "psgd_multi_widen_check")


def multi_narrow(srcs, dsts, *, plan=None):
    """One to three lists of float32 tensors narrowed into as many lists of bfloat16 tensors in ONE launch (psgd_multi_narrow_bf16):
    dsts[j][i] <- srcs[j][i].to(torch.bfloat16), bit for bit -- round to nearest even, NaN stays NaN, a finite value beyond the
    bfloat16 range becomes +-Inf.  multi_widen_check in the other direction, without a scale and without a flag: every destination
    is written whole and nothing is judged.  All tensors contiguous on one HIP device, dsts[j][i] with the element count of
    srcs[j][i].  Returns dsts."""
    what = "multi_narrow"
    srcs, dsts = list(srcs), list(dsts)
    if not 1 <= len(srcs) <= 3 or len(dsts) != len(srcs):
        raise ValueError("%s: one to three source lists and a destination list for each, got %d and %d" % (what, len(srcs), len(dsts)))
    if any(ts is None for ts in srcs) or any(ts is None for ts in dsts):
        raise ValueError("%s: a list is None" % what)
    names = ["dsts[%d]" % j for j in range(len(dsts))]
    lists, plan = _lists(what, *([("srcs[%d]" % j, ts) for j, ts in enumerate(srcs)] + list(zip(names, dsts))), plan=plan,
                         dtypes={n: torch.bfloat16 for n in names})
    srcs, dsts = lists[:len(srcs)], lists[len(srcs):]
    if not plan.nchunks:
        return dsts
    pad = [None] * (3 - len(srcs))
    rc = _lib.load().psgd_multi_narrow_bf16(*([plan.table("narrow_src%d" % j, ts, what) for j, ts in enumerate(srcs)] + pad),
                                            *([plan.table("narrow_dst%d" % j, ts, what, torch.bfloat16)
                                               for j, ts in enumerate(dsts)] + pad),
                                            len(srcs[0]), plan.chunks.data_ptr(), plan.nchunks, _psgd._stream_ptr(plan.device))
    _lib.check(rc, "psgd_multi_narrow_bf16")
    return dsts


def multi_randn(outs, seed, index0=0, scale=1.0, *, plan=None):
    """Standard normal draws into all tensors of a list in ONE launch (psgd_multi_randn_f32): element j of the concatenation of outs
    (contiguous float32 tensors on one HIP device, empty ones allowed) becomes float32(scale) * z_i, i = index0 + j, and z_i is a
    function of (seed, i) alone -- a counter hash and Box-Muller on pairs, the stream psgd.counter_randn restates in float64; the
    two agree to a few float32 ulps (profiles/kron_whitening.txt).  The draws do not depend on how the list is cut into tensors,
    on where the tensors start, on the launch shape or on any torch generator, and every value is finite.  seed: any integer (its
    low 64 bits); index0 >= 0; scale finite.  Returns outs."""
    what = "multi_randn"
    if int(index0) != index0 or int(index0) < 0 or int(index0) >= 2 ** 63:
        raise ValueError("%s: index0 must be an integer in [0, 2^63), got %r" % (what, index0))
    scale = float(np.float32(scale))
    if not math.isfinite(scale):
        raise ValueError("%s: scale must be a finite float32 value, got %r" % (what, scale))
    (outs,), plan = _lists(what, ("outs", outs), plan=plan)
    if not plan.nchunks:
        return outs
    rc = _lib.load().psgd_multi_randn_f32(plan.table("randn", outs, what), len(outs), plan.chunks.data_ptr(), plan.nchunks,
                                          int(seed) & (2 ** 64 - 1), int(index0), scale, _psgd._stream_ptr(plan.device))
    _lib.check(rc, "psgd_multi_randn_f32")
    return outs


# --------------------------------------------------------------------------- vector layers
def _vec_lists(what, qls, first, *others, plan=None):
    """the operand lists of a vector-layer kernel: `first` and `others` as _lists checks them, every tensor of at least 2 elements,
    and qls, one fp32 tensor of ONE element per vector.  Returns (qls, lists, plan, device pointer of the table of qls)."""
    lists, plan = _lists(what, first, *others, plan=plan)
    if any(ts is None for ts in lists):
        raise ValueError("%s: a list is None" % what)
    for i, n in enumerate(plan.sizes):
        if n < 2:
            raise ValueError("%s: %s[%d] has %d element%s; a vector layer has at least 2 (a scaling factor of length 1 is square, and "
                             "the reference's dispatcher would run it as a dense one)" % (what, first[0], i, n, "" if n == 1 else "s"))
    qls, _ = _check_list(what, "qls", qls, (1,) * len(plan.sizes), plan.device)
    tab = plan._tables.get("vec_ql")
    if tab is None:
        tab = plan._tables["vec_ql"] = _psgd._SegTable(list(range(len(qls))), [1] * len(qls), plan.device)
    return qls, lists, plan, tab.refresh([t.data_ptr() for t in qls])


def multi_vec_precond_update(qls, qrs, dXs, dGs, step, tiny=None, *, plan=None):
    """update_precond_kron on k vector layers in ONE launch (psgd_multi_vec_update_f32), IN PLACE.  Vector i of length n_i >= 2 is
    the reference's layer of shape [1, n_i] in the (dense, scaling) format (psgd.py:276-307): qls[i] holds the 1 x 1 left factor,
    qrs[i] the [1, n_i] scaling factor, dXs[i] and dGs[i] the pair (dx, dg), all contiguous fp32 tensors on one HIP device with these
    element counts, of any shape.  fp32 in the reference's order -- the balance rho = sqrt(ql / max(qr)) is performed, not cancelled
    -- with the two sums of squares accumulated in fp64 in a fixed order (the same bits on every call, whatever k and the vector's
    place in the list) and NaN-propagating maxima.  tiny defaults to the smallest normal float32.  One workgroup per vector: a
    vector of a million elements is correct but slow."""
    what = "multi_vec_precond_update"
    qls, (qrs, dXs, dGs), plan, ql_tab = _vec_lists(what, qls, ("qrs", qrs), ("dXs", dXs), ("dGs", dGs), plan=plan)
    rc = _lib.load().psgd_multi_vec_update_f32(ql_tab, plan.table("vec_qr", qrs, what), plan.table("vec_dx", dXs, what),
                                               plan.table("vec_dg", dGs, what), len(qrs), min(plan.sizes), float(step),
                                               float(_TINY if tiny is None else tiny), _psgd._stream_ptr(plan.device))
    _lib.check(rc, "psgd_multi_vec_update_f32")


def multi_vec_precond_grad(qls, qrs, gs, outs, *, plan=None):
    """precond_grad_kron on k vector layers in ONE launch (psgd_multi_vec_apply_f32): outs[i] <- ((ql ql) g) (qr qr), the M < N branch of
    psgd.py:318-319 and :322 on the [1, n_i] layer, every product rounded to float32 on its own.  Lists as in
    multi_vec_precond_update; outs may be gs itself (in place).  Returns outs."""
    what = "multi_vec_precond_grad"
    qls, (qrs, gs, outs), plan, ql_tab = _vec_lists(what, qls, ("qrs", qrs), ("gs", gs), ("outs", outs), plan=plan)
    rc = _lib.load().psgd_multi_vec_apply_f32(ql_tab, plan.table("vec_qr", qrs, what), plan.table("vec_g", gs, what),
                                              plan.table("vec_out", outs, what), len(qrs), min(plan.sizes),
                                              _psgd._stream_ptr(plan.device))
    _lib.check(rc, "psgd_multi_vec_apply_f32")
    return outs
