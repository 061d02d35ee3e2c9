"""The QUAD Kronecker update and apply on a LIST of ORDER-3 tensor layers (three symmetric factors each), on psgd_kron_qtlist.hip:
at most eight launches per group of layers for the update and six for the apply, whatever the number of layers, with the Gram of a
short side split along K and folded in fp64.

include/psgd_kron_quad_nd_list_hip.h states the contract.  A layer all of whose sides have one slice (plan.slices) gets, bit for
bit, what update_precond_kron_quad_nd_ gives on that layer alone; the apply always has the bits of precond_grad_kron_quad_nd; a
split side differs by the rounding of its Gram sum alone.  Nothing depends on the list, its order or the cap.

    KronQuadTensorListPlan(shapes, device, max_group_bytes, gram_slice_k)     the planner's output, the workspace, the tables
    update_precond_kron_quad_nd_list_(Qs_list, Ls, Gs, step, decay)           the update, in place on every factor and L
    precond_grad_kron_quad_nd_list(Qs_list, Gs, outs=None)                    outs[i] = G_i x1 Qa_i^2 x2 Qb_i^2 x3 Qc_i^2

The four C entry points are bound here, in a signature table of this module's own.  fp32 on the HIP device only; no fallback.
class Kron(preconditioner_update="quad", any_rank=True, quad_tensor=True, quad_tensor_route="list") runs its tensor layers through
the two functions.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd
from .kron_quad_list import _Table, _span
from .kron_quad_nd import MAX_NUMEL

WS_REGIONS = 21              # PSGD_KRON_QTL_WS_REGIONS
STAGES = 10                  # PSGD_KRON_QTL_STAGES
STAGE_NAMES = ("mode_a", "mode_b", "mode_c", "apply_0", "apply_1", "apply_2", "gram", "fold", "upper", "full")
DEFAULT_GROUP_BYTES = 1024 << 20     # PSGD_KRON_QTL_DEFAULT_GROUP_BYTES
DEFAULT_GRAM_SLICE_K = 2048          # PSGD_KRON_QTL_DEFAULT_SLICE_K (profiles/kron_quad_nd_list_timing.txt)
_ROW = 8 + WS_REGIONS        # int64 words of a psgd_kron_qtl_layer: Qa, Qb, Qc, L, G, out, (A | B << 32), C, ws_off[21]

_p, _i64, _int, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
_ip, _lp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
SIGNATURES = {
    "psgd_kron_qtl_workspace_bytes": (_i64, [_ip, _ip, _ip, _int, _i64, _int]),
    "psgd_kron_qtl_plan": (_int, [_ip, _ip, _ip, _int, _i64, _int, _ip, _ip, _lp, _ip]),
    "psgd_kron_qtl_update_f32": (_int, [_p, _p, _ip, _ip, _int, _ip, _ip, _ip, _int, _int, _flt, _flt, _p, _i64, _p]),
    "psgd_kron_qtl_apply_f32": (_int, [_p, _p, _ip, _ip, _int, _ip, _ip, _ip, _int, _int, _p, _i64, _p]),
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


def _ints(a):
    return a.ctypes.data_as(_ip)


def plan_layers(shapes, max_group_bytes=DEFAULT_GROUP_BYTES, gram_slice_k=DEFAULT_GRAM_SLICE_K):
    """The planner on the host (no device is touched): dict(groups=[(first, end), ...], order={stage: [layer, ...]},
    prefix={stage: [0, ..., workgroups]}, slices=[(Sa, Sb, Sc), ...], ws_off=int64 array [k, 21], ws_bytes=the workspace block,
    raw=(A, B, C, group_start, plan) the arrays the entry points take).  shapes: [(A, B, C), ...]."""
    shapes = [tuple(int(n) for n in s) for s in shapes]
    if not shapes or any(len(s) != 3 or min(s) < 1 or s[0] * s[1] * s[2] > MAX_NUMEL for s in shapes):
        raise ValueError("kron_quad_nd_list: shapes must be a non-empty list of (A, B, C) with A, B, C >= 1 and A B C < 2^31, got %r"
                         % (shapes,))
    gsk = int(gram_slice_k)
    if gsk < 16 or gsk % 16:
        raise ValueError("kron_quad_nd_list: gram_slice_k must be a positive multiple of 16, got %r" % (gram_slice_k,))
    k, cap, lib = len(shapes), int(max_group_bytes), load()
    A, B, C = (np.ascontiguousarray([s[d] for s in shapes], dtype=np.int32) for d in (0, 1, 2))
    group_start, plan = np.zeros(k + 1, dtype=np.int32), np.zeros(STAGES * (2 * k + 1), dtype=np.int32)
    ws_off, slices = np.zeros((k, WS_REGIONS), dtype=np.int64), np.zeros((k, 3), dtype=np.int32)
    groups = int(lib.psgd_kron_qtl_plan(_ints(A), _ints(B), _ints(C), k, cap, gsk, _ints(group_start), _ints(plan),
                                        ws_off.ctypes.data_as(_lp), _ints(slices)))
    if groups < 1:
        _lib.check(groups, "psgd_kron_qtl_plan")
    ws_bytes = int(lib.psgd_kron_qtl_workspace_bytes(_ints(A), _ints(B), _ints(C), k, cap, gsk))
    if ws_bytes < 1:
        _lib.check(ws_bytes, "psgd_kron_qtl_workspace_bytes")
    per = plan.reshape(STAGES, 2 * k + 1)
    return dict(groups=[(int(group_start[g]), int(group_start[g + 1])) for g in range(groups)],
                order={s: per[i, :k].tolist() for i, s in enumerate(STAGE_NAMES)},
                prefix={s: per[i, k:].tolist() for i, s in enumerate(STAGE_NAMES)},
                slices=[tuple(r) for r in slices.tolist()], ws_off=ws_off, ws_bytes=ws_bytes, raw=(A, B, C, group_start, plan))


def table_rows(shapes, ws_off):
    """the shape and carve columns of the descriptor table: int64 [k, 29], the six pointer columns zero"""
    rows = np.zeros((len(shapes), _ROW), dtype=np.int64)
    rows[:, 6] = [A | (B << 32) for A, B, _ in shapes]
    rows[:, 7] = [C for _, _, C in shapes]
    rows[:, 8:] = ws_off
    return rows


class _TensorTable(_Table):
    """kron_quad_list._Table (pinned host rows, uploaded only when a pointer moved) on the rows of psgd_kron_qtl_layer"""

    def __init__(self, shapes, ws_off, device):
        self.host = torch.from_numpy(table_rows(shapes, ws_off)).pin_memory()
        self.rows = self.host.numpy()
        self.dev = torch.zeros_like(self.host, device=device)
        self.ptrs, self.uploaded = None, None


class KronQuadTensorListPlan:
    """Everything about a list of tensor layers that does not change from call to call: the groups under max_group_bytes, the
    slice counts under gram_slice_k (plan.slices: (Sa, Sb, Sc) per layer), the per-stage order and workgroup prefixes (host and
    device copies), the workspace block of the largest group, and one descriptor table per role.  Calls that share a plan must run
    on one stream."""

    def __init__(self, shapes, device, max_group_bytes=DEFAULT_GROUP_BYTES, gram_slice_k=DEFAULT_GRAM_SLICE_K):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PsgdHipError("KronQuadTensorListPlan runs on the HIP device only (got %s); no CPU fallback" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.shapes = [tuple(int(n) for n in s) for s in shapes]
        self.max_group_bytes, self.gram_slice_k = int(max_group_bytes), int(gram_slice_k)
        self.plan = plan_layers(self.shapes, self.max_group_bytes, self.gram_slice_k)
        self.groups, self.slices = self.plan["groups"], self.plan["slices"]
        self.ws = torch.empty(self.plan["ws_bytes"], dtype=torch.uint8, device=self.device)
        self.plan_dev = torch.from_numpy(self.plan["raw"][4]).to(self.device)
        self._tables = {role: _TensorTable(self.shapes, self.plan["ws_off"], self.device) for role in ("update", "apply")}

    def call(self, role, fn_name, ptrs, *scalars):
        lib = load()
        A, B, C, group_start, plan = self.plan["raw"]
        table = self._tables[role].refresh(ptrs)
        rc = getattr(lib, fn_name)(table, self.plan_dev.data_ptr(), _ints(plan), _ints(group_start), len(self.groups), _ints(A),
                                   _ints(B), _ints(C), len(self.shapes), self.gram_slice_k, *scalars, self.ws.data_ptr(),
                                   self.ws.numel(), _psgd._stream_ptr(self.device))
        _lib.check(rc, fn_name)


_RULES = dict(Qa=lambda s: (s[0], s[0]), Qb=lambda s: (s[1], s[1]), Qc=lambda s: (s[2], s[2]), L=lambda s: (3,), G=lambda s: s,
              out=lambda s: s)


def _operands(name, Qs_list, lists, written, plan):
    """Qs_list: per layer three factors; lists: {operand name: list of tensors} with "G" among them.  Every list as long as G's,
    every tensor float32, shaped by _RULES, contiguous, on one HIP device; no written tensor overlaps any other tensor; the shapes
    are the plan's.  Returns (the plan, made here when None; the lists with Qa, Qb, Qc added)."""
    Gs = lists["G"]
    for key, ts in dict(Qs=Qs_list, **lists).items():
        if not isinstance(ts, (list, tuple)):
            raise TypeError("%s: %s must be a list, got %r" % (name, key if key == "Qs" else key + "s", type(ts)))
        if len(ts) != len(Gs):
            raise ValueError("%s: %d %s entries for %d gradients: the lists must have equal length" % (name, len(ts), key, len(Gs)))
    if not Gs:
        raise ValueError("%s: the lists are empty" % name)
    for i, Qs in enumerate(Qs_list):
        if not isinstance(Qs, (list, tuple)) or len(Qs) != 3:
            raise ValueError("%s: Qs of layer %d must be a list of three factors [Qa, Qb, Qc]" % (name, i))
    lists = dict(Qa=[Qs[0] for Qs in Qs_list], Qb=[Qs[1] for Qs in Qs_list], Qc=[Qs[2] for Qs in Qs_list], **lists)
    shapes, every = [], []
    for i, G in enumerate(Gs):
        for key, ts in lists.items():
            t, tag = ts[i], "%s of layer %d" % (key, i)
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a torch tensor, got %r" % (name, tag, type(t)))
            if t.dtype != torch.float32:
                raise TypeError("%s: %s must be float32, got %s" % (name, tag, t.dtype))
        shape = tuple(int(s) for s in G.shape)
        if len(shape) != 3 or min(shape) < 1 or shape[0] * shape[1] * shape[2] > MAX_NUMEL:
            raise ValueError("%s: G of layer %d must be a tensor [A, B, C] with A, B, C >= 1 and A B C < 2^31, got %s" % (name, i, shape))
        for key, ts in lists.items():
            t, tag = ts[i], "%s of layer %d" % (key, i)
            if tuple(t.shape) != _RULES[key](shape):
                raise ValueError("%s: %s must have shape %s for G of shape %s, got %s" % (name, tag, _RULES[key](shape), shape, tuple(t.shape)))
            if not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous" % (name, tag))
            every.append((tag, key in written, t))
        shapes.append(shape)
    # a sweep over the spans by address: `reach` ends last among those begun so far, `wreach` among the written ones
    reach = wreach = None
    for s in sorted((_span(t) + (w, tag) for tag, w, t in every), key=lambda s: s[:2]):
        hit = wreach if wreach is not None and s[0] < wreach[1] else reach if s[2] and reach is not None and s[0] < reach[1] else None
        if hit is not None:
            raise ValueError("%s: %s and %s share memory; a written operand (%s) must not appear twice or alias another operand"
                             % (name, hit[3], s[3], ", ".join(sorted(written))))
        if reach is None or s[1] > reach[1]:
            reach = s
        if s[2] and (wreach is None or s[1] > wreach[1]):
            wreach = s
    dev = _psgd._require_hip(name, *(t for _, _, t in every))
    if plan is None:
        plan = KronQuadTensorListPlan(shapes, dev)
    elif plan.shapes != shapes or plan.device != dev:
        raise ValueError("%s: the lists have shapes %s on %s, the plan was made for %s on %s" % (name, shapes, dev, plan.shapes, plan.device))
    return plan, lists


def _pointers(lists, k):
    return [[t.data_ptr() for t in lists[key]] if key in lists else [0] * k for key in ("Qa", "Qb", "Qc", "L", "G", "out")]


def update_precond_kron_quad_nd_list_(Qs_list, Ls, Gs, step, decay=0.95, *, plan=None):
    """Qa_i, Qb_i, Qc_i, L_i <- the QUAD step on the tensor G_i for every layer of the list, in place: at most eight launches per
    group of the plan, the host reads nothing.  Qs_list[i] = [Qa_i, Qb_i, Qc_i], Ls[i] of shape (3,).  A layer whose sides all
    have one slice has the bits of update_precond_kron_quad_nd_.  Returns None.  plan: a KronQuadTensorListPlan for these shapes
    (made per call when None: keep one across steps)."""
    plan, lists = _operands("update_precond_kron_quad_nd_list_", Qs_list, dict(L=Ls, G=Gs), {"Qa", "Qb", "Qc", "L"}, plan)
    plan.call("update", "psgd_kron_qtl_update_f32", _pointers(lists, len(Gs)), float(step), float(decay))


def precond_grad_kron_quad_nd_list(Qs_list, Gs, outs=None, *, plan=None):
    """[G_i x1 Qa_i^2 x2 Qb_i^2 x3 Qc_i^2 for every layer], six launches per group of the plan.  outs (made when None) must not
    share memory with any operand.  Bit-identical, layer by layer, to precond_grad_kron_quad_nd."""
    more = dict(G=Gs) if outs is None else dict(G=Gs, out=outs)
    plan, lists = _operands("precond_grad_kron_quad_nd_list", Qs_list, more, {"out"}, plan)
    if outs is None:
        outs = lists["out"] = [torch.empty_like(G) for G in Gs]
    plan.call("apply", "psgd_kron_qtl_apply_f32", _pointers(lists, len(Gs)))
    return list(outs)
