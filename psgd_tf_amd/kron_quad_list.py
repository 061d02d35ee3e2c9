"""The QUAD Kronecker update and apply on a LIST of (dense, dense) layers, on psgd_kron_qlist.hip: six launches per group of
layers for the update and four for the apply, whatever the number of layers.

include/psgd_kron_quad_list_hip.h states the contract.  For every layer the result is bit for bit what update_precond_kron_quad_
and precond_grad_kron_quad of kron_quad.py give on that layer alone; what changes is the number of launches and how full the
device is: a model of many small and medium layers pays 10 launches per group and step instead of 10 per layer.

    KronQuadListPlan(shapes, device, max_group_bytes)                  the planner's output, the workspace, the descriptor tables
    update_precond_kron_quad_list_(Qls, Qrs, Ls, Gs, step, decay)      the update, in place on every Ql, Qr and L
    precond_grad_kron_quad_list(Qls, Qrs, Gs, outs=None)               outs[i] = Ql_i (Ql_i G_i Qr_i) Qr_i

The four C entry points are bound here, in a signature table of this module's own.  fp32 on the HIP device only; no fallback.
Both factors of every layer are dense: a scale factor [1, n] is refused (diagonal sides stay on the per-layer calls).
class Kron(preconditioner_update="quad", quad_route="list") runs its (dense, dense) quad layers through the two functions.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd

WS_REGIONS = 13              # PSGD_KRON_QLIST_WS_REGIONS
STAGES = 6                   # PSGD_KRON_QLIST_STAGES: PROD_M, PROD_N, PROD_MIN, PROD_MAX, UPPER, FULL
STAGE_NAMES = ("prod_m", "prod_n", "prod_min", "prod_max", "upper", "full")
DEFAULT_GROUP_BYTES = 1024 << 20     # PSGD_KRON_QLIST_DEFAULT_GROUP_BYTES (DESIGN 4.9 says why)
_ROW = 6 + WS_REGIONS        # int64 words of a psgd_kron_qlist_layer: Ql, Qr, L, G, out, (M | N << 32), ws_off[13]

_p, _i64, _int, _flt = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
_ip, _lp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
SIGNATURES = {
    "psgd_kron_qlist_workspace_bytes": (_i64, [_ip, _ip, _int, _i64]),
    "psgd_kron_qlist_plan": (_int, [_ip, _ip, _int, _i64, _ip, _ip, _lp]),
    "psgd_kron_qlist_update_f32": (_int, [_p, _p, _ip, _ip, _int, _ip, _ip, _int, _flt, _flt, _p, _i64, _p]),
    "psgd_kron_qlist_apply_f32": (_int, [_p, _p, _ip, _ip, _int, _ip, _ip, _int, _p, _i64, _p]),
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


def plan_layers(shapes, max_group_bytes=DEFAULT_GROUP_BYTES):
    """The planner on the host (no device is touched): dict(groups=[(first, end), ...] over the list, order={stage: [layer, ...]},
    prefix={stage: [0, ..., workgroups]}, ws_off=int64 array [k, 13], ws_bytes=the workspace block, raw=(M, N, group_start, plan)
    the arrays the entry points take).  shapes: [(M, N), ...]."""
    shapes = [tuple(int(n) for n in s) for s in shapes]
    if not shapes or any(len(s) != 2 or s[0] < 1 or s[1] < 1 for s in shapes):
        raise ValueError("kron_quad_list: shapes must be a non-empty list of (M, N) with M, N >= 1, got %r" % (shapes,))
    k, cap, lib = len(shapes), int(max_group_bytes), load()
    M, N = (np.ascontiguousarray([s[d] for s in shapes], dtype=np.int32) for d in (0, 1))
    group_start, plan = np.zeros(k + 1, dtype=np.int32), np.zeros(STAGES * (2 * k + 1), dtype=np.int32)
    ws_off = np.zeros((k, WS_REGIONS), dtype=np.int64)
    groups = int(lib.psgd_kron_qlist_plan(_ints(M), _ints(N), k, cap, _ints(group_start), _ints(plan), ws_off.ctypes.data_as(_lp)))
    if groups < 1:
        _lib.check(groups, "psgd_kron_qlist_plan")
    ws_bytes = int(lib.psgd_kron_qlist_workspace_bytes(_ints(M), _ints(N), k, cap))
    if ws_bytes < 1:
        _lib.check(ws_bytes, "psgd_kron_qlist_workspace_bytes")
    per = plan.reshape(STAGES, 2 * k + 1)
    return dict(groups=[(int(group_start[g]), int(group_start[g + 1])) for g in range(groups)],
                order={s: per[i, :k].tolist() for i, s in enumerate(STAGE_NAMES)},
                prefix={s: per[i, k:].tolist() for i, s in enumerate(STAGE_NAMES)},
                ws_off=ws_off, ws_bytes=ws_bytes, raw=(M, N, group_start, plan))


class _Table:
    """The descriptor table of one role (the update's operands, or the apply's).  The host copy lives in pinned memory; the table
    is uploaded (one asynchronous copy on the current stream) only when a pointer differs from the last upload, after the
    previous upload's event: the pinned rows are not rewritten under a copy in flight."""

    def __init__(self, shapes, ws_off, device):
        k = len(shapes)
        self.host = torch.zeros((k, _ROW), dtype=torch.int64).pin_memory()
        self.rows = self.host.numpy()
        self.rows[:, 5] = [M | (N << 32) for M, N in shapes]
        self.rows[:, 6:] = ws_off
        self.dev = torch.zeros((k, _ROW), dtype=torch.int64, device=device)
        self.ptrs, self.uploaded = None, None

    def refresh(self, ptrs):
        """ptrs: five lists (Ql, Qr, L, G, out), a role's unused one all zeros"""
        if ptrs != self.ptrs:
            if self.uploaded is not None:
                self.uploaded.synchronize()
            for c, col in enumerate(ptrs):
                self.rows[:, c] = col
            self.dev.copy_(self.host, non_blocking=True)
            self.uploaded = torch.cuda.Event()
            self.uploaded.record()
            self.ptrs = ptrs
        return self.dev.data_ptr()


class KronQuadListPlan:
    """Everything about a list of (dense, dense) layers that does not change from call to call: the groups under
    max_group_bytes, the per-stage order and workgroup prefixes (host and device copies), the workspace block of the largest
    group, and one descriptor table per role.  Calls that share a plan must run on one stream."""

    def __init__(self, shapes, device, max_group_bytes=DEFAULT_GROUP_BYTES):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PsgdHipError("KronQuadListPlan runs on the HIP device only (got %s); no CPU fallback" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.shapes = [tuple(int(n) for n in s) for s in shapes]
        self.max_group_bytes = int(max_group_bytes)
        self.plan = plan_layers(self.shapes, self.max_group_bytes)
        self.groups = self.plan["groups"]
        self.ws = torch.empty(self.plan["ws_bytes"], dtype=torch.uint8, device=self.device)
        self.plan_dev = torch.from_numpy(self.plan["raw"][3]).to(self.device)
        self._tables = {role: _Table(self.shapes, self.plan["ws_off"], self.device) for role in ("update", "apply")}

    def call(self, role, fn_name, ptrs, *scalars):
        lib = load()
        M, N, group_start, plan = self.plan["raw"]
        table = self._tables[role].refresh(ptrs)
        rc = getattr(lib, fn_name)(table, self.plan_dev.data_ptr(), _ints(plan), _ints(group_start), len(self.groups), _ints(M),
                                   _ints(N), len(self.shapes), *scalars, self.ws.data_ptr(), self.ws.numel(),
                                   _psgd._stream_ptr(self.device))
        _lib.check(rc, fn_name)


def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _operands(name, lists, written, plan):
    """lists: {operand name: (list of tensors, shape rule (M, N) -> shape)} with "G" among them.  Every list as long as G's,
    every tensor float32, shaped by its rule, contiguous, on one HIP device; no written tensor overlaps any other tensor; the
    shapes are the plan's.  Returns (the plan, made here when None; the shapes)."""
    Gs = lists["G"][0]
    for key, (ts, _) in lists.items():
        if not isinstance(ts, (list, tuple)):
            raise TypeError("%s: %ss must be a list of tensors, got %r" % (name, key, type(ts)))
        if len(ts) != len(Gs):
            raise ValueError("%s: %d %s tensors for %d gradients: the lists must have equal length" % (name, len(ts), key, len(Gs)))
    if not Gs:
        raise ValueError("%s: the lists are empty" % name)
    shapes, every = [], []
    for i, G in enumerate(Gs):
        for key, (ts, _) in lists.items():
            t, tag = ts[i], "%s of layer %d" % (key, i)
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a torch tensor, got %r" % (name, tag, type(t)))
            if t.dtype != torch.float32:
                raise TypeError("%s: %s must be float32, got %s" % (name, tag, t.dtype))
        if G.dim() != 2 or G.shape[0] < 1 or G.shape[1] < 1:
            raise ValueError("%s: G of layer %d must be a matrix [M, N] with M, N >= 1, got %s" % (name, i, tuple(G.shape)))
        M, N = (int(s) for s in G.shape)
        for key, (ts, rule) in lists.items():
            t, tag = ts[i], "%s of layer %d" % (key, i)
            if key in ("Ql", "Qr") and t.dim() == 2 and t.shape[0] == 1 and t.shape[1] >= 2:
                raise ValueError("%s: %s is a scale factor %s; the list route takes dense factors only (diagonal sides stay on "
                                 "the per-layer calls)" % (name, tag, tuple(t.shape)))
            if tuple(t.shape) != rule(M, N):
                raise ValueError("%s: %s must have shape %s for G of shape %s, got %s" % (name, tag, rule(M, N), (M, N), tuple(t.shape)))
            if not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous" % (name, tag))
            every.append((tag, key in written, t))
        shapes.append((M, N))
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
        plan = KronQuadListPlan(shapes, dev)
    elif plan.shapes != shapes or plan.device != dev:
        raise ValueError("%s: the lists have shapes %s on %s, the plan was made for %s on %s" % (name, shapes, dev, plan.shapes, plan.device))
    return plan, shapes


def update_precond_kron_quad_list_(Qls, Qrs, Ls, Gs, step, decay=0.95, *, plan=None):
    """Ql_i, Qr_i, L_i <- the QUAD step on G_i for every layer of the list, in place: six launches per group of the plan, the
    host reads nothing.  Bit-identical, layer by layer, to update_precond_kron_quad_.  Returns None.  plan: a KronQuadListPlan for
    these shapes (made per call when None: keep one across steps)."""
    name = "update_precond_kron_quad_list_"
    lists = dict(Ql=(Qls, lambda M, N: (M, M)), Qr=(Qrs, lambda M, N: (N, N)), L=(Ls, lambda M, N: (2,)), G=(Gs, lambda M, N: (M, N)))
    plan, _ = _operands(name, lists, {"Ql", "Qr", "L"}, plan)
    ptrs = [[t.data_ptr() for t in ts] for ts in (Qls, Qrs, Ls, Gs)] + [[0] * len(Gs)]
    plan.call("update", "psgd_kron_qlist_update_f32", ptrs, float(step), float(decay))


def precond_grad_kron_quad_list(Qls, Qrs, Gs, outs=None, *, plan=None):
    """[Ql_i (Ql_i G_i Qr_i) Qr_i for every layer], four launches per group of the plan.  outs (made when None) must not share
    memory with any operand.  Bit-identical, layer by layer, to precond_grad_kron_quad."""
    name = "precond_grad_kron_quad_list"
    lists = dict(Ql=(Qls, lambda M, N: (M, M)), Qr=(Qrs, lambda M, N: (N, N)), G=(Gs, lambda M, N: (M, N)))
    if outs is not None:
        lists["out"] = (outs, lambda M, N: (M, N))
    plan, _ = _operands(name, lists, {"out"}, plan)
    if outs is None:
        outs = [torch.empty_like(G) for G in Gs]
    ptrs = [[t.data_ptr() for t in ts] for ts in (Qls, Qrs)] + [[0] * len(Gs)] + [[t.data_ptr() for t in ts] for ts in (Gs, outs)]
    plan.call("apply", "psgd_kron_qlist_apply_f32", ptrs)
    return list(outs)
