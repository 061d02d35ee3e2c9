"""Row-sharded UVd preconditioner across the GPUs of one node (one process per GPU).

The flat parameter vector is split into contiguous row blocks: rank k owns rows
[k N / W, (k+1) N / W) of U, V, d, g, v, h and of the output.  Every sweep is local; the only
exchange is of the tiny reduced buffers between sweeps -- never of N-sized data.  An exchange
is ONE collective: an all-gather (RCCL over xGMI; `backend="nccl"` is RCCL on ROCm) of every
rank's fp64 send region, followed by a local fold of the W copies in rank order (a small HIP
kernel, psgd_*_fold_gathered_f64).  xGMI is point to point, the payloads are 8 B - 30 KB, so
the exchanges are latency-bound: what matters is how many there are per call, and that every
rank ends up with bit-identical reduced values (it folds the same copies in the same order,
whatever algorithm RCCL picks), so the r x r solves and step sizes redone on every rank agree.

    apply  (psgd.py:619-627):  sweep1 -> X(r sums) -> sweep2 -> X(r sums) -> sweep3            2 exchanges
    update (psgd.py:554-617):  [max -> X(2 maxima) -> scale]                                   (balance, :562-567)
                               sweep1 -> X(Gram, <= 30 KB) -> sweep2 -> X(1 maximum) -> sweep3  2 exchanges
    fused update -> apply:     sweep1 -> X(Gram) -> sweep2 -> X([pU | pV | qU | qV | max]) ->
                               r x r algebra -> last sweep (d update + whole apply)             2 exchanges

A bf16-stored state (U, V, d all bfloat16, r <= 32; psgd_uvd_bf16.hip) runs the staged forms of the bf16 kernels.  Its fused
step cannot use the algebraic short cut above -- the apply must see the STORED, rounded state, which exists only after the
rewrite sweep and the d update -- so it is the update's exchanges followed by the apply's:

    apply:                     sweep1 -> X(1) -> sweep2 -> X(2) -> sweep3                        2 exchanges
    update:                    [max -> X(10)] gram -> X(11) -> rewrite -> X(12) -> d update      2 exchanges
    fused update -> apply:     [max -> X(10)] gram -> X(11) -> rewrite -> X(12) ->
                               sweep1 (+ d update) -> X(1) -> sweep2 -> X(2) -> sweep3           4 exchanges

The stochastic-rounding stream is keyed by the GLOBAL element index: every rank passes row0, the number of rows on the ranks
before it (one set-up collective per (group, local row count), cached).

The two random branches of the reference (psgd.py:562, :588) must agree across ranks as well:
pass them explicitly, or let them be drawn from a branch generator whose state is synchronised
from rank 0 ONCE (first use); afterwards every rank draws the same numbers locally -- no
per-step broadcast and no host synchronisation.

The stage backend is an object with the methods of `HipStages` (the product backend: the C ABI
stage functions of include/psgd_hip.h).  tests/ injects a CPU backend to exercise this
choreography under gloo; there is no CPU backend in the product.
"""
import ctypes

import torch
import torch.distributed as dist

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd
from . import uvd_wide as _wide
from . import splu_wide as _splu_wide


class _HipStageBase:
    """What the HIP stage backends share: this rank's shard shape, the library, the device workspace, the reduced buffers as
    cached views into it and the exchange half of the stage interface (send / gather_buf / fold).  A subclass names the region
    query of its workspace layout (_region) and the fold kernel of its send regions (_fold)."""
    _region = _fold = None

    def __init__(self, device, n_local, r, workspace):
        self.device, self.N, self.r = device, int(n_local), int(r)
        self.lib = _lib.load()
        self.ws = workspace(device, self.N, self.r)
        self._fold_fn = getattr(self.lib, self._fold)
        self._views = {}
        self._out = None

    def _w(self):
        return self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream(self.device).cuda_stream

    def _view(self, which, stage, dtype, itemsize):
        key = (which, stage)
        if key not in self._views:
            off, cnt = self._region(which, stage, self.N, self.r)
            self._views[key] = self.ws[off:off + cnt * itemsize].view(dtype)
        return self._views[key]

    def send(self, stage):
        """This rank's fp64 contribution to the exchange after `stage` (a view into the workspace)."""
        return self._view(_lib.PSGD_WS_SEND_F64, stage, torch.float64, 8)

    def gather_buf(self, stage, world):
        key = ("gather", stage, world)
        if key not in self._views:
            self._views[key] = torch.empty(world * self.send(stage).numel(), dtype=torch.float64, device=self.device)
        return self._views[key]

    def fold(self, stage, gathered, world):
        """Fold the all-gathered send regions ([world][count], rank order) into this rank's workspace."""
        _lib.check(self._fold_fn(stage, gathered.data_ptr(), world, self.N, self.r, *self._w()), self._fold)


class HipStages(_HipStageBase):
    """Stage functions of the C ABI on this rank's shard; the reduced buffers are views into the
    device workspace (psgd_uvd_ws_region)."""
    _region, _fold = staticmethod(_lib.ws_region), "psgd_uvd_fold_gathered_f64"

    def __init__(self, device, n_local, r):
        if int(r) > _lib.UVD_MAX_RANK:
            raise _lib.PsgdHipError("the stage kernels take ranks up to %d; wider preconditioners go through uvd_wide.py "
                                    "(the sharded entry points route them there), got r = %d" % (_lib.UVD_MAX_RANK, int(r)))
        super().__init__(device, n_local, r, _psgd.uvd_workspace)

    def sums(self, stage):
        return self._view(_lib.PSGD_WS_SUMS_F64, stage, torch.float64, 8)

    def maxbuf(self, stage):
        return self._view(_lib.PSGD_WS_MAX_F32, stage, torch.float32, 4)

    def apply_sweep1(self, V, d, g):
        _lib.check(self.lib.psgd_uvd_apply_sweep1_f32(V.data_ptr(), d.data_ptr(), g.data_ptr(), self.N, self.r,
                                                      *self._w()), "apply_sweep1")

    def apply_sweep2(self, U, d, g):
        self._out = torch.empty_like(g)           # holds g1 = d.*g + U s1 until sweep 3
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_apply_sweep2_f32(U.data_ptr(), d.data_ptr(), g.data_ptr(), self._out.data_ptr(),
                                                      self.N, self.r, 1, wp, wn, st), "apply_sweep2")

    def apply_sweep3(self, U, V, d, g):
        out, self._out = self._out, None
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_apply_sweep3_f32(V.data_ptr(), d.data_ptr(), out.data_ptr(), self.N, self.r, 1,
                                                      wp, wn, st), "apply_sweep3")
        return out

    def balance_max(self, U, V):
        _lib.check(self.lib.psgd_uvd_balance_max_f32(U.data_ptr(), V.data_ptr(), self.N, self.r, *self._w()),
                   "balance_max")

    def balance_scale(self, U, V):
        _lib.check(self.lib.psgd_uvd_balance_scale_f32(U.data_ptr(), V.data_ptr(), self.N, self.r, *self._w()),
                   "balance_scale")

    def update_sweep1(self, U, V, d, v, h):
        _lib.check(self.lib.psgd_uvd_update_sweep1_f32(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(),
                                                       h.data_ptr(), self.N, self.r, *self._w()), "update_sweep1")

    def update_sweep2(self, U, V, d, v, h, step, tiny, update_U):
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_update_sweep2_f32(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(),
                                                       h.data_ptr(), self.N, self.r, float(step), float(tiny),
                                                       int(bool(update_U)), wp, wn, st), "update_sweep2")

    def update_sweep2_fused(self, U, V, d, v, h, g, step, tiny, update_U):
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_update_sweep2_fused_f32(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(),
                                                             h.data_ptr(), g.data_ptr(), self.N, self.r, float(step),
                                                             float(tiny), int(bool(update_U)), wp, wn, st),
                   "update_sweep2_fused")

    def fused_post(self, step, tiny, update_U):
        """r x r algebra of the fused step on the exchanged sums: s1', s2' of the apply on the updated state."""
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_fused_post_f32(self.N, self.r, float(step), float(tiny), int(bool(update_U)),
                                                    wp, wn, st), "fused_post")

    def fused_final(self, U, V, d, g, step, tiny, out=None):
        """last sweep of the fused step: d update + the whole apply; returns this rank's rows of the result (written to `out` when
        given: placement.UVdArena.out)."""
        out = torch.empty_like(g) if out is None else out
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_fused_final_f32(U.data_ptr(), V.data_ptr(), d.data_ptr(), g.data_ptr(),
                                                     out.data_ptr(), self.N, self.r, float(step), float(tiny),
                                                     wp, wn, st), "fused_final")
        return out

    def update_sweep3(self, d, step, tiny):
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_update_sweep3_f32(d.data_ptr(), self.N, self.r, float(step), float(tiny),
                                                       wp, wn, st), "update_sweep3")


class HipStagesBf16(_HipStageBase):
    """Stage functions of the bf16-state kernels (psgd_uvd_*_bf16) on this rank's shard: U, V, d bfloat16, vectors fp32.  The
    send regions are views into the device workspace (psgd_uvd_bf16_ws_region); the fold after every stage is what publishes
    the reduced values to the next one (with one rank as well)."""
    _region, _fold = staticmethod(_lib.uvd_bf16_ws_region), "psgd_uvd_bf16_fold_gathered_f64"

    def __init__(self, device, n_local, r):
        if int(r) > _lib.UVD_MAX_RANK:
            raise ValueError("a bfloat16 state supports ranks up to %d, got r = %d" % (_lib.UVD_MAX_RANK, int(r)))
        super().__init__(device, n_local, r, _psgd.uvd_bf16_workspace)

    def coefficients(self):
        """the r-vectors of the last r x r algebra (fp32 header words 8 .. 8 + 224: identical on every rank)"""
        return self.ws[32:32 + 224 * 4].view(torch.float32)

    def balance_max(self, U, V):
        _lib.check(self.lib.psgd_uvd_balance_max_bf16(U.data_ptr(), V.data_ptr(), self.N, self.r, *self._w()), "bf16 balance_max")

    def update_gram(self, U, V, d, v, h):
        _lib.check(self.lib.psgd_uvd_update_gram_bf16(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(), h.data_ptr(),
                                                      self.N, self.r, *self._w()), "bf16 update_gram")

    def update_rewrite(self, U, V, d, v, h, step, tiny, balance, update_U, mode, seed, row0):
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_update_rewrite_bf16(U.data_ptr(), V.data_ptr(), d.data_ptr(), v.data_ptr(), h.data_ptr(),
                                                         self.N, self.r, float(step), float(tiny), int(bool(balance)),
                                                         int(bool(update_U)), mode, seed, row0, wp, wn, st), "bf16 update_rewrite")

    def update_d(self, d, step, tiny, mode, seed, row0):
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_update_d_bf16(d.data_ptr(), self.N, self.r, float(step), float(tiny), mode, seed, row0,
                                                   wp, wn, st), "bf16 update_d")

    def apply_sweep1(self, V, d, g):
        _lib.check(self.lib.psgd_uvd_apply_sweep1_bf16(V.data_ptr(), d.data_ptr(), g.data_ptr(), self.N, self.r, *self._w()),
                   "bf16 apply_sweep1")

    def apply_sweep1_d(self, V, d, g, step, tiny, mode, seed, row0):
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_uvd_apply_sweep1_d_bf16(V.data_ptr(), d.data_ptr(), g.data_ptr(), self.N, self.r, float(step),
                                                         float(tiny), mode, seed, row0, wp, wn, st), "bf16 apply_sweep1_d")

    def apply_sweep2(self, U, d, g, out=None):
        self._out = torch.empty_like(g) if out is None else out           # holds g1 = d.*g + U s1 until sweep 3
        _lib.check(self.lib.psgd_uvd_apply_sweep2_bf16(U.data_ptr(), d.data_ptr(), g.data_ptr(), self._out.data_ptr(),
                                                       self.N, self.r, *self._w()), "bf16 apply_sweep2")

    def apply_sweep3(self, V, d):
        out, self._out = self._out, None
        _lib.check(self.lib.psgd_uvd_apply_sweep3_bf16(V.data_ptr(), d.data_ptr(), out.data_ptr(), self.N, self.r, *self._w()),
                   "bf16 apply_sweep3")
        return out


_backends = {}


def hip_backend_for(U):
    if not U.is_cuda:
        raise _lib.PsgdHipError("sharded UVd runs on HIP devices only (tensor is on %s); no CPU fallback" % U.device)
    key = (U.device.index, U.shape[0], U.shape[1], torch.cuda.current_stream(U.device).cuda_stream, U.dtype)
    if key not in _backends:
        cls = HipStagesBf16 if U.dtype == torch.bfloat16 else HipStages
        _backends[key] = cls(U.device, U.shape[0], U.shape[1])
    return _backends[key]


def shard_rows(n_global, rank, world):
    """Contiguous row block of rank `rank`: [lo, hi).  Block starts are multiples of 64 rows: every shard of an
    aligned [N, r] array stays 16-byte aligned for any r, and the per-row vectors (d, g, v, h) of a shard start on a
    256-byte boundary, so the tiles of the sweeps cover whole 128-byte lines."""
    per = -(-n_global // world)
    per = (per + 63) // 64 * 64
    lo = min(rank * per, n_global)
    hi = min(lo + per, n_global)
    return lo, hi


def reshard_uvd_state(state_dicts, new_row_counts):
    """The W state dicts of ONE row-sharded checkpoint (UVd.state_dict() of every rank, in any order) as W' dicts whose row
    counts are new_row_counts: offline, on the CPU, no process group.  The inputs must tile [0, num_params_global) without gap
    or overlap and agree on format, rank, dtypes, route, rounding, hyper, round_seed0 / round_step, param_round_seed0 /
    param_round_step (the parameters' rounding stream of param_rounding="stochastic": carried through), probe_seed0 / probe_step
    (the probe stream of preconditioner_fit="whitening": global, not per-rank, carried through unchanged), momentum_step, the keys of a guarded
    optimizer (nonfinite, skipped_steps, loss_scale, loss_scale_good_steps: carried through as they are) and branch_rng
    (ValueError naming what does not).  A dict that carries 'param_groups' is refused (ValueError): groups name a rank's own
    tensors, which a split by rows does not keep, and are rebuilt by the constructor.  momentum_buffer is split by rows as d is when every input dict has one (dropped otherwise).  new_row_counts must sum to num_params_global, and every entry but the last must be a multiple of 64
    (shards start at multiples of 64 rows, see shard_rows).  Output k holds rows [row0', row0' + n') with its own num_params
    and row0; its param_sizes is None (the new ranks' parameter lists are not known here), which UVd.load_state_dict skips.

    The stochastic-rounding stream is keyed by the global element index, so the resharded run stores the same codes up to the
    fp64 fold order of the exchanges."""
    name = "reshard_uvd_state"
    sds = sorted(state_dicts, key=lambda s: int(s["row0"]))
    if not sds:
        raise ValueError("%s: no state dicts" % name)
    if any("param_groups" in s for s in sds):
        raise ValueError("%s: a state dict carries 'param_groups'; parameter groups are made of a rank's own tensors and cannot be "
                         "resharded by rows: drop the key and pass param_groups= to the constructors of the new ranks" % name)
    first = sds[0]
    if first.get("format") != 1:
        raise ValueError("%s: 'format' is %r; this version reads format 1" % (name, first.get("format")))
    for key in ("format", "rank", "num_params_global", "state_dtype", "state_route", "state_rounding", "hyper", "round_seed0",
                "round_step", "param_round_seed0", "param_round_step", "probe_seed0", "probe_step", "momentum_step", "nonfinite", "skipped_steps", "loss_scale",
                "loss_scale_good_steps"):
        for s in sds[1:]:
            if s.get(key) != first.get(key):
                raise ValueError("%s: the state dicts disagree on %r (%r and %r)" % (name, key, first.get(key), s.get(key)))
    for s in sds:
        if not torch.equal(s["branch_rng"], first["branch_rng"]):
            raise ValueError("%s: the state dicts disagree on 'branch_rng'" % name)
        for k in ("U", "V", "d"):
            if s[k].dtype != first["U"].dtype:
                raise ValueError("%s: the state dicts disagree on the dtype of %r (%s and %s)" % (name, k, first["U"].dtype, s[k].dtype))
            if s[k].shape[0] != int(s["num_params"]):
                raise ValueError("%s: %r has %d rows where 'num_params' says %d" % (name, k, s[k].shape[0], int(s["num_params"])))
    total, pos = int(first["num_params_global"]), 0
    for s in sds:
        if int(s["row0"]) != pos:
            raise ValueError("%s: 'row0' = %d where the rows before it end at %d (%s)"
                             % (name, int(s["row0"]), pos, "a gap" if int(s["row0"]) > pos else "an overlap"))
        pos += int(s["num_params"])
    if pos != total:
        raise ValueError("%s: the rows end at %d but 'num_params_global' is %d" % (name, pos, total))
    counts = [int(c) for c in new_row_counts]
    if not counts or any(c < 1 for c in counts) or sum(counts) != total:
        raise ValueError("%s: new_row_counts %r must be positive and sum to num_params_global = %d" % (name, counts, total))
    if any(c % 64 for c in counts[:-1]):
        raise ValueError("%s: every entry of new_row_counts but the last must be a multiple of 64, got %r" % (name, counts))
    whole = {k: torch.cat([s[k] for s in sds], 0) for k in ("U", "V", "d")}
    if all(s.get("momentum_buffer") is not None for s in sds):      # the momentum buffer of class UVd: split by rows, as d is
        for s in sds:
            if s["momentum_buffer"].numel() != int(s["num_params"]):
                raise ValueError("%s: 'momentum_buffer' has %d elements where 'num_params' says %d"
                                 % (name, s["momentum_buffer"].numel(), int(s["num_params"])))
        whole["momentum_buffer"] = torch.cat([s["momentum_buffer"].reshape(-1) for s in sds], 0)
    out, lo = [], 0
    for c in counts:
        new = {k: v for k, v in first.items() if k not in ("U", "V", "d", "momentum_buffer")}
        new["hyper"] = dict(first["hyper"])
        new["branch_rng"] = first["branch_rng"].clone()
        for k in whole:
            new[k] = whole[k][lo:lo + c].clone()
        if "momentum_buffer" not in whole:
            new.pop("momentum_step", None)
        new["num_params"], new["row0"], new["param_sizes"] = c, lo, None
        out.append(new)
        lo += c
    return out


def _host_collectives(group):
    """gloo groups reduce host tensors (set-up-time scalars only; the per-step exchanges take device tensors on either backend)"""
    return dist.get_backend(group) == "gloo"


def global_rows(n_local, device, group=None):
    """Rows of the global flat vector = the sum of the ranks' row counts (psgd.py:686 across the group).  Set-up time only:
    one all-reduce and a host read."""
    on_host = _host_collectives(group) or device is None or torch.device(device).type == "cpu"
    t = torch.tensor([int(n_local)], dtype=torch.int64, device="cpu" if on_host else device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return int(t.item())


def global_norm(x, group=None):
    """2-norm of the global vector whose rows on this rank are x (the clip norm of psgd.py:753): the local sum of squares in fp64,
    ONE scalar all-reduce (every rank receives the same bits), the root as a device tensor of x's dtype -- no host read."""
    sq = torch.sum(x.to(torch.float64) ** 2).reshape(1)
    all_reduce_sum_f64_(sq, group)
    return torch.sqrt(sq[0]).to(x.dtype)


def all_reduce_sum_f64_(sq, group=None):
    """in-place SUM over the ranks of a contiguous fp64 tensor, on the current stream: the one scalar collective of the clip norm
    (global_norm above, and the fused step tail, which hands the kernel the reduced sum of squares)"""
    comm = _direct_comm(group, sq.device) if sq.is_cuda else None
    if comm is not None:
        comm.all_reduce_sum_f64(sq, torch.cuda.current_stream(sq.device).cuda_stream)
    else:
        dist.all_reduce(sq, op=dist.ReduceOp.SUM, group=group)
    return sq


def all_reduce_max_i32_(t, group=None):
    """in-place MAX over the ranks of an int32 tensor: the one extra collective of a guarded step of class UVd (every rank's "my
    v, h or g is not finite" bit; all ranks then skip the step or none does)"""
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return t


class BranchRng:
    """The two coin flips of update_precond_UVd_math_ (psgd.py:562 p = 0.01, :588 p = 0.5), agreed across ranks
    without a per-step exchange: the state of rank 0's generator is broadcast once, when the object is built (the only
    host synchronisation, at set-up time); afterwards every rank draws the same sequence locally on the host."""

    def __init__(self, generator=None, group=None, device=None):
        src_gen = generator if generator is not None else _psgd._branch_rng
        state = src_gen.get_state().clone()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            on_host = dist.get_backend(group) == "gloo" or device is None
            buf = state if on_host else state.to(device)
            dist.broadcast(buf, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            state = buf.cpu()
        self.gen = torch.Generator(device="cpu")
        self.gen.set_state(state)

    def draw(self, p):
        return bool(torch.rand((), generator=self.gen).item() < p)


_branch_rngs = {}


def branch_rng_for(generator, group, device):
    """One BranchRng per (generator object, group): synchronised from rank 0 on first use, local draws afterwards.
    All ranks must make the same sequence of calls with it (they do: the sharded calls are collective)."""
    key = (id(generator) if generator is not None else None, id(group) if group is not None else None)
    ent = _branch_rngs.get(key)
    if ent is None or ent[0] is not generator:
        ent = (generator, BranchRng(generator, group, device))        # the strong reference keeps id() unique
        _branch_rngs[key] = ent
    return ent[1]


CHECK_EXPLICIT_BRANCHES = False     # debugging aid: verify (one all-reduce + a host read per call) that every rank passed the
                                    # same explicit balance / update_U values; drawn values agree by construction


class _RcclDirect:
    """An RCCL communicator of our own for the exchanges, used through ctypes so that the all-gather is enqueued on the CALLER'S
    stream -- sweep, collective and fold are then one stream-ordered sequence.  torch.distributed runs NCCL / RCCL collectives on a
    stream of the process group: every exchange is a hop there and back (two cross-stream event waits), which measured 26-64 us per
    step on a 1.37-ms step.  The unique id travels over the existing torch.distributed group once, at set-up."""

    class _Uid(ctypes.Structure):
        _fields_ = [("internal", ctypes.c_byte * 128)]

    NCCL_FLOAT64 = 8        # ncclDataType_t

    def __init__(self, group, device):
        import os
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        self.lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        lib = self.lib
        lib.ncclGetErrorString.restype = ctypes.c_char_p
        lib.ncclGetUniqueId.argtypes = [ctypes.POINTER(self._Uid)]
        lib.ncclCommInitRank.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, self._Uid, ctypes.c_int]
        lib.ncclAllGather.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_void_p]
        lib.ncclAllReduce.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_void_p]
        lib.ncclCommDestroy.argtypes = [ctypes.c_void_p]
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        uid = self._Uid()
        if self.rank == 0:
            self._check(lib.ncclGetUniqueId(ctypes.byref(uid)), "ncclGetUniqueId")
        buf = torch.frombuffer(bytearray(bytes(uid)), dtype=torch.uint8).to(device)
        dist.broadcast(buf, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        ctypes.memmove(ctypes.byref(uid), bytes(buf.cpu().numpy().tobytes()), 128)
        self.comm = ctypes.c_void_p()
        with torch.cuda.device(device):
            self._check(lib.ncclCommInitRank(ctypes.byref(self.comm), self.world, uid, self.rank), "ncclCommInitRank")

    def _check(self, rc, what):
        if rc != 0:
            raise _lib.PsgdHipError("%s failed: %s" % (what, self.lib.ncclGetErrorString(rc).decode()))

    def all_gather_f64(self, send, recv, stream):
        """recv[rank k] = rank k's send (fp64, contiguous device tensors), enqueued on `stream` (a raw hipStream_t)"""
        self._check(self.lib.ncclAllGather(send.data_ptr(), recv.data_ptr(), send.numel(), self.NCCL_FLOAT64, self.comm, stream),
                    "ncclAllGather")


    def all_reduce_sum_f64(self, t, stream):
        """in place SUM over the ranks of a contiguous fp64 device tensor, enqueued on `stream`"""
        self._check(self.lib.ncclAllReduce(t.data_ptr(), t.data_ptr(), t.numel(), self.NCCL_FLOAT64, 0, self.comm, stream),
                    "ncclAllReduce")


_direct_comms = {}
EXCHANGES = {"count": 0}    # exchange points passed since import (tests count them per step whatever carries the collective)
DIRECT_RCCL = True      # exchanges of the HIP backend on RCCL groups go through _RcclDirect (PSGD_DIRECT_RCCL=0 or False: torch.distributed)


def _direct_comm(group, device):
    """the _RcclDirect of (group, device), or None when the exchange should go through torch.distributed (gloo groups, the switch
    off, or a set-up failure -- reported once)"""
    import os
    if not DIRECT_RCCL or os.environ.get("PSGD_DIRECT_RCCL", "1") == "0" or dist.get_backend(group) != "nccl":
        return None
    key = (id(group) if group is not None else None, torch.device(device).index, dist.get_world_size(group), dist.get_rank(group))
    if key not in _direct_comms:
        comm, why = None, None
        try:
            comm = _RcclDirect(group, device)
        except Exception as exc:                                            # noqa: BLE001 -- any failure means "use torch.distributed"
            why = exc
        # Every rank must take the SAME route from here on (a rank on torch.distributed and a rank on its own communicator would wait for
        # each other forever): one MIN over "my set-up worked" through the existing group; a single failure anywhere switches all ranks.
        ok = torch.tensor([1.0 if comm is not None else 0.0], device=device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=group)
        if float(ok.item()) < 1.0:
            if comm is not None:
                why = "another rank's set-up failed"
                try:
                    comm.lib.ncclCommDestroy(comm.comm)
                except Exception:                                            # noqa: BLE001
                    pass
                comm = None
            import warnings
            warnings.warn("psgd_tf_amd.sharded: direct RCCL communicator not available (%s); exchanges use torch.distributed" % (why,))
        _direct_comms[key] = (group, comm)                                  # (the strong reference keeps id() unique)
    return _direct_comms[key][1]


def _exchange(be, stage, group):
    """One exchange point = one collective: all-gather the send regions, fold them in rank order on every rank."""
    EXCHANGES["count"] += 1
    world = dist.get_world_size(group)
    send = be.send(stage)
    gathered = be.gather_buf(stage, world)
    comm = _direct_comm(group, send.device) if send.is_cuda else None
    if comm is not None:
        comm.all_gather_f64(send, gathered, torch.cuda.current_stream(send.device).cuda_stream)
    else:
        dist.all_gather_into_tensor(gathered, send, group=group)
    be.fold(stage, gathered, world)


def _wide_reduce(group):
    """Exchange of the wide-rank path (r > 32, uvd_wide.py): an all-reduce of one small stacked tensor per exchange point.
    Every rank receives the same bits (the collective computes each element once and distributes it).  "max": an all-gather and a
    NaN-propagating fold in rank order (a NaN maximum on any rank reaches every rank).  "summax" (the fused step's
    second exchange: 4r sums and one maximum in one buffer): an all-gather and a fold in rank order on every rank."""
    def reduce(t, op):
        if op == "summax":
            world = dist.get_world_size(group)
            t = t.contiguous()
            gathered = torch.empty(world * t.numel(), dtype=t.dtype, device=t.device)
            EXCHANGES["count"] += 1
            comm = _direct_comm(group, t.device) if (t.is_cuda and t.dtype == torch.float64) else None
            if comm is not None:
                comm.all_gather_f64(t, gathered, torch.cuda.current_stream(t.device).cuda_stream)
            else:
                dist.all_gather_into_tensor(gathered, t, group=group)
            g2 = gathered.view(world, -1)
            out = g2[0].clone()
            for k in range(1, world):                          # rank order: the same bits on every rank
                out[:-1] += g2[k][:-1]
                out[-1] = torch.maximum(out[-1], g2[k][-1])
            return out
        EXCHANGES["count"] += 1
        if op == "sum":
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
            return t
        # "max": a floating-point MAX all-reduce promises nothing about NaN (gloo's keeps the NaN of one operand and drops that of
        # the other: one rank's state would turn NaN while the other's stays finite).  All-gather and fold in rank order with
        # torch.maximum, which propagates NaN like tf.reduce_max: one collective, the same bits on every rank, signed operands
        # (the sparse-LU diagonals) included.
        world = dist.get_world_size(group)
        t = t.contiguous()
        gathered = torch.empty(world * t.numel(), dtype=t.dtype, device=t.device)
        dist.all_gather_into_tensor(gathered, t.reshape(-1), group=group)
        g2 = gathered.view(world, *t.shape)
        out = g2[0].clone()
        for k in range(1, world):
            out = torch.maximum(out, g2[k])
        return out
    return reduce


def _is_wide(U, backend):
    return backend is None and U.dim() == 2 and U.shape[1] > _lib.UVD_MAX_RANK


def _check_explicit_branches_agree(balance, update_U, device, group):
    """Explicit branch values must be the same on every rank (drawn ones are, by construction): the ranks would otherwise
    run different stage sequences and hang or mix branches.  One tiny MAX/MIN pair rides on a single all-reduce."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) < 2:
        return
    b, u = float(bool(balance)), float(bool(update_U))
    on_host = dist.get_backend(group) == "gloo"
    t = torch.tensor([b, -b, u, -u], dtype=torch.float32, device="cpu" if on_host else device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    t = t.cpu()
    if float(t[0]) != -float(t[1]) or float(t[2]) != -float(t[3]):
        raise ValueError("sharded UVd: ranks passed different explicit balance / update_U values")


_row0s = {}


def global_row0(n_local, device=None, group=None):
    """Rows on the ranks before this one = the global index of this rank's first row (the exclusive prefix of the ranks' row
    counts).  One all-gather and a host read the first time a (group, local row count) is seen; cached afterwards."""
    key = (id(group) if group is not None else None, int(n_local))
    ent = _row0s.get(key)
    if ent is None or ent[0] is not group:
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        on_host = _host_collectives(group) or device is None or torch.device(device).type == "cpu"
        dev = "cpu" if on_host else device
        counts = torch.empty(world, dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(counts, torch.tensor([int(n_local)], dtype=torch.int64, device=dev), group=group)
        ent = (group, int(counts.cpu()[:rank].sum().item()))              # (the strong reference keeps id() unique)
        _row0s[key] = ent
    return ent[1]


def _classify(name, U, V, d, cols, backend):
    """True when U, V, d are a bf16-stored state, False for an fp32 one (raises for a float16 or mixed state and for a bfloat16
    one of rank above 32).  Product backend: also the single-GPU entry points' checks on this rank's tensors (device, dtype,
    contiguity -- a strided operand is refused, not copied: a copy of a shard helps nobody -- and shapes): the stage kernels and
    the wide-rank chunks take raw pointers.  A backend passed in (the CPU doubles of tests/) takes CPU tensors as they come."""
    bf16 = _psgd._bf16_state(name, U, V, d)
    if backend is None:
        _psgd._require_hip(name, U, V, d, *cols, **(_psgd._BF16_STATE if bf16 else _psgd._FP32_STATE))
        _psgd._uvd_shapes(name, U, V, d, *cols)
    return bf16


def _resolve(name, bf16, U, balance, update_U, generator, rounding, rounding_seed, row0, group):
    """(balance, update_U, rounding mode, seed, row0) of an updating call, the same on every rank: what is None is drawn from the
    synchronised branch generator (psgd's _resolve_branches: one order of draws for the single-GPU and the sharded calls); row0
    (bf16 state only) defaults to the rows on the ranks before this one"""
    mode = _psgd._rounding_mode(name, bf16, rounding, rounding_seed, row0)
    if CHECK_EXPLICIT_BRANCHES and balance is not None and update_U is not None:
        _check_explicit_branches_agree(balance, update_U, U.device, group)
    balance, update_U, seed = _psgd._resolve_branches(balance, update_U, generator, mode, rounding_seed,
                                                      lambda: branch_rng_for(generator, group, U.device))
    if bf16:
        row0 = global_row0(U.shape[0], U.device, group) if row0 is None else int(row0)
        if row0 < 0:
            raise ValueError("%s: row0 must be >= 0, got %r" % (name, row0))
    return balance, update_U, mode, seed, row0


def _update_front(be, U, V, d, v, h, balance, group):
    """what the fp32 update and fused step start with: [max -> X(10) -> scale] -> sweep1 -> X(Gram)"""
    if balance:
        be.balance_max(U, V)
        _exchange(be, 10, group)
        be.balance_scale(U, V)
    be.update_sweep1(U, V, d, v, h)
    _exchange(be, 11, group)


def _bf16_update_front(be, U, V, d, v, h, step, tiny, balance, update_U, mode, seed, row0, group):
    """... and the bf16 ones: [max -> X(10)] -> Gram -> X(11) -> rewrite (which applies the balancing factors) -> X(12)"""
    if balance:
        be.balance_max(U, V)
        _exchange(be, 10, group)
    be.update_gram(U, V, d, v, h)
    _exchange(be, 11, group)
    be.update_rewrite(U, V, d, v, h, step, tiny, balance, update_U, mode, seed, row0)
    _exchange(be, 12, group)


def _bf16_apply_tail(be, U, V, d, g, group, out=None):
    _exchange(be, 1, group)
    be.apply_sweep2(U, d, g, out=out)
    _exchange(be, 2, group)
    return be.apply_sweep3(V, d)


def precond_grad_UVd_math(U, V, d, g, group=None, backend=None):
    """Sharded psgd.py:619-627 on this rank's rows; returns this rank's rows of the result.  2 exchanges (fp32 and bf16 state)."""
    bf16 = _classify("sharded precond_grad_UVd_math", U, V, d, (g,), backend)
    if _is_wide(U, backend):
        return _wide.precond_grad(U, V, d, g, _psgd.uvd_workspace, reduce=_wide_reduce(group))
    be = backend if backend is not None else hip_backend_for(U)
    be.apply_sweep1(V, d, g)
    if bf16:
        return _bf16_apply_tail(be, U, V, d, g, group)
    _exchange(be, 1, group)
    be.apply_sweep2(U, d, g)
    _exchange(be, 2, group)
    return be.apply_sweep3(U, V, d, g)


def update_precond_UVd_math_(U, V, d, v, h, step, tiny, *, balance=None, update_U=None, generator=None,
                             group=None, backend=None, rounding="nearest", rounding_seed=None, row0=None):
    """Sharded psgd.py:554-617 on this rank's rows (in place, returns None).  2 exchanges (+1 on the balance branch).
    A bfloat16 U, V, d (fp32 v, h; r <= 32) is updated by the bf16-state kernels: rounding / rounding_seed as in the single-GPU
    function (every rank must use the same seed: None draws it from the synchronised branch generator); row0 = the global index
    of this rank's first row (None: the exclusive prefix of the ranks' row counts, one set-up collective)."""
    name = "sharded update_precond_UVd_math_"
    bf16 = _classify(name, U, V, d, (v, h), backend)
    balance, update_U, mode, seed, row0 = _resolve(name, bf16, U, balance, update_U, generator, rounding, rounding_seed, row0, group)
    if _is_wide(U, backend):
        return _wide.update(U, V, d, v, h, float(step), float(tiny), balance, update_U, _psgd.uvd_workspace,
                            reduce=_wide_reduce(group))
    be = backend if backend is not None else hip_backend_for(U)
    if bf16:
        _bf16_update_front(be, U, V, d, v, h, step, tiny, balance, update_U, mode, seed, row0, group)
        be.update_d(d, step, tiny, mode, seed, row0)
        return None
    _update_front(be, U, V, d, v, h, balance, group)
    be.update_sweep2(U, V, d, v, h, step, tiny, update_U)
    _exchange(be, 12, group)
    be.update_sweep3(d, step, tiny)
    return None


def update_precond_UVd_math_and_precond_grad(U, V, d, v, h, g, step, tiny, *, balance=None, update_U=None,
                                             generator=None, group=None, backend=None, out=None, rounding="nearest",
                                             rounding_seed=None, row0=None):
    """Sharded fused update -> apply; returns this rank's rows of the preconditioned gradient.
    2 exchanges: the Gram; the 4r column sums of sweep 2 with max|nablaD| in one buffer (every rank, r > 32 included since
    round 6).  A bfloat16 state takes 4 exchanges (11, 12, 1, 2): the gradient is preconditioned with the state as it was
    STORED, so the apply's reductions cannot be derived from sums over the unrounded one; rounding, rounding_seed and row0 as in
    update_precond_UVd_math_.  out (a placed state passes its arena's output region): where to write the result; ranks above 32
    and an fp32 stage backend passed in ignore it."""
    name = "sharded update_precond_UVd_math_and_precond_grad"
    bf16 = _classify(name, U, V, d, (v, h, g) if out is None else (v, h, g, out), backend)
    balance, update_U, mode, seed, row0 = _resolve(name, bf16, U, balance, update_U, generator, rounding, rounding_seed, row0, group)
    if _is_wide(U, backend):
        # r > 32: the fused sequence on the wide-rank building blocks, 2 exchanges (+ 1 on the balance branch) like the ranks below
        return _wide.update_apply(U, V, d, v, h, g, float(step), float(tiny), balance, update_U, _psgd.uvd_workspace,
                                  reduce=_wide_reduce(group))
    be = backend if backend is not None else hip_backend_for(U)
    if bf16:
        if out is not None and (out.shape != g.shape or not out.is_contiguous()):
            raise ValueError("%s: out must be contiguous and shaped like g" % name)
        _bf16_update_front(be, U, V, d, v, h, step, tiny, balance, update_U, mode, seed, row0, group)
        be.apply_sweep1_d(V, d, g, step, tiny, mode, seed, row0)
        return _bf16_apply_tail(be, U, V, d, g, group, out)
    _update_front(be, U, V, d, v, h, balance, group)
    be.update_sweep2_fused(U, V, d, v, h, g, step, tiny, update_U)
    _exchange(be, 13, group)
    be.fused_post(step, tiny, update_U)
    if backend is not None:                                # (the fp32 stage interface of a backend passed in has no out)
        return be.fused_final(U, V, d, g, step, tiny)
    return be.fused_final(U, V, d, g, step, tiny, out=out)


# --------------------------------------------------------------------------- sparse LU (psgd.py:396-524), tail rows sharded
class HipSpluStages(_HipStageBase):
    """Stage functions of the C ABI on this rank's shard of the sparse-LU preconditioner: local tensors
    L12 = [L1; local rows of L2] ([r + n_local, r]), U12 = [U1, local columns of U2], local slices of l3 / u3, flat
    vectors [r corner entries (replicated); local slice of the tail].  Reduced buffers are views into the workspace."""
    _region, _fold = staticmethod(_lib.splu_ws_region), "psgd_splu_fold_gathered_f64"

    def __init__(self, device, n_local_total, r):
        super().__init__(device, n_local_total, r, _psgd._splu_workspace)

    def sums(self, stage):
        return self._view(0, stage, torch.float64, 8)

    def maxbuf(self):
        return self._view(1, 3, torch.float32, 4)

    def stage1(self, U12, x):
        _lib.check(self.lib.psgd_splu_stage1_f32(U12.data_ptr(), x.data_ptr(), self.N, self.r, *self._w()), "splu stage1")

    def apply_stage2(self, L12, l3, U12, u3, g):
        self._out = torch.empty_like(g)
        _lib.check(self.lib.psgd_splu_apply_stage2_f32(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(),
                                                       g.data_ptr(), self._out.data_ptr(), self.N, self.r, *self._w()),
                   "splu apply stage2")

    def apply_stage3(self, L12, l3, U12, u3):
        out, self._out = self._out, None
        _lib.check(self.lib.psgd_splu_apply_stage3_f32(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(),
                                                       out.data_ptr(), self.N, self.r, *self._w()), "splu apply stage3")
        return out

    def update_stage2(self, L12, l3, U12, u3, dx, dg):
        _lib.check(self.lib.psgd_splu_update_stage2_f32(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(),
                                                        dx.data_ptr(), dg.data_ptr(), self.N, self.r, *self._w()),
                   "splu update stage2")

    def update_stage3(self, L12, l3, U12, u3, dx, dg):
        _lib.check(self.lib.psgd_splu_update_stage3_f32(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(),
                                                        dx.data_ptr(), dg.data_ptr(), self.N, self.r, *self._w()),
                   "splu update stage3")

    def update_stage4(self, L12, l3, U12, u3, dx, dg, step, tiny, has_tail):
        new = [torch.empty_like(t) for t in (L12, l3, U12, u3)]
        wp, wn, st = self._w()
        _lib.check(self.lib.psgd_splu_update_stage4_f32(L12.data_ptr(), l3.data_ptr(), U12.data_ptr(), u3.data_ptr(),
                                                        dx.data_ptr(), dg.data_ptr(), new[0].data_ptr(), new[1].data_ptr(),
                                                        new[2].data_ptr(), new[3].data_ptr(), self.N, self.r, float(step),
                                                        float(tiny), int(bool(has_tail)), wp, wn, st), "splu update stage4")
        return tuple(new)


_splu_backends = {}


def _splu_backend_for(L12):
    if not L12.is_cuda:
        raise _lib.PsgdHipError("sharded sparse LU runs on HIP devices only (tensor is on %s); no CPU fallback" % L12.device)
    key = (L12.device.index, L12.shape[0], L12.shape[1], torch.cuda.current_stream(L12.device).cuda_stream)
    if key not in _splu_backends:
        _splu_backends[key] = HipSpluStages(L12.device, L12.shape[0], L12.shape[1])
    return _splu_backends[key]


def _refuse_bf16_splu(name, L12, l3, U12, u3):
    """Row sharding of a bf16-stored sparse-LU state does not exist: the state is classified as the single-GPU calls classify it
    (a float16 or mixed state raises TypeError there) and a bfloat16 one is refused before anything is launched."""
    if _psgd._splu_bf16_state(name, L12, l3, U12, u3):
        raise ValueError("%s: a bfloat16 sparse-LU state is not row-sharded (single-GPU update_precond_splu / precond_grad_splu "
                         "only); shard an fp32 state" % name)


def _splu_is_wide(L12, backend):
    return backend is None and L12.dim() == 2 and L12.shape[1] > _lib.SPLU_MAX_RANK


def precond_grad_splu(L12, l3, U12, u3, grad, group=None, backend=None):
    """Sharded psgd.py:483-524.  `grad` is this rank's flat vector [r corner entries; local tail slice]; returns the
    same layout (corner entries identical on every rank).  2 exchanges (r sums; 2r sums of which r are used).  Ranks above 32
    (the reference has no limit, psgd.py:420) run on column chunks (splu_wide.py) with an all-reduce per exchange."""
    _refuse_bf16_splu("sharded precond_grad_splu", L12, l3, U12, u3)
    if _splu_is_wide(L12, backend):
        _psgd._require_hip("sharded precond_grad_splu", L12, l3, U12, u3, grad)
        return _splu_wide.precond_grad(L12, l3, U12, u3, grad.reshape(-1), _psgd.uvd_workspace,
                                       reduce=_wide_reduce(group)).reshape(grad.shape)
    be = backend if backend is not None else _splu_backend_for(L12)
    be.stage1(U12, grad)
    _exchange(be, 1, group)
    be.apply_stage2(L12, l3, U12, u3, grad)
    _exchange(be, 2, group)
    return be.apply_stage3(L12, l3, U12, u3)


def update_precond_splu(L12, l3, U12, u3, dx, dg, step=0.01, tiny=None, has_tail=True, group=None, backend=None):
    """Sharded psgd.py:396-480 on this rank's rows; returns this rank's (L12, l3, U12, u3) (corner blocks identical on
    every rank).  3 exchanges: r sums, 2r sums, [r sums | 4 maxima].  has_tail: the global problem has tail rows."""
    tiny = _psgd._tiny if tiny is None else tiny
    _refuse_bf16_splu("sharded update_precond_splu", L12, l3, U12, u3)
    if _splu_is_wide(L12, backend):
        _psgd._require_hip("sharded update_precond_splu", L12, l3, U12, u3, dx, dg)
        return _splu_wide.update(L12, l3, U12, u3, dx.reshape(-1), dg.reshape(-1), float(step), float(tiny), _psgd.uvd_workspace,
                                 reduce=_wide_reduce(group))
    be = backend if backend is not None else _splu_backend_for(L12)
    be.stage1(U12, dg)
    _exchange(be, 1, group)
    be.update_stage2(L12, l3, U12, u3, dx, dg)
    _exchange(be, 2, group)
    be.update_stage3(L12, l3, U12, u3, dx, dg)
    _exchange(be, 3, group)
    return be.update_stage4(L12, l3, U12, u3, dx, dg, step, tiny, has_tail)
