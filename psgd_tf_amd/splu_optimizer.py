"""class SPLU: the sparse LU decomposition preconditioner as an optimizer.

The reference has no such class: its demo hand-writes the step (demo_usage_of_all_preconditioners.py:43-64) from
update_precond_splu / precond_grad_splu (psgd.py:396-524).  The interface and the step(closure) contract are those of class UVd
(psgd.py:630-764): the same argument names in the same order, so that a user swaps the class name; the defaults that differ are the
demo's (initial scale 0.1, preconditioner step 0.1).

    splu_initial_factors                                  the initial L12, l3, U12, u3 of the demo (:47-51)
    SPLU(...).step(closure)                               the optimizer

Both classes precondition ONE flat vector, so both are subclasses of _FlatStep, which owns step(), the flat-vector plumbing, the
stages of the constructor and the checkpoint skeleton.  This class supplies the state, _precondition, _flat_region (buffers this
object owns, on both tails) and the codec of its checkpoint keys; it has no group and no placed state.
"""
import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd

_FACTORS = ("L12", "l3", "U12", "u3")


def splu_initial_factors(num_params, rank, scale, dtype=torch.float32, device=None):
    """demo_usage_of_all_preconditioners.py:47-51 with s = scale on all four, as the demo has it: L12 = s [I_r; 0] ([N, r]),
    l3 = s 1 ([N - r, 1]), U12 = s [I_r, 0] ([r, N]), u3 = s 1.  Formed in float32 and rounded once to dtype."""
    N, r = int(num_params), int(rank)
    if not 1 <= r <= N:
        raise ValueError("splu_initial_factors: 1 <= rank <= num_params required, got rank %d for %d parameters" % (r, N))
    s = float(scale)
    L12 = torch.zeros(N, r, dtype=torch.float32, device=device)
    L12[:r] = s * torch.eye(r, dtype=torch.float32, device=device)
    l3 = s * torch.ones(N - r, 1, dtype=torch.float32, device=device)
    return L12.to(dtype), l3.to(dtype), L12.t().contiguous().to(dtype), l3.clone().to(dtype)


class SPLU(_psgd._FlatStep):
    """Sparse LU decomposition preconditioner (psgd.py:396-524) as an optimizer with the interface of class UVd.

    The preconditioner is P = Q'Q with Q = L U, L = [L1, 0; L2, diag(l3)] and U = [U1, U2; 0, diag(u3)], L1 and U1 r x r
    triangular, r = rank_of_modification; the state is L12 = [L1; L2] ([N, r]), l3, U12 = [U1, U2] ([r, N]) and u3, N the number
    of elements of the parameters with requires_grad (float32, bfloat16 or float16 tensors of one dtype on a ROCm device).
    rank_of_modification > N is a ValueError; == N is allowed (no diagonal tail).

    step(closure) is _FlatStep.step (psgd.py:692-764; see its docstring for the guard, the loss scale and the whitening fit) with
    the sparse-LU pair as the preconditioner: the coin of preconditioner_update_probability, an exact double backward or the finite
    difference of :716-727, v, h and g packed into three flat float32 vectors this object allocates once, update_precond_splu
    fed (dx, dg) = (v, h) with step lr_preconditioner, precond_grad_splu fed g (or the momentum buffer), the clip of :753-754
    and the parameter update.  It returns whatever the closure returns.  Every keyword that class UVd and class SPLU share
    (step_tail, momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval, param_rounding, param_rounding_seed,
    preconditioner_fit, probe_seed) means what it means there; step_tail="fused" gives the bits of step_tail="torch" under the
    same conditions.  preconditioner_fit="whitening" feeds (dx, dg) = (probe, raw gradient): ONE multi_randn launch fills the
    flat v buffer under uvd_step_rounding_seed(probe_seed0, probe_step).  The preconditioner arithmetic is float32 whatever
    the parameters' dtype, with the float32 tiny of the functions (psgd.py:22); the clip's tiny and the finite-difference scale
    follow the parameters' dtype (:682-683).

    How the state is held and what a step allocates depends on the route:

      float32 state, rank 1 .. 64      the C ABI directly: psgd_splu_update_f32 with its *_new pointers on the state itself (in
                                       place) and psgd_splu_apply_f32 into a flat output this object owns.  A step makes no
                                       state-sized allocation, no torch.cat of the lists and no copy of a factor.
      float32 state, rank > 64         the column chunks of splu_wide.py, as the functions run them: fresh factors come back
                                       from every update and replace the old ones (chunk copies besides).
      bfloat16 state, rank <= 32       state_dtype=torch.bfloat16, or "param" with bfloat16 parameters; a higher rank is a
                                       ValueError, a float16 state a TypeError.  psgd_splu_update_bf16 is pure and refuses
                                       aliased outputs: the new factors go to fresh tensors and the old ones are dropped --
                                       one bfloat16 copy of the state between steps, two during the update.  state_rounding
                                       is "stochastic" (default) or "nearest"; the stream of updating step k is
                                       uvd_step_rounding_seed(seed0, k), seed0 drawn from the generator behind the coins.

    state_dict() / load_state_dict() carry the four factors in their stored dtype, the hyper-parameters, the generator state
    and every counter and seed class UVd saves; a resumed run is bit-identical to the uninterrupted one.

    mixed_dtypes=True (keyword-only, False by default: nothing changes): the switch of class UVd, with its meaning there -- one
    optimizer over float32, bfloat16 and float16 tensors on both tails; state_dtype="param" is then a ValueError.

    Out of scope: group= (a row-sharded state; the staged entry points exist, the class does not drive them), placement=, a
    float32 checkpoint continued on a bfloat16 state, and any fused update -> apply."""

    def __init__(self, params_with_grad, rank_of_modification: int = 10, preconditioner_init_scale=0.1,
                 lr_params=0.01, lr_preconditioner=0.1,
                 grad_clip_max_norm=None, preconditioner_update_probability=1.0,
                 exact_hessian_vector_product: bool = True, generator=None, state_dtype=None, state_rounding=None,
                 step_tail="torch", momentum=0.0, weight_decay=0.0, nonfinite="propagate", loss_scale=None,
                 loss_scale_growth_interval=2000, *, param_rounding="nearest", param_rounding_seed=None,
                 preconditioner_fit="hessian", probe_seed=None, param_groups=None, mixed_dtypes=False):
        # the stages of _FlatStep with this class's checks between them; every check comes before anything touches a device
        N = self._init_params(params_with_grad, generator, param_rounding, preconditioner_fit, mixed_dtypes)
        store = torch.float32 if state_dtype is None else \
            _psgd._state_dtype_param("SPLU", self._mixed, self._dtype) if state_dtype == "param" else state_dtype
        if store == torch.float16:
            raise TypeError("SPLU: a float16 state is not supported (the native narrow state is bfloat16 only)")
        if store not in (torch.float32, torch.bfloat16):
            raise TypeError("SPLU: state_dtype must be None, 'param', float32 or bfloat16, got %r" % (state_dtype,))
        self._store_dtype, self._bf16 = store, store == torch.bfloat16
        r = self._rank = int(rank_of_modification)
        if r < 1:
            raise ValueError("SPLU: rank_of_modification must be >= 1, got %d" % r)
        if r > N:
            raise ValueError("SPLU: rank_of_modification must be <= the %d elements of the parameters, got %d" % (N, r))
        if self._bf16:
            if r > _lib.UVD_MAX_RANK:
                raise ValueError("SPLU: a bfloat16 state supports ranks up to %d, got %d" % (_lib.UVD_MAX_RANK, r))
            state_rounding = "stochastic" if state_rounding is None else state_rounding
            if state_rounding not in _psgd._ROUNDINGS:
                raise ValueError("SPLU: state_rounding must be 'stochastic' or 'nearest', got %r" % (state_rounding,))
        elif state_rounding is not None:
            raise ValueError("SPLU: state_rounding applies to a bfloat16 state only")
        self._state_rounding = state_rounding
        self._init_hypers(lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                          exact_hessian_vector_product, momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval)
        self._init_groups(param_groups)          # (None: nothing changes; _StepFeatures._init_groups)
        self._init_tail(step_tail)
        self._draw_seeds(self._bf16, param_rounding_seed, probe_seed)
        # the native kernels take a float32 state in place; anything else goes through the functions and gets fresh factors
        self._in_place = not self._bf16 and not _psgd._splu_chunked(r)
        self._L12, self._l3, self._U12, self._u3 = splu_initial_factors(N, r, float(preconditioner_init_scale), store, self._device)
        # v, h, g of :729-730, :747 and the preconditioned gradient: made once, written by every step
        self._flat_bufs = {k: torch.empty(N, dtype=torch.float32, device=self._device) for k in ("v", "h", "g")}
        self._out = torch.empty(N, dtype=torch.float32, device=self._device)

    @property
    def factors(self):
        """(L12, l3, U12, u3) as stored.  With a float32 state of rank <= 64 these tensors are updated in place for the life of
        the object; on the other routes every updating step replaces them."""
        return self._L12, self._l3, self._U12, self._u3

    def _flat_region(self, name, narrow=False):
        """v, h and g (the probe is drawn into v) live in the buffers this object owns, on both tails; the momentum buffer is
        _FlatStep's"""
        return self._flat_bufs.get("v" if name == "probe" else name)

    def _precondition(self, v, h, grad):
        """psgd.py:396-480 with (dx, dg) = (v, h) where v is given, then :483-524 on the flat gradient; returns the flat
        preconditioned gradient (this object's output buffer on the in-place route)."""
        if self._device.type != "cuda":
            raise _lib.PsgdHipError("SPLU.step runs on the HIP device only (the parameters are on %s); no CPU fallback" % self._device)
        state = self.factors
        if not self._in_place:
            if v is not None:
                kw = {}
                if self._bf16:
                    kw = dict(rounding=self._state_rounding,
                              rounding_seed=_psgd.uvd_step_rounding_seed(self._round_seed0, self._round_step))
                    self._round_step += 1
                state = _psgd.update_precond_splu(*state, [v], [h], float(self.lr_preconditioner), **kw)
                self._L12, self._l3, self._U12, self._u3 = state
            return _psgd.precond_grad_splu(*state, [grad])[0]
        N, r = self._L12.shape
        lib, ws, stream = _lib.load(), _psgd._splu_workspace(self._device, N, r), _psgd._stream_ptr(self._device)
        ptrs = [t.data_ptr() for t in state]
        if v is not None:
            rc = lib.psgd_splu_update_f32(*ptrs, v.data_ptr(), h.data_ptr(), *ptrs, N, r, float(self.lr_preconditioner),
                                          float(_psgd._tiny), ws.data_ptr(), ws.numel(), stream)
            _lib.check(rc, "psgd_splu_update_f32")
        rc = lib.psgd_splu_apply_f32(*ptrs, grad.data_ptr(), self._out.data_ptr(), N, r, ws.data_ptr(), ws.numel(), stream)
        _lib.check(rc, "psgd_splu_apply_f32")
        return self._out

    # ------------------------------------------------------------------------------------------------- checkpoint / resume
    def _state_encode(self, sd, host):
        """state_dict() of _FlatStep with "preconditioner": "splu" and L12, l3, U12, u3 in the stored dtype besides"""
        sd["preconditioner"] = "splu"
        sd.update((k, host(t)) for k, t in zip(_FACTORS, self.factors))

    def _state_judge(self, sd, name, need, same):
        """Dtypes: the stored dtype is a bitwise copy and a bfloat16 checkpoint widens exactly into a float32 state; a float32
        checkpoint into a bfloat16 state is a TypeError (out of scope)."""
        same("preconditioner", "splu")
        src = [need(k) for k in _FACTORS]
        for k, s, t in zip(_FACTORS, src, self.factors):
            if not isinstance(s, torch.Tensor) or tuple(s.shape) != tuple(t.shape):
                raise ValueError("%s: %r must be a tensor of shape %s" % (name, k, tuple(t.shape)))
        have = {s.dtype for s in src}
        if have != {self._store_dtype} and not (have == {torch.bfloat16} and self._store_dtype == torch.float32):
            raise TypeError("%s: a checkpoint of dtype %s cannot be loaded into a %s state: the same dtype and bfloat16 into float32 "
                            "are supported" % (name, sorted(str(x) for x in have), self._store_dtype))
        return src

    def _state_commit(self, src):
        for s, t in zip(src, self.factors):
            t.copy_(s)
