"""class SPLU: the sparse LU decomposition preconditioner as an optimizer.

The reference has no such class: its demo hand-writes the step (demo_usage_of_all_preconditioners.py:43-64) from
update_precond_splu / precond_grad_splu (psgd.py:396-524).  The interface and the step(closure) contract are those of class UVd
(psgd.py:630-764): the same argument names in the same order, so that a user swaps the class name; the defaults that differ are the
demo's (initial scale 0.1, preconditioner step 0.1).

    splu_initial_factors                                  the initial L12, l3, U12, u3 of the demo (:47-51)
    SPLU(...).step(closure)                               the optimizer

Both classes precondition ONE flat vector, so everything of UVd.step but the preconditioner pair is the same code: SPLU takes
UVd.step and the flat-vector helpers behind it as they are (their row-sharded and placed-state branches are never entered: SPLU has
no group and no arena) and supplies _flat (buffers this object owns, on both tails), _draw_probe, _precondition and the checkpoint
pair.  The switches come from _StepFeatures, unchanged.
"""
import math

import numpy as np
import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd
from .multi_tail import MultiTailPlan

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


class SPLU(_psgd._StepFeatures):
    """Sparse LU decomposition preconditioner (psgd.py:396-524) as an optimizer with the interface of class UVd.

    The preconditioner is P = Q'Q with Q = L U, L = [L1, 0; L2, diag(l3)] and U = [U1, U2; 0, diag(u3)], L1 and U1 r x r
    triangular, r = rank_of_modification; the state is L12 = [L1; L2] ([N, r]), l3, U12 = [U1, U2] ([r, N]) and u3, N the number
    of elements of the parameters with requires_grad (float32, bfloat16 or float16 tensors of one dtype on a ROCm device).
    rank_of_modification > N is a ValueError; == N is allowed (no diagonal tail).

    step(closure) is UVd.step (psgd.py:692-764; see its docstring for the guard, the loss scale and the whitening fit) with the
    sparse-LU pair where the UVd pair was: the coin of preconditioner_update_probability, an exact double backward or the finite
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

    Out of scope: group= (a row-sharded state; the staged entry points exist, the class does not drive them), placement=, a
    float32 checkpoint continued on a bfloat16 state, and any fused update -> apply."""

    # the step and the flat-vector plumbing of class UVd, taken as they are (module docstring)
    step = _psgd.UVd.step
    _pack_scale, _momentum_buffer = _psgd.UVd._pack_scale, _psgd.UVd._momentum_buffer
    _grad_flat, _grad_cat, _guarded_grad = _psgd.UVd._grad_flat, _psgd.UVd._grad_cat, _psgd.UVd._guarded_grad
    _whitening_inputs = _psgd.UVd._whitening_inputs
    _HYPER_KEYS = _psgd.UVd._HYPER_KEYS
    _arena = None                                            # no placed state: the helpers take their plain branches

    def __init__(self, params_with_grad, rank_of_modification: int = 10, preconditioner_init_scale=0.1,
                 lr_params=0.01, lr_preconditioner=0.1,
                 grad_clip_max_norm=None, preconditioner_update_probability=1.0,
                 exact_hessian_vector_product: bool = True, generator=None, state_dtype=None, state_rounding=None,
                 step_tail="torch", momentum=0.0, weight_decay=0.0, nonfinite="propagate", loss_scale=None,
                 loss_scale_growth_interval=2000, *, param_rounding="nearest", param_rounding_seed=None,
                 preconditioner_fit="hessian", probe_seed=None):
        # every check comes before anything touches a device, in the order of class UVd's
        params = _psgd._flatten_params(params_with_grad)
        self._params = self._params_with_grad = [p for p in params if p.requires_grad]
        p0 = self._params_with_grad[0]
        self._dtype, self._device = p0.dtype, p0.device
        if self._dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError("SPLU: parameters must be float32, float16 or bfloat16, got %s" % self._dtype)
        self._param_sr = _psgd._param_rounding("SPLU", param_rounding, self._dtype)
        self._param_round_seed0, self._param_round_step = None, 0
        self._init_fit(preconditioner_fit)
        store = torch.float32 if state_dtype is None else self._dtype if state_dtype == "param" else state_dtype
        if store == torch.float16:
            raise TypeError("SPLU: a float16 state is not supported (the native narrow state is bfloat16 only)")
        if store not in (torch.float32, torch.bfloat16):
            raise TypeError("SPLU: state_dtype must be None, 'param', float32 or bfloat16, got %r" % (state_dtype,))
        self._store_dtype, self._bf16 = store, store == torch.bfloat16
        self._param_sizes, self._param_cumsizes = _psgd.uvd_param_index(self._params_with_grad)
        N, r = self._param_cumsizes[-1], int(rank_of_modification)
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
        self._state_rounding, self._generator = state_rounding, generator
        self._init_features(momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval)
        if step_tail not in ("torch", "fused"):
            raise ValueError("SPLU: step_tail must be 'torch' or 'fused', got %r" % (step_tail,))
        # the construction seeds, from the generator behind the coins, in the order of class UVd: state, parameters, probe
        if self._bf16:
            self._round_seed0, self._round_step = self._draw_seed(None), 0
        if self._param_sr:
            self._param_round_seed0 = self._draw_seed(param_rounding_seed)
        if self._whiten:
            self._probe_seed0 = self._draw_seed(probe_seed)
        self.lr_params = _psgd._Hyper(lr_params)
        self.lr_preconditioner = _psgd._Hyper(lr_preconditioner)
        self.grad_clip_max_norm = _psgd._Hyper(math.inf if grad_clip_max_norm is None else grad_clip_max_norm)
        self.preconditioner_update_probability = _psgd._Hyper(preconditioner_update_probability)
        self.exact_hessian_vector_product = _psgd._Hyper(bool(exact_hessian_vector_product))
        self._stamp = 0
        self._tiny = torch.finfo(self._dtype).tiny                                           # :682 (the clip's)
        self._delta_param_scale = torch.finfo(self._dtype).eps ** 0.5                        # :683
        self._fd_inv_scale = float(np.float32(1.0) / np.float32(self._delta_param_scale))
        self._tail = None
        if step_tail == "fused":
            if all(p.is_contiguous() and p.dtype == self._dtype for p in self._params_with_grad):
                self._tail = _psgd.UVdTailPlan(self._param_sizes, self._dtype, self._device)
            else:
                import warnings
                warnings.warn("SPLU: step_tail='fused' needs contiguous parameters of one dtype; this optimizer keeps the torch tail")
        # the native kernels take a float32 state in place; anything else goes through the functions and gets fresh factors
        self._in_place = not self._bf16 and not _psgd._splu_chunked(r)
        self._L12, self._l3, self._U12, self._u3 = splu_initial_factors(N, r, float(preconditioner_init_scale), store, self._device)
        # v, h, g of :729-730, :747 and the preconditioned gradient: made once, written by every step
        self._flat_bufs = {k: torch.empty(N, dtype=torch.float32, device=self._device) for k in ("v", "h", "g")}
        self._out = torch.empty(N, dtype=torch.float32, device=self._device)
        self._probe_plan = None

    @property
    def factors(self):
        """(L12, l3, U12, u3) as stored.  With a float32 state of rank <= 64 these tensors are updated in place for the life of
        the object; on the other routes every updating step replaces them."""
        return self._L12, self._l3, self._U12, self._u3

    def _row0(self):
        return 0

    def _flat(self, tensors, name, fd_scaled=False, inv=1.0, slot=None):
        """psgd.py:729-730, :747: the per-parameter tensors as one flat float32 vector, written into this object's buffer for it
        -- by one uvd_pack launch on the fused tail (fd_scaled: the division of :734-736 rides on it; slot: the guarded step's
        pack judges what it writes), by one torch.cat on the torch tail.  inv: 1 / loss_scale."""
        out = self._flat_bufs[name]
        if self._tail is not None:
            kw = {} if slot is None else dict(flag=self._tail.flags[slot:slot + 1], stamp=self._stamp)
            return _psgd.uvd_pack([_psgd._c(x) for x in tensors], out, self._pack_scale(fd_scaled, inv), plan=self._tail,
                                  role=name, **kw)
        parts = [torch.reshape(x, [-1]) for x in tensors]
        if all(x.dtype == torch.float32 for x in parts):
            torch.cat(parts, 0, out=out)
        else:
            out.copy_(torch.cat(parts, 0))
        return out if inv == 1.0 else out.mul_(inv)

    def _draw_probe(self):
        """v ~ N(0, I) of an updating whitening step: ONE multi_randn launch over one segment into the flat v buffer, on either
        tail, under uvd_step_rounding_seed(probe_seed0, probe_step).  Advances probe_step."""
        v = self._flat_bufs["v"]
        if self._probe_plan is None:
            self._probe_plan = MultiTailPlan([v.numel()], self._device)
        _psgd.multi_randn([v], self._next_probe_seed(), 0, plan=self._probe_plan)
        return v

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
    def state_dict(self):
        """Everything a bit-faithful resume needs, as a flat dict of CPU tensors and plain Python values: the keys of
        UVd.state_dict() with L12, l3, U12, u3 (in the stored dtype) in place of U, V, d, without the row-shard and state_route
        keys, and with "preconditioner": "splu".  Not saved, as there: the parameters and the global CUDA generator behind the
        draws of :713 / :721."""
        def host(t):
            return t.detach().to("cpu", copy=True).contiguous()
        sd = {"format": 1, "preconditioner": "splu", "rank": int(self._L12.shape[1]), "num_params": int(self._L12.shape[0]),
              "param_sizes": [int(s) for s in self._param_sizes], "state_dtype": str(self._store_dtype),
              "state_rounding": self._state_rounding if self._state_rounding is not None else "none",
              "hyper": {k: (bool if k == "exact_hessian_vector_product" else float)(getattr(self, k)) for k in self._HYPER_KEYS},
              "branch_rng": self._coin_generator().get_state().clone()}
        sd.update((k, host(t)) for k, t in zip(_FACTORS, self.factors))
        sd["hyper"]["momentum"], sd["hyper"]["weight_decay"] = float(self.momentum), float(self.weight_decay)
        if float(self.momentum) > 0.0:
            sd["momentum_buffer"], sd["momentum_step"] = host(self._momentum_buffer()), int(self._m_step)
        if self._bf16:
            sd["round_seed0"], sd["round_step"] = int(self._round_seed0), int(self._round_step)
        _psgd._param_rounding_encode(sd, self._param_sr, self._param_round_seed0, self._param_round_step)
        _psgd._probe_encode(sd, self._whiten, self._probe_seed0, self._probe_step)
        return _psgd._guard_encode(sd, self._guard, self.skipped_steps, self.loss_scale.value, self._good_steps)

    def load_state_dict(self, sd):
        """Restore what state_dict() saved, in place: the factors are copied into the tensors this object holds, the
        hyper-parameters are assigned, the generator behind the coins gets the saved state, and the momentum buffer, the seeds
        and the counters are restored under the rules of UVd.load_state_dict (a dict without a momentum buffer restarts the
        warm-up; a dict without the keys of a switch this object has on leaves its seed and starts the counter at 0).  Checked
        against this object (ValueError naming the key): format, preconditioner, rank, num_params, param_sizes.  Dtypes: the
        stored dtype is a bitwise copy and a bfloat16 checkpoint widens exactly into a float32 state; a float32 checkpoint
        into a bfloat16 state is a TypeError (out of scope).  A dict that is refused leaves this object as it was."""
        name = "SPLU.load_state_dict"

        def need(key):
            if key not in sd:
                raise ValueError("%s: the state dict has no %r" % (name, key))
            return sd[key]
        mine = {"format": 1, "preconditioner": "splu", "rank": int(self._L12.shape[1]), "num_params": int(self._L12.shape[0]),
                "param_sizes": [int(s) for s in self._param_sizes]}
        for key, want in mine.items():
            got = need(key)
            if (list(got) if key == "param_sizes" else got) != want:
                raise ValueError("%s: %r is %r in the state dict, %r in this optimizer" % (name, key, got, want))
        src = [need(k) for k in _FACTORS]
        for k, s, t in zip(_FACTORS, src, self.factors):
            if not isinstance(s, torch.Tensor) or tuple(s.shape) != tuple(t.shape):
                raise ValueError("%s: %r must be a tensor of shape %s" % (name, k, tuple(t.shape)))
        have = {s.dtype for s in src}
        if have != {self._store_dtype} and not (have == {torch.bfloat16} and self._store_dtype == torch.float32):
            raise TypeError("%s: a checkpoint of dtype %s cannot be loaded into a %s state: the same dtype and bfloat16 into float32 "
                            "are supported" % (name, sorted(str(x) for x in have), self._store_dtype))
        hyper = need("hyper")
        for k in self._HYPER_KEYS:
            if k not in hyper:
                raise ValueError("%s: 'hyper' has no %r" % (name, k))
        n = mine["num_params"]
        mbuf = sd.get("momentum_buffer")
        if mbuf is not None and (not isinstance(mbuf, torch.Tensor) or mbuf.dtype != torch.float32 or mbuf.numel() != n):
            raise ValueError("%s: 'momentum_buffer' must be a float32 tensor of %d elements" % (name, n))
        if mbuf is not None:
            need("momentum_step")
        # everything that can refuse the dict is judged before anything of this object changes
        gen = self._coin_generator()
        try:
            torch.Generator(device=gen.device).set_state(need("branch_rng"))
        except (RuntimeError, TypeError) as e:
            raise ValueError("%s: 'branch_rng' does not fit this optimizer's generator: %s" % (name, e))
        if self._bf16 and "round_seed0" in sd:
            need("round_step")
        param_round = _psgd._param_rounding_decode(name, sd, self._param_sr, self._param_round_seed0)
        probe = _psgd._probe_decode(sd, self._whiten, self._probe_seed0, name)
        if self._guard and sd.get("loss_scale") is not None and self.loss_scale.value is not None:
            S = float(sd["loss_scale"])
            if not (S > 0.0 and math.isfinite(S) and math.frexp(S)[0] == 0.5):
                raise ValueError("%s: 'loss_scale' must be a power of two, got %r" % (name, sd["loss_scale"]))
        gen.set_state(sd["branch_rng"])
        for k in self._HYPER_KEYS + tuple(k for k in ("momentum", "weight_decay") if k in hyper):
            getattr(self, k).assign(hyper[k])
        with torch.no_grad():
            if mbuf is not None:
                self._momentum_buffer().copy_(mbuf.reshape(-1))
                self._m_step = int(sd["momentum_step"])
            else:
                self._m_step = 0
                if float(self.momentum) > 0.0:
                    self._momentum_buffer().zero_()
            for s, t in zip(src, self.factors):
                t.copy_(s)
        if self._bf16 and "round_seed0" in sd:
            self._round_seed0, self._round_step = int(sd["round_seed0"]), int(sd["round_step"])
        (self._param_round_seed0, self._param_round_step), (self._probe_seed0, self._probe_step) = param_round, probe
        self._guard_decode(sd)
