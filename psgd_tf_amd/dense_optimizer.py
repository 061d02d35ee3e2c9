"""class Dense: the dense preconditioner as an optimizer.

The reference has no such class: its first two scripts hand-write the step (hello_psgd.py:15-27,
demo_usage_of_all_preconditioners.py:26-41) from update_precond_dense / precond_grad_dense (psgd.py:26-63).  The interface and the
step(closure) contract are those of class SPLU without the three arguments of its state (rank_of_modification, state_dtype,
state_rounding): the same names in the same order, so that a user swaps the class name; the defaults are the demo's (initial scale
0.1, learning rate 0.01, preconditioner step 0.1).

    dense_initial_factor                                  the initial Q of the demo (:28) and of hello_psgd.py:8
    Dense(...).step(closure)                              the optimizer

The class preconditions ONE flat vector, so it is a subclass of _FlatStep, which owns step(), the flat-vector plumbing, the stages
of the constructor and the checkpoint skeleton.  This class supplies the state, _precondition, _flat_region (buffers this object
owns, on both tails) and the codec of its checkpoint keys; it has no group and no placed state.
"""
import torch

from . import _lib
from . import preconditioned_stochastic_gradient_descent as _psgd


def dense_initial_factor(num_params, scale, dtype=torch.float32, device=None):
    """demo_usage_of_all_preconditioners.py:28, hello_psgd.py:8: Q = scale I ([N, N]).  Formed in float32 and rounded once to
    dtype."""
    N = int(num_params)
    if N < 1:
        raise ValueError("dense_initial_factor: num_params must be >= 1, got %d" % N)
    return (float(scale) * torch.eye(N, dtype=torch.float32, device=device)).to(dtype)


class Dense(_psgd._FlatStep):
    """Dense preconditioner (psgd.py:26-63) as an optimizer with the interface of class SPLU.

    The preconditioner is P = Q'Q with ONE float32 N x N factor Q, N the number of elements of the parameters with requires_grad
    (float32, bfloat16 or float16 tensors of one dtype on a ROCm device).  The state takes 2 * 4 * N^2 bytes (see below), so the
    class is for small problems: N > max_num_params (keyword-only, 32768 by default: 8 GiB) is a ValueError before a device is
    touched; class SPLU and class UVd are the preconditioners whose state grows with N.

    step(closure) is _FlatStep.step (psgd.py:692-764; see its docstring for the guard, the loss scale and the whitening fit) with
    the dense pair as the preconditioner: the coin of preconditioner_update_probability, an exact double backward or the finite
    difference of :716-727, v, h and g packed into three flat float32 vectors this object allocates once, update_precond_dense
    fed (dx, dg) = (v, h) with step lr_preconditioner, precond_grad_dense fed g (or the momentum buffer), the clip of :753-754
    and the parameter update.  It returns whatever the closure returns.  Every keyword that class SPLU and class Dense share
    (step_tail, momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval, param_rounding, param_rounding_seed,
    preconditioner_fit, probe_seed) means what it means there; step_tail="fused" gives the bits of step_tail="torch" under the
    same conditions.  preconditioner_fit="whitening" feeds (dx, dg) = (probe, raw gradient): ONE multi_randn launch fills the
    flat v buffer under uvd_step_rounding_seed(probe_seed0, probe_step).  The preconditioner arithmetic is float32 whatever
    the parameters' dtype, with the float32 tiny of the functions (psgd.py:22); the clip's tiny and the finite-difference scale
    follow the parameters' dtype (:682-683).

    The state is TWO float32 N x N buffers, allocated once.  psgd_dense_update_f32 is pure (it refuses Qout == Q), so an updating
    step reads the current buffer and writes the new factor into the other one, and the two swap roles; psgd_dense_apply_f32
    writes into a flat output this object owns.  Both are called straight through the C ABI: a step makes no N^2-sized allocation
    (update_precond_dense returns a fresh N x N tensor from every call).  A step whose coin says "no update", and a step the
    guard skips, touches neither buffer.  The second buffer is never read before it has been written.

    Q is the current factor.  The tensor behind it ALTERNATES between the two buffers from one updating step to the next: what
    a caller read before a step holds the previous factor after it and is overwritten by the step after that.  Do not hold it
    across steps; read opt.Q again, or clone it.  A Q with a non-zero lower triangle (from a checkpoint) is accepted: the kernels
    keep the reference's full-matrix products, and the triangular solve of psgd.py:39 reads the upper triangle only.

    state_dict() / load_state_dict() carry "preconditioner": "dense" and "Q" (float32 [N, N], the current factor), the
    hyper-parameters, the generator state and every counter and seed class UVd saves ("rank" is 0); a resumed run is
    bit-identical to the uninterrupted one.  A load writes into the current buffer.

    mixed_dtypes=True (keyword-only, False by default: nothing changes): the switch of class UVd, with its meaning there -- one
    optimizer over float32, bfloat16 and float16 tensors on both tails.

    Out of scope: group= (a row-sharded state), placement=, a narrow (bfloat16) state, any fused update -> apply, and any
    in-place update."""

    def __init__(self, params_with_grad, preconditioner_init_scale=0.1, lr_params=0.01, lr_preconditioner=0.1,
                 grad_clip_max_norm=None, preconditioner_update_probability=1.0,
                 exact_hessian_vector_product: bool = True, generator=None,
                 step_tail="torch", momentum=0.0, weight_decay=0.0, nonfinite="propagate", loss_scale=None,
                 loss_scale_growth_interval=2000, *, param_rounding="nearest", param_rounding_seed=None,
                 preconditioner_fit="hessian", probe_seed=None, param_groups=None, mixed_dtypes=False,
                 max_num_params=32768):
        # the stages of _FlatStep with this class's check between them; every check comes before anything touches a device
        N = self._init_params(params_with_grad, generator, param_rounding, preconditioner_fit, mixed_dtypes)
        if N > int(max_num_params):
            raise ValueError("Dense: the parameters have %d elements and the state of the dense preconditioner would take 2 * 4 * N^2 "
                             "= %d bytes; max_num_params is %d.  psgd.SPLU and psgd.UVd hold a state that grows with N, not N^2"
                             % (N, 2 * 4 * N * N, int(max_num_params)))
        self._rank, self._store_dtype, self._state_rounding = 0, torch.float32, None
        self._init_hypers(lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                          exact_hessian_vector_product, momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval)
        self._init_groups(param_groups)          # (None: nothing changes; _StepFeatures._init_groups)
        self._init_tail(step_tail)
        self._draw_seeds(False, param_rounding_seed, probe_seed)
        # the two buffers of the factor: the update reads _Qs[_cur] and writes the other, which holds nothing until then
        self._Qs = [dense_initial_factor(N, preconditioner_init_scale, torch.float32, self._device),
                    torch.empty((N, N), dtype=torch.float32, device=self._device)]
        self._cur = 0
        # v, h, g of :729-730, :747 and the preconditioned gradient: made once, written by every step
        self._flat_bufs = {k: torch.empty(N, dtype=torch.float32, device=self._device) for k in ("v", "h", "g")}
        self._out = torch.empty(N, dtype=torch.float32, device=self._device)

    @property
    def Q(self):
        """The current factor, float32 [N, N].  The tensor alternates between this object's two buffers: every updating step
        returns the other one here.  Do not hold it across steps."""
        return self._Qs[self._cur]

    def _flat_region(self, name, narrow=False):
        """v, h and g (the probe is drawn into v) live in the buffers this object owns, on both tails; the momentum buffer is
        _FlatStep's"""
        return self._flat_bufs.get("v" if name == "probe" else name)

    def _precondition(self, v, h, grad):
        """psgd.py:26-42 with (dx, dg) = (v, h) where v is given, from the current buffer into the other one, which becomes the
        current one; then :45-63 on the flat gradient.  Returns this object's flat output buffer."""
        if self._device.type != "cuda":
            raise _lib.PsgdHipError("Dense.step runs on the HIP device only (the parameters are on %s); no CPU fallback" % self._device)
        N = self._out.numel()
        lib, ws, stream = _lib.load(), _psgd._dense_workspace(self._device, N), _psgd._stream_ptr(self._device)
        if v is not None:
            cur, other = self._Qs[self._cur], self._Qs[1 - self._cur]
            rc = lib.psgd_dense_update_f32(cur.data_ptr(), v.data_ptr(), h.data_ptr(), other.data_ptr(), N,
                                           float(self.lr_preconditioner), float(_psgd._tiny), ws.data_ptr(), ws.numel(), stream)
            _lib.check(rc, "psgd_dense_update_f32")
            self._cur = 1 - self._cur
        rc = lib.psgd_dense_apply_f32(self.Q.data_ptr(), grad.data_ptr(), self._out.data_ptr(), N, ws.data_ptr(), ws.numel(), stream)
        _lib.check(rc, "psgd_dense_apply_f32")
        return self._out

    # ------------------------------------------------------------------------------------------------- checkpoint / resume
    def _state_encode(self, sd, host):
        """state_dict() of _FlatStep with "preconditioner": "dense" and Q, the current factor, besides"""
        sd["preconditioner"] = "dense"
        sd["Q"] = host(self.Q)

    def _state_judge(self, sd, name, need, same):
        """Q must be a float32 tensor of shape [N, N]: a wrong shape is a ValueError, any other dtype a TypeError (a narrow state
        is out of scope).  Its lower triangle is not judged."""
        same("preconditioner", "dense")
        src, shape = need("Q"), tuple(self.Q.shape)
        if not isinstance(src, torch.Tensor) or tuple(src.shape) != shape:
            raise ValueError("%s: 'Q' must be a tensor of shape %s" % (name, shape))
        if src.dtype != torch.float32:
            raise TypeError("%s: 'Q' is %s; the state of class Dense is float32" % (name, src.dtype))
        return src

    def _state_commit(self, src):
        self.Q.copy_(src)
