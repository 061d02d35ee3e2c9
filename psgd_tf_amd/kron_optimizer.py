"""class Kron: the per-layer Kronecker-product preconditioner as an optimizer.

The reference has no such class: its Kron demos hand-write the step (mnist_with_lenet5.py:43-57, repeated in
lstm_with_xor_problem.py and the NMT demo).  The interface and the step(closure) contract are those of class UVd (psgd.py:630-764);
the arithmetic is that of mnist_with_lenet5.py:43-57, with the finite-difference Hessian-vector product of psgd.py:716-727.

    kron_layers, kron_operand_layers                      how the parameters become layers, and which run on bf16 operands
    kron_initial_factors                                  the initial factor pair of one layer
    Kron(...).step(closure)                               the optimizer

The list kernels of its step tail (multi_sumsq, multi_param_update, ...) are the functions of multi_tail.py, imported here by name:
the class calls them as globals of this module.  The switches it shares with class UVd are _StepFeatures of the UVd module.
"""
import contextlib
import math

import numpy as np
import torch

from . import kron as _kron
from . import preconditioned_stochastic_gradient_descent as _psgd
from .multi_tail import MultiTailPlan, _lists, _f32, _TINY, _HALF, _MIXED, _DTYPE_NAMES  # noqa: F401
from .multi_tail import multi_sumsq, multi_param_update, multi_diff_scale, multi_blend, multi_scale_check  # noqa: F401
from .multi_tail import multi_widen_check, multi_narrow, multi_randn, multi_vec_precond_update, multi_vec_precond_grad  # noqa: F401

_DELTA = float(np.float32(np.sqrt(np.float32(np.finfo(np.float32).eps))))      # psgd.py:683 for fp32 parameters
_FD_INV = float(np.float32(1.0) / np.float32(_DELTA))                           # the s of dG = (g' - g) s, dX = v s


def _dtype_constants(dtype):
    """(delta, s, tiny) of parameters of this dtype: the perturbation scale of psgd.py:683, s = float32(1) / float32(delta) of
    dG = (g' - g) s and dX = v s, and the tiny of the clip norm (psgd.py:682).  float32: the module's constants; bfloat16 /
    float16: formed as class UVd forms its _delta_param_scale, _fd_inv_scale and _tiny."""
    if dtype == _f32:
        return _DELTA, _FD_INV, _TINY
    delta = torch.finfo(dtype).eps ** 0.5
    return delta, float(np.float32(1.0) / np.float32(delta)), torch.finfo(dtype).tiny


# --------------------------------------------------------------------------- formats and initial factors
KRON_SIDES = ("dense", "norm", "scale")
KRON_PAIRS = (("dense", "dense"), ("dense", "norm"), ("dense", "scale"), ("norm", "dense"), ("norm", "scale"), ("scale", "dense"),
              ("scale", "norm"))                                   # the seven formats of the dispatcher (psgd.py:82-107)


def _format_pair(pair, what):
    if isinstance(pair, str):
        pair = (pair, pair)
    try:
        pair = tuple(pair)
    except TypeError:
        raise ValueError("%s: a preconditioner format is a side name or a (left, right) pair, got %r" % (what, pair))
    if len(pair) != 2 or any(s not in KRON_SIDES for s in pair):
        raise ValueError("%s: a preconditioner format is a (left, right) pair of %r, got %r" % (what, KRON_SIDES, pair))
    if pair not in KRON_PAIRS:
        raise ValueError("%s: the format %r does not exist: update_precond_kron / precond_grad_kron dispatch on the seven pairs of "
                         "psgd.py:82-107, where a normalization or scaling factor always faces a factor of another kind" % (what, pair))
    return pair


def kron_formats(preconditioner_formats, k):
    """`preconditioner_formats` of class Kron as a list of k (left, right) pairs.  Accepted: one side name ("dense" means
    ("dense", "dense")); one pair of two names, for every parameter (also when k == 2); or a sequence of k entries, each a pair or
    a side name."""
    f = preconditioner_formats
    if isinstance(f, str) or (isinstance(f, (tuple, list)) and len(f) == 2 and all(isinstance(s, str) for s in f)):
        return [_format_pair(f, "Kron")] * k
    try:
        f = list(f)
    except TypeError:
        raise ValueError("Kron: preconditioner_formats must be a side name, a (left, right) pair or one of either per parameter, got %r"
                         % (f,))
    if len(f) != k:
        raise ValueError("Kron: preconditioner_formats lists %d formats for %d parameters" % (len(f), k))
    return [_format_pair(p, "Kron (parameter %d)" % i) for i, p in enumerate(f)]


def _initial_factor(side, n, scale, device):
    """demo_usage_of_all_preconditioners.py:68-78"""
    if side == "dense":
        q = torch.eye(n, dtype=_f32, device=device)
    elif side == "scale":
        q = torch.ones(1, n, dtype=_f32, device=device)
    else:
        q = torch.stack([torch.ones(n, dtype=_f32, device=device), torch.zeros(n, dtype=_f32, device=device)])
    return q if scale == 1.0 else q * scale


def kron_initial_factors(shape, pair, init_scale=1.0, device=None, name="parameter"):
    """[Ql, Qr] of an (M, N) layer in the format `pair` (demo_usage_of_all_preconditioners.py:68-78): dense eye(n), scale ones(1, n),
    norm stack([ones(n), zeros(n)]); the LEFT factor is multiplied by init_scale.  Refuses a scaling side of length 1 and a
    normalization side of length 2: their factors are square, and the dispatcher, which knows a format by the factor shapes alone
    and tests for square first, would run them as dense factors."""
    pair = _format_pair(pair, "kron_initial_factors")
    M, N = (int(s) for s in shape)
    for side, n, where in ((pair[0], M, "left"), (pair[1], N, "right")):
        if n < 1:
            raise ValueError("Kron: %s of shape %s has an empty side" % (name, (M, N)))
        if (side == "scale" and n == 1) or (side == "norm" and n == 2):
            raise ValueError("Kron: %s of shape %s cannot take a %r factor on its %s side of length %d: that factor has shape (%d, %d), "
                             "square like a dense one, and update_precond_kron / precond_grad_kron, which tell the formats apart by "
                             "the factor shapes and test for square first, would treat it as dense -- use 'dense' for this side"
                             % (name, (M, N), side, where, n, n, n))
    return [_initial_factor(pair[0], M, float(init_scale), device), _initial_factor(pair[1], N, 1.0, device)]


def _factor_shape(side, n):
    return (n, n) if side == "dense" else (1, n) if side == "scale" else (2, n)


VECTOR_FORMAT = ("dense", "scale")      # a vector of length n is the reference's [1, n] layer in this format (psgd.py:87-88, :129-130)


def kron_layers(shapes, preconditioner_formats="dense", any_rank=False):
    """How class Kron(any_rank=...) lays parameters of these shapes out as layers: one (kind, (M, N), (left, right)) per parameter.
        rank 2                     "matrix", the shape itself, the format asked for
        rank >= 3                  "matrix", (shape[0], prod(shape[1:])): the usual folding of a conv kernel
        rank 1, length n >= 2      "vector", (1, n), ("dense", "scale"): Ql is 1 x 1, Qr is [1, n]
        rank 0, rank 1 length 1    "scalar", (1, 1), ("dense", "dense"): a scaling side of length 1 does not exist
    One format given for all parameters applies to the matrix layers only.  In a per-parameter list the entry of a vector must be
    ("dense", "scale") or the default name "dense", that of a scalar ("dense", "dense") or "dense"; anything else is a ValueError
    that names the parameter.  With any_rank off, or when every shape has rank 2, this is kron_formats on the shapes as they are."""
    shapes = [tuple(int(n) for n in s) for s in shapes]
    k = len(shapes)
    if not any_rank or all(len(s) == 2 for s in shapes):
        return [("matrix", s, f) for s, f in zip(shapes, kron_formats(preconditioner_formats, k))]
    f = preconditioner_formats
    if isinstance(f, str) or (isinstance(f, (tuple, list)) and len(f) == 2 and all(isinstance(s, str) for s in f)):
        entries = [None] * k
        matrix_pair = _format_pair(f, "Kron")
    else:
        try:
            entries = list(f)
        except TypeError:
            raise ValueError("Kron: preconditioner_formats must be a side name, a (left, right) pair or one of either per parameter, "
                             "got %r" % (f,))
        if len(entries) != k:
            raise ValueError("Kron: preconditioner_formats lists %d formats for %d parameters" % (len(entries), k))
        matrix_pair = None

    def fixed(i, entry, kind, pair):
        """the entry of a vector or scalar layer: nothing, the default name, or the one pair such a layer has"""
        if entry is None or entry == "dense":
            return pair
        if isinstance(entry, (tuple, list)) and tuple(entry) == pair:
            return pair
        raise ValueError("Kron: parameter %d (shape %s) is a %s layer; its preconditioner format is %r (or the default name 'dense'), "
                         "got %r" % (i, shapes[i], kind, pair, entry))
    out = []
    for i, (s, e) in enumerate(zip(shapes, entries)):
        if len(s) >= 2:
            shape2d = s if len(s) == 2 else (s[0], int(np.prod(s[1:], dtype=np.int64)))
            out.append(("matrix", shape2d, matrix_pair if e is None else _format_pair(e, "Kron (parameter %d)" % i)))
        elif len(s) == 1 and s[0] >= 2:
            out.append(("vector", (1, s[0]), fixed(i, e, "vector", VECTOR_FORMAT)))
        else:
            out.append(("scalar", (1, s[0] if s else 1), fixed(i, e, "scalar", ("dense", "dense"))))
    return out


# operand_min_dim of class Kron when none is given: the smallest short side at which narrow + bf16 update + narrow + bf16 apply beat
# the fp32 update + apply by more than the spread of the legs, on the square and on the 1:4 layer, and at every larger side measured
# (profiles/kron_class_operands.txt: 768 x 768 by 36 us of 431, 768 x 3072 by 54 us of 892; at 512 x 512 the legs are not resolved,
# at 256 x 256 the fp32 route wins).
OPERAND_MIN_DIM = 768


def _operands_dtype(operands):
    """`operands` of class Kron: None, or torch.bfloat16 for "bfloat16" / torch.bfloat16; ValueError otherwise"""
    if operands is None:
        return None
    if operands is torch.bfloat16 or (isinstance(operands, str) and operands == "bfloat16"):
        return torch.bfloat16
    raise ValueError("Kron: operands must be None, 'bfloat16' or torch.bfloat16, got %r" % (operands,))


def _operand_min_dim(operand_min_dim):
    if isinstance(operand_min_dim, bool) or not isinstance(operand_min_dim, (int, np.integer)) or operand_min_dim < 1:
        raise ValueError("Kron: operand_min_dim must be an integer >= 1, got %r" % (operand_min_dim,))
    return int(operand_min_dim)


def kron_operand_layers(layer_shapes, formats, operands=None, operand_min_dim=OPERAND_MIN_DIM):
    """The indices of the OPERAND LAYERS of class Kron(operands=..., operand_min_dim=...): the layers whose factor update and
    apply run on the bf16-operand kernels.  layer_shapes: the (M, N) of every layer, as kron_layers gives them (with any_rank the
    [shape[0], prod(shape[1:])] view, not the parameter's own shape); formats: one (left, right) pair per layer.  A layer is chosen
    when operands is bfloat16, its format is ("dense", "dense") and min(M, N) >= operand_min_dim; sizes that are no multiple of 8
    qualify (the functional calls pad them).  Vector layers (("dense", "scale")), the other sparse formats and smaller layers are
    never chosen; operands=None gives []."""
    op = _operands_dtype(operands)
    min_dim = _operand_min_dim(operand_min_dim)
    layer_shapes, formats = list(layer_shapes), list(formats)
    if len(layer_shapes) != len(formats):
        raise ValueError("kron_operand_layers: %d layer shapes and %d formats" % (len(layer_shapes), len(formats)))
    if op is None:
        return []
    out = []
    for i, (s, f) in enumerate(zip(layer_shapes, formats)):
        if len(s) != 2:
            raise ValueError("kron_operand_layers: layer %d has shape %r; a layer shape is (M, N)" % (i, tuple(s)))
        if _format_pair(f, "kron_operand_layers (layer %d)" % i) == ("dense", "dense") and min(int(s[0]), int(s[1])) >= min_dim:
            out.append(i)
    return out


# --------------------------------------------------------------------------- checkpoint, host part
_HYPER_KEYS = _psgd._StepFeatures._HYPER_KEYS


def _encode_state(factors, formats, shapes, hyper, rng_state):
    """state_dict() of class Kron from its parts (CPU clones of the factors; plain Python values otherwise)"""
    return {"format": 1, "kind": "kron",
            "factors": [[q.detach().to("cpu", copy=True).contiguous() for q in pair] for pair in factors],
            "preconditioner_formats": [list(p) for p in formats], "param_shapes": [list(map(int, s)) for s in shapes],
            "hyper": {k: (bool if k == "exact_hessian_vector_product" else float)(hyper[k]) for k in _HYPER_KEYS},
            "rng": rng_state.clone()}


def _decode_state(sd, formats, shapes, layer_shapes=None):
    """the checks of load_state_dict(): returns (factors, hyper, rng_state) of a dict that fits an optimizer with these formats and
    parameter shapes; ValueError naming the key otherwise.  layer_shapes: the (M, N) of every layer where they are not the
    parameters' own shapes (Kron(any_rank=True): 'param_shapes' holds the true shapes, the factors have those of the layers)"""
    name = "Kron.load_state_dict"
    layer_shapes = shapes if layer_shapes is None else layer_shapes

    def need(key):
        if key not in sd:
            raise ValueError("%s: the state dict has no %r" % (name, key))
        return sd[key]
    if need("format") != 1 or need("kind") != "kron":
        raise ValueError("%s: 'format' / 'kind' are %r / %r; this version reads format 1 of kind 'kron'"
                         % (name, sd.get("format"), sd.get("kind")))
    if [list(p) for p in need("preconditioner_formats")] != [list(p) for p in formats]:
        raise ValueError("%s: 'preconditioner_formats' is %r in the state dict, %r in this optimizer"
                         % (name, sd["preconditioner_formats"], [list(p) for p in formats]))
    if [list(map(int, s)) for s in need("param_shapes")] != [list(map(int, s)) for s in shapes]:
        raise ValueError("%s: 'param_shapes' is %r in the state dict, %r in this optimizer"
                         % (name, sd["param_shapes"], [list(map(int, s)) for s in shapes]))
    factors = need("factors")
    if len(factors) != len(shapes):
        raise ValueError("%s: 'factors' holds %d pairs for %d parameters" % (name, len(factors), len(shapes)))
    for i, (pair, fmt, (M, N)) in enumerate(zip(factors, formats, layer_shapes)):
        want = (_factor_shape(fmt[0], M), _factor_shape(fmt[1], N))
        if len(pair) != 2 or any(not isinstance(q, torch.Tensor) or q.dtype != _f32 or tuple(q.shape) != w
                                 for q, w in zip(pair, want)):
            raise ValueError("%s: 'factors'[%d] must be two float32 tensors of shapes %s and %s" % (name, i, want[0], want[1]))
    hyper = need("hyper")
    for k in _HYPER_KEYS:
        if k not in hyper:
            raise ValueError("%s: 'hyper' has no %r" % (name, k))
    return factors, hyper, need("rng")


def _encode_features(sd, momentum, weight_decay, buffers=None, momentum_step=0, guard=False, skipped_steps=0, loss_scale=None,
                     good_steps=0):
    """the keys that momentum, weight decay and the guard add to a state dict, as class UVd names them: 'hyper' always gains
    momentum and weight_decay; momentum_buffers (CPU clones, one per parameter) and momentum_step only when momentum > 0;
    nonfinite, skipped_steps, loss_scale, loss_scale_good_steps only when the optimizer is guarded.  Returns sd."""
    sd["hyper"]["momentum"], sd["hyper"]["weight_decay"] = float(momentum), float(weight_decay)
    if float(momentum) > 0.0:
        sd["momentum_buffers"] = [m.detach().to("cpu", copy=True).contiguous() for m in buffers]
        sd["momentum_step"] = int(momentum_step)
    return _psgd._guard_encode(sd, guard, skipped_steps, loss_scale, good_steps)


# the checkpoint keys of the probe stream: one implementation for both classes (_StepFeatures of the UVd module)
_probe_encode, _probe_decode = _psgd._probe_encode, _psgd._probe_decode


def _decode_features(sd, shapes):
    """the optional keys of _encode_features, checked: (momentum buffers or None, momentum_step).  A dict from before them has
    none and is valid."""
    name = "Kron.load_state_dict"
    bufs = sd.get("momentum_buffers")
    if bufs is None:
        return None, 0
    if len(bufs) != len(shapes) or any(not isinstance(m, torch.Tensor) or m.dtype != _f32 or tuple(m.shape) != tuple(s)
                                       for m, s in zip(bufs, shapes)):
        raise ValueError("%s: 'momentum_buffers' must be one float32 tensor per parameter, of the parameter's shape" % name)
    if "momentum_step" not in sd:
        raise ValueError("%s: the state dict has 'momentum_buffers' but no 'momentum_step'" % name)
    return bufs, int(sd["momentum_step"])


# --------------------------------------------------------------------------- the optimizer
def _flatten(params_with_grad):
    """the flattening order of class UVd (lists / tuples depth first, dict keys sorted); anything else is a leaf for the checks"""
    if isinstance(params_with_grad, dict):
        return [q for k in sorted(params_with_grad) for q in _flatten(params_with_grad[k])]
    if isinstance(params_with_grad, (list, tuple)):
        return [q for p in params_with_grad for q in _flatten(p)]
    return [params_with_grad]


class Kron(_psgd._StepFeatures):
    """Kronecker-product preconditioned SGD, one factor pair per rank-2 parameter: the train_step of mnist_with_lenet5.py:43-57 behind
    the interface of class UVd.  Shared with the flat classes through _StepFeatures, not written here: the switches and
    _init_step_hypers, _step_route, _closure_gradients, _tail_coefficients, _fused_tail_kwargs.  This class's own: _screen, _judge,
    _widen, _blend, _update_factors, _precondition.

    params_with_grad: contiguous rank-2 tensors of one dtype (float32, bfloat16 or float16) with requires_grad=True on one HIP
    device (nested lists / dicts are flattened as class UVd does).  preconditioner_formats: "dense", a (left, right) pair of "dense" / "norm" / "scale", or one of either per
    parameter.  The five hyper-parameters are _Hyper objects (.assign()).  grad_clip_max_norm=None: no clipping.
    layer_batch: the per-layer calls of a step run inside kron.layer_batch() blocks (one for the updates, one for the applies).
    step_tail: "torch" = per-tensor torch expressions around the preconditioner calls; "fused" = the list kernels (at most five
    launches whatever the number of layers).  Both round alike.
    generator: draws the update coin, then the perturbations in parameter order, each step; a CPU or a device generator.  None: the
    coin comes from the module's branch generator (psgd.manual_seed), the perturbations from the global device generator, as in
    class UVd.

    momentum, weight_decay (off by default; _Hyper objects): one fp32 buffer per parameter, m <- beta_k m + (1 - beta_k) g with the
    warm-up beta_k = min(k / (k + 1), momentum) of class UVd (uvd_momentum_coefficients), and m takes the place of g in
    precond_grad_kron; decoupled weight decay adds float32(float32(lr_eff weight_decay) p) to what the update subtracts.
    nonfinite="skip": a step whose gradients, Hessian-vector products (perturbed gradients) or probe vectors hold +-Inf or NaN
    changes nothing (skipped_steps, last_step_skipped).  loss_scale (needs "skip"): None, a power of two, or "dynamic" (starts at
    2^16, uvd_loss_scale_next with loss_scale_growth_interval); a _Hyper that holds the CURRENT scale.  See step().

    Parameters of dtype T = bfloat16 or float16 (all of one optimizer share T): the factors, the momentum buffers, dX, dG, the
    gradients given to precond_grad_kron, the preconditioned gradients and the clip norm stay float32; the gradients, the second
    list and the probe vectors are widened once per step, and only the update is rounded in T, with the chain of class UVd's
    psgd_uvd_param_update_multi_wd (see step()).  delta = finfo(T).eps ** 0.5 and tiny = finfo(T).tiny as in class UVd
    (psgd.py:682-683).  A checkpoint has no dtype in it: a dict saved from a float32 optimizer loads into a bfloat16 one of the same
    shapes and back.

    any_rank=True (keyword-only, off by default: nothing changes) takes the parameters of an ordinary torch.nn.Module, laid out as
    kron_layers says.  A rank-1 parameter of length n >= 2 is a VECTOR LAYER: the reference's layer of shape [1, n] in the
    ("dense", "scale") format (psgd.py:87-88, :129-130), Ql of shape (1, 1) equal to preconditioner_init_scale and Qr = ones(1, n)
    -- a diagonal preconditioner with one scalar of balance; a per-parameter format list may name it ("dense", "scale") or "dense"
    and nothing else.  Rank 0 and rank 1 of length 1 are [1, 1] layers in ("dense", "dense").  Rank >= 3 is the matrix layer
    [shape[0], prod(shape[1:])] in the format asked for, a view that shares the parameter's storage (the usual folding of a conv
    kernel).  One format given for all parameters applies to the matrix layers only.  factors, state_dict() and
    load_state_dict() carry every layer's pair in parameter order; 'param_shapes' holds the parameters' true shapes.  Every other
    switch keeps its meaning; the step-tail kernels work on element counts and do not see the shapes.
    vector_route="list" (default): all vector layers of a step are updated by ONE launch and applied by ONE launch
    (multi_vec_precond_update, in place, and multi_vec_precond_grad; one workgroup per vector, so a vector of a million elements is
    correct but slow).  vector_route="layer": they go through update_precond_kron / precond_grad_kron on [1, n] views like any
    other layer, about ten launches each -- the comparison leg.  The two routes round differently and need not agree bit for bit.

    operands="bfloat16" (or torch.bfloat16; keyword-only, None by default: nothing changes) runs the large (dense, dense) layers on
    the bf16-operand Kron kernels (psgd_kron_dd_update_bf16, psgd_kron_dd_apply_bf16[_prepared]), whatever the parameters' dtype.
    A layer is an OPERAND LAYER when its format is ("dense", "dense") and min(M, N) >= operand_min_dim on its layer shape (with
    any_rank the [shape[0], prod(shape[1:])] view); kron_operand_layers is the rule, opt.operand_layers the indices chosen.  Sizes
    that are no multiple of 8 qualify (the functional calls pad them); vector layers, the sparse formats and smaller layers keep
    the fp32 path.  For an operand layer step 4 is update_precond_kron(Ql, Qr, bf16(dX), bf16(dG), lr_q) and step 5
    precond_grad_kron(Ql, Qr, bf16(g)), g the momentum buffer after the blend when momentum is on; the factors stay float32, the
    preconditioned gradient is a bfloat16 tensor, and steps 6 and 7 read it as float(pg) and round as they always do (see step()).
    The fused tail keeps three bfloat16 buffers per operand layer, in the layer's shape, for the gradient, dX and dG: 6 bytes per
    element of those layers (the torch tail makes them per step).  operands is a constructor choice like step_tail: it is not in
    state_dict(), and a checkpoint loads into an optimizer with either setting.
    operand_min_dim defaults to 768 (OPERAND_MIN_DIM): the smallest short side at which the bf16 route (narrow + update + narrow +
    apply) beats the fp32 update + apply by more than the spread of the legs on both the square and the 1:4 layer, and at every
    larger side measured (1024, 2048); at 512 the square layer is not resolved and at 256 the fp32 route wins
    (profiles/kron_class_operands.txt).
    Known limitation: kron.py keeps ONE prepared bf16 factor slot per (device, M, N, stream), so several operand layers of one
    shape convert their factors again on every apply of a step that did not update them.

    param_rounding="stochastic" (keyword-only, "nearest" by default: nothing changes; bfloat16 parameters only, anything else is a
    ValueError before a device is touched).  The parameters are the only copy of the weights, and under round to nearest a
    bfloat16 weight ignores every update below half its spacing (2^-9 for a weight near 1): late in training most updates are
    lost without a sign of it.  With "stochastic" step 7 forms the update once in float32 and narrows it once with the stochastic
    rounding of the bf16-stored UVd / sparse-LU states: w = float(p), d = fl32(lr_eff * float(pg)), after step 3 d = fl32(d +
    float(v)), with weight decay d = fl32(d + fl32(c * w)), p <- SR(fl32(w - d)) (psgd_multi_param_update_sr / _mixed_sr on the
    fused tail, param_update_stochastic_ on the torch tail: the same bits).  SR is unbiased, so small updates accumulate in
    expectation.  The stream of step k is keyed by uvd_step_rounding_seed(seed0, k) and the element's index in the flat
    parameter order; seed0 = param_rounding_seed, or a draw from the generator behind the coin; k counts the steps that wrote the
    parameters (a skipped step does not advance it).  The perturbation of step 3 and its undo on a skipped step stay
    round-to-nearest.  state_dict() carries param_round_seed0 / param_round_step; param_rounding itself is a constructor choice.

    preconditioner_fit="whitening" (keyword-only, "hessian" by default: nothing changes, no new entry point is called; any other
    value is a ValueError before a device is touched) fits the factors to the GRADIENTS instead of to Hessian-vector products:
    the update rule of step 4 is fed the pair (dX, dG) = (v, g), v ~ N(0, I) drawn fresh on every updating step and g the raw
    float32 gradient of this step (unscaled, widened; never the momentum buffer).  The criterion E[dG' P dG + dX' P^-1 dX] is then
    minimised by P = Q'Q = (E[g g'])^(-1/2): the preconditioner whitens the gradient (the gradient-whitening fit of the PSGD
    papers).  A step needs ONE ordinary backward pass: no create_graph, no second closure call, no perturbation of the
    parameters -- so closures whose backward cannot be differentiated again (fused attention kernels, custom Functions marked
    once_differentiable) train, at about half the autograd cost.  exact_hessian_vector_product is ignored on this route (nothing
    is rejected).  The probe vectors are float32 tensors in the parameters' shapes, made once, and filled by ONE multi_randn
    launch per updating step on BOTH step tails (there is no torch.randn on this route): the stream of updating step k is keyed
    by uvd_step_rounding_seed(probe_seed0, k) and the element's index in the flat parameter order, whatever `generator` is;
    probe_seed0 = probe_seed, or a draw from the generator behind the coin (after the draw of param_rounding_seed where that
    happens); k = probe_step counts the steps that drew a probe.  The probe is finite by construction and is not judged by the
    guard; a skipped step returns before it is drawn and leaves probe_step alone.  state_dict() carries probe_seed0 / probe_step;
    preconditioner_fit itself is a constructor choice like step_tail.  The whitened gradient has roughly unit scale per element,
    as Adam's update has: lr_params and grad_clip_max_norm tuned for the Hessian fit do NOT carry over.

    mixed_dtypes=True (keyword-only; False by default: nothing changes, a second dtype is the TypeError it was; anything but a
    bool is a ValueError before a device is touched): every parameter is float32, bfloat16 or float16 on its own, on both tails;
    a list of one dtype behaves bit for bit as with False.  The switch of class UVd: each tensor is
    updated as in a one-dtype optimizer of its own dtype given the same float32 preconditioned gradient; delta and tiny are the
    largest over the dtypes present; param_rounding="stochastic" rounds the bfloat16 tensors and leaves the float32 ones to
    "nearest" (a float16 tensor, or no bfloat16 one, is a ValueError).  The widening pass widens the bfloat16 and the float16
    tensors (multi_widen_check once per such dtype over its sub-plan); the float32 tensors SKIP it and are their own wide copies,
    scaled and judged in place by one multi_scale_check launch over the float32 sub-plan on a guarded step, under the same stamp
    and flag word: still one host read.  The perturbation and the update run once per dtype present, crossed with param_groups
    once per (group, dtype) pair that has tensors; sums of squares, blend, randn, diff-scale and the narrowing of operands stay
    single.  Operand layers are chosen by shape and format as always.  Not in state_dict(), which carries no dtype.

    Out of scope: mixed dtypes with the switch off, a narrow (bfloat16) factor state, a format for vectors other than the reference's (dense, scale),
    float16 stochastic rounding."""

    def __init__(self, params_with_grad, preconditioner_formats="dense", preconditioner_init_scale=1.0, lr_params=0.01,
                 lr_preconditioner=0.01, grad_clip_max_norm=None, preconditioner_update_probability=1.0,
                 exact_hessian_vector_product=True, *, layer_batch=True, step_tail="torch", generator=None,
                 momentum=0.0, weight_decay=0.0, nonfinite="propagate", loss_scale=None, loss_scale_growth_interval=2000,
                 any_rank=False, vector_route="list", operands=None, operand_min_dim=OPERAND_MIN_DIM,
                 param_rounding="nearest", param_rounding_seed=None, preconditioner_fit="hessian", probe_seed=None,
                 param_groups=None, mixed_dtypes=False):
        _psgd._mixed_dtypes_switch("Kron", mixed_dtypes)
        if step_tail not in ("torch", "fused"):
            raise ValueError("Kron: step_tail must be 'torch' or 'fused', got %r" % (step_tail,))
        self._init_fit(preconditioner_fit)
        self._probe, self._probe_plan = None, None
        self._operands, self._operand_min_dim = _operands_dtype(operands), _operand_min_dim(operand_min_dim)
        if vector_route not in ("list", "layer"):
            raise ValueError("Kron: vector_route must be 'list' or 'layer', got %r" % (vector_route,))
        any_rank = bool(any_rank)
        # momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval: the switches of class UVd with their meaning
        # there (see step()); all off by default, and checked before anything touches a device
        self._init_features(momentum, weight_decay, nonfinite, loss_scale, loss_scale_growth_interval)
        params = _flatten(params_with_grad)
        if not params:
            raise ValueError("Kron: no parameters")
        for i, p in enumerate(params):
            if not isinstance(p, torch.Tensor):
                raise TypeError("Kron: parameter %d is not a torch tensor (%r)" % (i, type(p)))
            tag = "parameter %d (shape %s, %s)" % (i, tuple(p.shape), p.dtype)
            if p.dtype not in _DTYPE_NAMES:
                raise TypeError("Kron: %s must be float32, bfloat16 or float16" % tag)
            if p.dtype != params[0].dtype and not mixed_dtypes:
                raise TypeError("Kron: %s must be %s like parameter 0" % (tag, params[0].dtype))     # one dtype per optimizer
            if p.dim() != 2 and not any_rank:
                raise ValueError("Kron: %s must have rank 2; reshape it (the reference's demos fold a bias into its matrix)" % tag)
            if not p.requires_grad:
                raise ValueError("Kron: %s does not require grad" % tag)
            if not p.is_contiguous():
                raise ValueError("Kron: %s is not contiguous" % tag)
        # param_rounding (see the class docstring): judged before the parameters' device is looked at
        # mixed_dtypes (see the class docstring): _dtypes holds every tensor's own, _mixed says that more than one is present
        self._dtypes = [p.dtype for p in params]
        self._mixed = len(set(self._dtypes)) > 1
        self._param_sr = _psgd._param_rounding("Kron", param_rounding, set(self._dtypes) if self._mixed else params[0].dtype)
        self._param_round_seed0, self._param_round_step = None, 0
        # param_groups (None by default: nothing changes): a learning-rate scale and a weight decay per group of parameter tensors,
        # the switch of class UVd (_StepFeatures._init_groups); judged here, before the parameters' device is looked at
        self._params = params
        self._init_groups(param_groups)
        self._shapes = [tuple(int(s) for s in p.shape) for p in params]
        layers = kron_layers(self._shapes, preconditioner_formats, any_rank)
        self._formats = [f for _, _, f in layers]
        # the (M, N) of every layer; _reshape: some parameter is not its own layer (any_rank), so what the preconditioner calls take
        # and return is brought to the layers' shapes and back
        self._layer_shapes = [s for _, s, _ in layers]
        self._reshape = self._layer_shapes != self._shapes
        dev = params[0].device
        for i, p in enumerate(params):
            if not p.is_cuda or p.device != dev:
                raise ValueError("Kron: parameter %d (shape %s) is on %s; all parameters must be on one HIP device (parameter 0 is on %s)"
                                 % (i, tuple(p.shape), p.device, dev))
        self._device = dev
        # T = the parameters' dtype.  Half precision: factors, momentum buffers and everything the preconditioner reads stay fp32;
        # delta, s and tiny follow T as in class UVd (psgd.py:682-683)
        self._dtype = params[0].dtype
        self._half = self._dtype != _f32 or self._mixed
        self._delta, self._fd_inv, self._tiny = _dtype_constants(self._dtype)
        if self._mixed:           # one perturbation scale and one floor for all tensors: the largest over the dtypes present
            self._tiny, self._delta = _psgd.mixed_dtype_constants(self._dtypes)
            self._fd_inv = float(np.float32(1.0) / np.float32(self._delta))
        self._Qs = [kron_initial_factors(s, f, preconditioner_init_scale, dev, "parameter %d" % i)
                    for i, (s, f) in enumerate(zip(self._layer_shapes, self._formats))]
        # the vector layers of the list route (none with any_rank off or vector_route="layer") and all other layers; the applies of
        # the vectors write into buffers made once: the pointers of their table never move
        self._vec = [i for i, (kind, _, _) in enumerate(layers) if kind == "vector" and vector_route == "list"]
        self._mat = sorted(set(range(len(params))) - set(self._vec))
        # the operand layers (none with operands=None): (dense, dense) matrix layers, never one of self._vec; self._f32: the layers
        # of self._mat that keep the fp32 calls
        self._ops = kron_operand_layers(self._layer_shapes, self._formats, self._operands, self._operand_min_dim)
        self._f32 = [i for i in self._mat if i not in set(self._ops)]
        self._op_plan, self._op_bufs = None, None
        self._vec_plan, self._vec_out = None, None
        if self._vec:
            self._vec_plan = MultiTailPlan([self._layer_shapes[i][1] for i in self._vec], dev)
            self._vec_out = [torch.empty(self._layer_shapes[i], dtype=_f32, device=dev) for i in self._vec]
        self._init_step_hypers(lr_params, lr_preconditioner, grad_clip_max_norm, preconditioner_update_probability,
                               exact_hessian_vector_product)
        self._layer_batch = bool(layer_batch)
        self._generator = generator
        # the construction seeds, from the generator behind the coin: the parameters' first, then the probe's
        self._param_starts = None
        if self._param_sr:
            self._param_round_seed0 = self._draw_seed(param_rounding_seed)
            self._param_starts = [0]
            for p in params[:-1]:
                self._param_starts.append(self._param_starts[-1] + int(p.numel()))
        if self._whiten:
            self._probe_seed0 = self._draw_seed(probe_seed)
        self._tail = None
        if step_tail == "fused":
            self._tail = MultiTailPlan([int(p.numel()) for p in params], dev, self._dtypes if self._mixed else None)
            for g in self.param_groups or ():                   # the groups' chunk tables: made here, once
                self._tail.group_chunks(g.indices)
                if self._mixed:                                 # ... and those of the (group, dtype) pairs
                    self._tail.dtype_chunks(g.indices)
            # dG and dX of the finite-difference route: written whole by multi_diff_scale before anything reads them
            self._fd_h = [torch.empty_like(p, dtype=_f32, requires_grad=False) for p in params]
            self._fd_x = [torch.empty_like(p, dtype=_f32, requires_grad=False) for p in params]
            if self._half:
                # the fp32 copies of the gradients, the second list and the probe vectors: written whole by the one
                # multi_widen_check launch of a step before anything reads them
                # (mixed: a float32 tensor skips the widening pass and has no copy)
                self._wide = [[None if p.dtype == _f32 else torch.empty_like(p, dtype=_f32, requires_grad=False) for p in params]
                              for _ in range(3)]
            if self._ops:
                # the bf16 copies of the gradient, dX and dG of every operand layer, in the layer's shape (6 bytes per element of
                # these layers): each is written whole by a multi_narrow launch before the preconditioner call that reads it
                self._op_plan = MultiTailPlan([int(params[i].numel()) for i in self._ops], dev)
                self._op_bufs = [[torch.empty(self._layer_shapes[i], dtype=torch.bfloat16, device=dev) for i in self._ops]
                                 for _ in range(3)]
        if self._whiten:
            # the probe vectors of the whitening fit, fp32 whatever the parameters' dtype: written whole by the one multi_randn
            # launch of an updating step before anything reads them; the torch tail has no list plan of its own, so it gets one
            self._probe = [torch.empty_like(p, dtype=_f32, requires_grad=False) for p in params]
            self._probe_plan = self._tail if self._tail is not None else MultiTailPlan([int(p.numel()) for p in params], dev)

    # ------------------------------------------------------------------------------------------------- state
    @property
    def factors(self):
        """[[Ql, Qr], ...] in parameter order: the tensors the last update returned (never copies)"""
        return self._Qs

    @property
    def operand_layers(self):
        """the indices (parameter order) of the layers that run on the bf16-operand kernels: kron_operand_layers of this optimizer"""
        return list(self._ops)

    def state_dict(self):
        """Everything a bit-faithful resume needs except the parameters (the caller's): the factors (CPU clones), the formats and
        parameter shapes, the five hyper-parameters, and get_state() of the generator behind the coin and the perturbations
        (generator=None: of the module's branch generator; the global device generator that then draws the perturbations is the
        caller's, as in class UVd).  'hyper' also holds momentum and weight_decay; with momentum > 0 the dict gains
        momentum_buffers (CPU clones) and momentum_step, with nonfinite="skip" it gains nonfinite, skipped_steps, loss_scale (the
        current one; None without loss scaling) and loss_scale_good_steps, with param_rounding="stochastic" param_round_seed0 and
        param_round_step (param_rounding itself is a constructor choice and is not saved), with preconditioner_fit="whitening"
        probe_seed0 and probe_step (preconditioner_fit itself is a constructor choice too).  The 'rng' entry keeps its meaning on
        every route: the coin comes from that generator; the probe of the whitening fit does not."""
        sd = _encode_state(self._Qs, self._formats, self._shapes, {k: getattr(self, k) for k in _HYPER_KEYS},
                           self._coin_generator().get_state())
        mom = float(self.momentum)
        sd = _encode_features(sd, mom, float(self.weight_decay), self._momentum_buffers() if mom > 0.0 else None, self._m_step,
                              self._guard, self.skipped_steps, self.loss_scale.value, self._good_steps)
        sd = _psgd._param_rounding_encode(sd, self._param_sr, self._param_round_seed0, self._param_round_step)
        return self._groups_encode(_probe_encode(sd, self._whiten, self._probe_seed0, self._probe_step))

    def load_state_dict(self, sd):
        """Restore what state_dict() saved.  The factors become NEW device tensors (as after an update), the hyper-parameters are
        assigned, the generator gets the saved state.  Formats and parameter shapes must be this optimizer's.
        momentum and weight_decay are assigned when 'hyper' has them (a dict from before them leaves this object's values); the
        momentum buffers and their step counter are restored, and a dict without them zeroes the buffers of a momentum optimizer
        and restarts its warm-up.  A guarded optimizer restores skipped_steps, loss_scale_good_steps and, when both sides scale
        the loss, loss_scale where the dict has them and starts them fresh where it has not; an unguarded one ignores them.
        param_rounding="stochastic": param_round_seed0 / param_round_step are restored where the dict has them; a dict without them
        leaves this object's seed and sets the counter to 0; a nearest optimizer ignores them.
        preconditioner_fit="whitening": probe_seed0 / probe_step likewise -- restored where the dict has them, this object's seed
        and a counter of 0 where it has not (a dict of a hessian-fit optimizer); a hessian-fit optimizer ignores them."""
        factors, hyper, rng = _decode_state(sd, self._formats, self._shapes, self._layer_shapes)
        bufs, m_step = _decode_features(sd, self._shapes)
        sr_state = _psgd._param_rounding_decode("Kron.load_state_dict", sd, self._param_sr, self._param_round_seed0)
        probe_state = _probe_decode(sd, self._whiten, self._probe_seed0, "Kron.load_state_dict")
        group_values = self._groups_judge(sd, "Kron.load_state_dict")
        try:
            self._coin_generator().set_state(rng)
        except (RuntimeError, TypeError) as e:
            raise ValueError("Kron.load_state_dict: 'rng' does not fit this optimizer's generator: %s" % e)
        for k in _HYPER_KEYS:
            getattr(self, k).assign(hyper[k])
        for k in ("momentum", "weight_decay"):
            if k in hyper:
                getattr(self, k).assign(hyper[k])
        self._Qs = [[q.to(self._device, copy=True) for q in pair] for pair in factors]
        self._m_step = m_step
        self._param_round_seed0, self._param_round_step = sr_state
        self._probe_seed0, self._probe_step = probe_state
        self._groups_commit(group_values)
        with torch.no_grad():
            if bufs is not None:
                for m, b in zip(self._momentum_buffers(), bufs):
                    m.copy_(b)
            elif float(self.momentum) > 0.0:             # no buffer saved: a momentum optimizer starts its warm-up again
                for m in self._momentum_buffers():
                    m.zero_()
        self._guard_decode(sd)

    # ------------------------------------------------------------------------------------------------- momentum, guard
    def _momentum_buffers(self):
        """one zero-initialised fp32 buffer per parameter, created on first use"""
        if self._m is None:
            self._m = [torch.zeros_like(p, dtype=_f32, requires_grad=False) for p in self._params]
        return self._m

    @staticmethod
    def _owned(tensors):
        """detached contiguous tensors, no two of them the same memory (autograd may hand one tensor to two parameters): safe to
        scale in place"""
        out, seen = [], set()
        for t in tensors:
            t = t.detach().contiguous()
            if t.data_ptr() in seen and t.numel():
                t = t.clone()
            seen.add(t.data_ptr())
            out.append(t)
        return out

    def _judge(self, grads, second, vs, inv):
        """The guard and the loss scale of one step, BEFORE anything else reads its inputs: the gradients and the second list (Hvs on
        the exact route, the perturbed gradients on the finite-difference one; None on a step that leaves the factors alone) are
        multiplied by inv = 1 / loss_scale (nothing when inv == 1), and they and the probe vectors vs (never scaled) are judged.
        Returns (grads, second, bad).  Guarded fused tail: ONE multi_scale_check launch and ONE 4-byte host read; guarded torch
        tail: per-tensor `* inv` and torch.isfinite(...).all(), one host read of one bool.  Unguarded (inv == 1): nothing runs."""
        if not self._guard:
            return grads, second, False
        if self._tail is not None:
            grads = self._owned(grads)
            lists, scales = [grads], [inv]
            if second is not None:
                second = self._owned(second)
                lists += [second, [v.contiguous() for v in vs]]
                scales += [inv, 1.0]
            plan = self._tail
            stamp = plan.next_stamp()
            multi_scale_check(lists, scales, flag=plan.flag, stamp=stamp, plan=plan)
            return grads, second, int(plan.flag.item()) == stamp                            # the host read of a guarded step
        if inv != 1.0:
            grads = [g * inv for g in grads]
            second = None if second is None else [h * inv for h in second]
        ok = None
        for x in list(grads) + list(second or ()) + list(vs or ()):
            f = torch.isfinite(x).all()
            ok = f if ok is None else ok & f
        return grads, second, not bool(ok.item())                                           # ... and of the torch tail

    def _widen(self, grads, second, vs, inv):
        """The widening pass of a step on bfloat16 / float16 parameters, BEFORE anything else reads its inputs: the gradients and
        the second list become float32(float(x) * inv), the probe vectors float(v); the guard, where on, judges exactly the values
        written (a finite input that overflows under inv counts, and so does an fp16 +-Inf).  second and vs are None on a step
        that leaves the factors alone.  Returns (grads, second, vs, bad), fp32 lists.  Fused tail: ONE multi_widen_check launch
        into the preallocated lists, guarded or not, and ONE 4-byte host read when guarded; torch tail: per-tensor expressions and,
        when guarded, torch.isfinite(...).all() with one host read of one bool."""
        if self._tail is not None:
            srcs, scales = [[g.contiguous() for g in grads]], [inv]
            if second is not None:
                srcs += [[h.contiguous() for h in second], [v.contiguous() for v in vs]]
                scales += [inv, 1.0]
            dsts = self._wide[:len(srcs)]
            plan, bad = self._tail, False
            scale_f32 = self._mixed and (self._guard or inv != 1.0)
            if self._mixed:
                # the float32 tensors skip the widening pass: they are their own wide copies, scaled in place and judged by a
                # multi_scale_check launch over the float32 sub-plan where there is a scale or a guard, else not touched at all
                if scale_f32 and inv != 1.0:
                    srcs = [self._owned(ts) for ts in srcs]
                dsts = [[x if w is None else w for x, w in zip(ts, ws)] for ts, ws in zip(srcs, dsts)]
            if self._guard:
                stamp = plan.next_stamp()                       # one stamp, one flag word for all launches of this pass
                multi_widen_check(srcs, dsts, scales, flag=plan.flag, stamp=stamp, plan=plan)
                if scale_f32:
                    multi_scale_check(srcs, scales, flag=plan.flag, stamp=stamp, plan=plan)
                bad = int(plan.flag.item()) == stamp                                            # the host read of a guarded step
            else:
                multi_widen_check(srcs, dsts, scales, plan=plan)
                if scale_f32:
                    multi_scale_check(srcs, scales, plan=plan)
            wide = dsts + [None] * (3 - len(dsts))
            return wide[0], wide[1], wide[2], bad
        grads = [g.float() * inv for g in grads]
        if second is not None:
            second, vs = [h.float() * inv for h in second], [v.float() for v in vs]
        bad = False
        if self._guard:
            ok = None
            for x in list(grads) + list(second or ()) + list(vs or ()):
                f = torch.isfinite(x).all()
                ok = f if ok is None else ok & f
            bad = not bool(ok.item())                                                           # ... and of the torch tail
        return grads, second, vs, bad

    def _screen(self, grads, second, vs, inv, undo=None):
        """The one pass of a step over its inputs, BEFORE anything else reads them: _widen for bfloat16 / float16 parameters, else
        _judge for a guarded step, then the guard's book-keeping (a skipped finite-difference step takes the perturbation `undo`
        back).  Returns (grads, second, vs, bad); bad: the caller returns at once.  Neither half nor guarded: the inputs come
        back untouched -- nothing runs, no host read."""
        if not (self._half or self._guard):
            return grads, second, vs, False
        with torch.no_grad():
            if self._half:
                grads, second, vs, bad = self._widen(grads, second, vs, inv)
            else:
                grads, second, bad = self._judge(grads, second, vs, inv)
        if self._guard:
            self._guard_outcome(bad, undo if bad else None)
        return grads, second, vs, bad

    def _blend(self, grads, mom):
        """the gradients that precond_grad_kron takes: with momentum the buffers after m <- fl32(fl32(beta_k m) + fl32((1 - beta_k) g))
        (fused tail: one multi_blend launch; torch tail: the same three roundings per tensor; beta_k == 0 does not read m).  A
        step with momentum == 0 sets the warm-up counter back."""
        if mom == 0.0:
            self._m_step = 0
            return grads
        beta, omb = _psgd.uvd_momentum_coefficients(self._m_step, mom)
        self._m_step += 1
        ms = self._momentum_buffers()
        if self._tail is not None:
            multi_blend(ms, [g.contiguous() for g in grads], beta, omb, plan=self._tail)
            return ms
        for m, g in zip(ms, grads):
            if beta == 0.0:
                m.copy_(g * omb)
            else:
                m.mul_(beta)
                m.add_(g * omb)
        return ms

    # ------------------------------------------------------------------------------------------------- step
    def _randn(self, p):
        gen = self._generator
        if gen is None:
            return torch.randn_like(p, requires_grad=False)
        v = torch.randn(p.shape, dtype=p.dtype, device=gen.device, generator=gen)
        return v if v.device == p.device else v.to(p.device)

    def _coin(self):
        """psgd.py:703, drawn as class UVd draws it (always, whatever the probability); a device generator gives a device draw"""
        gen = self._generator
        if gen is None or gen.device.type == "cpu":
            return _psgd._draw_branch(float(self.preconditioner_update_probability), gen)
        return bool(torch.rand((), generator=gen, device=gen.device).item() < float(self.preconditioner_update_probability))

    def _block(self):
        return _kron.layer_batch() if self._layer_batch else contextlib.nullcontext()

    def _as_layers(self, tensors):
        """parameter-shaped tensors in the (M, N) of their layers (views where the memory allows); nothing without any_rank"""
        if not self._reshape:
            return tensors
        return [t.reshape(s) for t, s in zip(tensors, self._layer_shapes)]

    def _update_factors(self, dXs, dGs, lr_q):
        """step 4: one update_precond_kron per layer inside one block, the factor references rebound to the returned tensors; the
        vector layers of the list route in ONE multi_vec_precond_update launch, in place"""
        dXs, dGs = self._as_layers(dXs), self._as_layers(dGs)
        Qs = self._Qs
        if not self._vec and not self._ops:
            with self._block():
                new = [_psgd.update_precond_kron(q[0], q[1], dX, dG, lr_q) for q, dX, dG in zip(Qs, dXs, dGs)]
            self._Qs = [[a, b] for a, b in new]
            return
        Qs = list(Qs)
        if self._ops:
            # the operand layers: bf16(dX), bf16(dG) -- ONE multi_narrow launch for all of them (torch tail: .to(bfloat16) per
            # tensor) -- into update_precond_kron, which runs them at once on the bf16-operand kernel: outside the block, so that
            # the queue of the small fp32 layers stays whole
            ops = self._ops
            bX, bG = self._narrow([[dXs[i] for i in ops], [dGs[i] for i in ops]], self._op_bufs and self._op_bufs[1:])
            for i, x, g in zip(ops, bX, bG):
                Qs[i] = list(_psgd.update_precond_kron(Qs[i][0], Qs[i][1], x, g, lr_q))
        if self._f32:
            with self._block():
                new = [_psgd.update_precond_kron(Qs[i][0], Qs[i][1], dXs[i], dGs[i], lr_q) for i in self._f32]
            for i, (a, b) in zip(self._f32, new):
                Qs[i] = [a, b]
        vec = self._vec
        if vec:
            multi_vec_precond_update([Qs[i][0] for i in vec], [Qs[i][1] for i in vec], [dXs[i].contiguous() for i in vec],
                                     [dGs[i].contiguous() for i in vec], lr_q, plan=self._vec_plan)
        self._Qs = Qs

    def _narrow(self, lists, bufs):
        """bf16(x) of the fp32 tensors of one to three lists, one list per role of the operand layers: round to nearest even of the
        values the step already has; nothing is judged again (the guard has seen the fp32 values).  Fused tail: ONE multi_narrow
        launch into the preallocated buffers; torch tail: x.to(torch.bfloat16) per tensor."""
        if self._tail is not None:
            return multi_narrow([[x.contiguous() for x in xs] for xs in lists], bufs, plan=self._op_plan)
        return [[x.to(torch.bfloat16) for x in xs] for xs in lists]

    def _precondition(self, grads):
        """step 5: one precond_grad_kron per layer inside a second block; the vector layers of the list route in ONE
        multi_vec_precond_grad launch.  Returns the preconditioned gradients in the layers' shapes."""
        grads = self._as_layers(grads)
        Qs = self._Qs
        if not self._vec and not self._ops:
            with self._block():
                return [_psgd.precond_grad_kron(q[0], q[1], g) for q, g in zip(Qs, grads)]
        pre = [None] * len(grads)
        if self._ops:
            # the operand layers: bf16(g) (one multi_narrow launch) into precond_grad_kron; their preconditioned gradient is bf16
            ops = self._ops
            (bg,) = self._narrow([[grads[i] for i in ops]], self._op_bufs and self._op_bufs[:1])
            for i, g in zip(ops, bg):
                pre[i] = _psgd.precond_grad_kron(Qs[i][0], Qs[i][1], g)
        if self._f32:
            with self._block():
                out = [_psgd.precond_grad_kron(Qs[i][0], Qs[i][1], grads[i]) for i in self._f32]
            for i, g in zip(self._f32, out):
                pre[i] = g
        vec = self._vec
        if vec:
            multi_vec_precond_grad([Qs[i][0] for i in vec], [Qs[i][1] for i in vec], [grads[i].contiguous() for i in vec],
                                   self._vec_out, plan=self._vec_plan)
            for i, g in zip(vec, self._vec_out):
                pre[i] = g
        return pre

    def step(self, closure):
        """One step; returns what closure() returns (the loss is its first element when it is an iterable).

        1. the coin of psgd.py:703: update the factors this step?  (_step_route names what follows; the closure calls, the
           backward passes and the draws of steps 2 and 3 are _StepFeatures._closure_gradients's, whose docstring fixes their order.)
        2. exact product: dX = v, dG = Hv, the probe vectors drawn from `generator` (_randn).
        3. finite differences (psgd.py:716-727, :734-736): delta = sqrt(eps_fp32); dG = (g' - g) * s, dX = v * s with
           s = float32(1) / float32(delta); the perturbation p += v is undone in step 7.
        4. one update_precond_kron per layer (inside one kron.layer_batch() block); the factor references are rebound to the returned
           tensors, nothing is copied.
        5. one precond_grad_kron per layer (a second block).  any_rank: dX, dG and the gradients are taken in the shapes of the
           layers (views), and with vector_route="list" the vector layers leave steps 4 and 5 for one multi_vec_precond_update launch
           (in place: these factor tensors are not rebound) and one multi_vec_precond_grad launch.
        6. lr_eff and the decay coefficient c per tensor: the rule of _StepFeatures._tail_coefficients, S = the fp64 sum of the
           float32 squares of all preconditioned gradients.  tiny = finfo(float32).tiny follows psgd.py:753 (class UVd), not
           mnist_with_lenet5.py:54-55, which divides by the bare norm: a zero gradient gives a zero step, not NaN.
        7. p <- p - float32(lr_eff * pg); after step 3, p <- p - float32(float32(lr_eff * pg) + v) (psgd.py:761).

        The switches of class UVd, with their meaning there; both tails round alike, and with all of them at their defaults none of
        this runs (the same launches, the same bits, no host read):
        loss_scale=S: every gradient the step takes is that of loss * S (the closure is unchanged and returns the unscaled loss);
        inv = 1 / S, exact because S is a power of two, is applied once to the gradients and to the second list (Hvs in step 2, the
        perturbed gradients in step 3) before anything else reads them; the probe vectors are never scaled.
        nonfinite="skip": in that same pass the gradients, the second list and the probe vectors are judged, and a step with a
        +-Inf or NaN among them is SKIPPED before the first update_precond_kron: factors, parameters, momentum buffers and the
        warm-up counter keep their bits; after step 3 the perturbation is taken back by p <- float32(p - v), within one rounding of
        the old parameters.  A skipped step has consumed the coin and the probe vectors and nothing else.  Fused tail: one
        multi_scale_check launch and one 4-byte host read per guarded step; torch tail: per-tensor `* inv` and
        torch.isfinite(...).all(), one host read of one bool.  "dynamic" halves S on a skip and doubles it after
        loss_scale_growth_interval good steps in a row (uvd_loss_scale_next).
        momentum: m <- float32(float32(beta_k m) + float32((1 - beta_k) g)) on the unscaled gradient, beta_k of
        uvd_momentum_coefficients (k counts the steps blended so far; a step taken with momentum == 0 sets it back to 0), and step 5
        is applied to m (fused tail: one multi_blend launch).  weight_decay: step 7 subtracts float32(delta + float32(c p)) with
        c = float32(lr_eff weight_decay).  With everything on the fused tail issues at most seven launches besides the
        preconditioner calls: perturbation, scale-check, difference, blend, two for the sum of squares, update.

        Parameters of dtype T = bfloat16 / float16 (nothing of this runs for float32).  The probe vectors are drawn in T (step 3:
        T(randn_T * delta), delta = finfo(T).eps ** 0.5; the perturbation is p <- T(p + v)).  A WIDENING PASS comes first, once per
        step and before anything else reads its inputs: gradients and second list -> float32(float(x) * inv), probe vectors ->
        float(v); the guard, where on, judges exactly these written values, so an fp16 gradient that is already +-Inf skips the
        step.  Fused tail: one multi_widen_check launch into preallocated float32 lists (in the place of the scale-check; one
        4-byte host read when guarded); torch tail: `g.float() * inv` per tensor.  Steps 3-6 then run on float32 lists as above,
        with s = float32(1) / float32(delta): dG = fl32(fl32(g'_wide - g_wide) * s) subtracts in float32, where the reference and
        class UVd subtract in T.  Step 7 rounds as psgd_uvd_param_update_multi_wd does, every operation to nearest even on its own:
        delta = T(fl32(lr_eff * pg)); after step 3, delta = T(delta + v); with weight decay, delta = T(delta + T(fl32(c *
        float(p)))), c = fl32(lr_eff * wd); p <- T(p - delta); tiny = finfo(T).tiny in step 6.  The torch tail is the same chain,
        one torch op per rounding.  With everything on the fused tail still issues seven launches: perturbation, widen-check,
        difference, blend, two for the sum of squares, update.

        operands="bfloat16" (nothing of this runs without operand layers).  bf16(x) is round-to-nearest-even of the float32 value
        the step already has -- after the widening / scale / guard pass and, for the gradient, after the blend: NaN stays NaN, a
        finite value beyond the bfloat16 range becomes +-Inf, exactly as tensor.to(torch.bfloat16) does.  The guard has judged the
        float32 values: the narrowing is not judged again and there is no second host read, so a finite float32 value beyond
        3.39e38 that overflows HERE propagates into the factors or the parameters, under the "propagate silently" contract of an
        unguarded step.  Fused tail: at most two multi_narrow launches per step whatever the number of layers -- one before the
        updates (dX and dG, on steps that update the factors), one before the applies (gradients or momentum buffers) -- so at
        most nine launches with everything on; the sum of squares and the update then go through psgd_multi_sumsq_mixed and
        psgd_multi_param_update_mixed, which read a bf16 preconditioned gradient as float(pg): S adds fl32(float(pg) float(pg)) in
        fp64 and delta = T(fl32(lr_eff float(pg))), everything after that unchanged.  Torch tail: x.to(torch.bfloat16) and
        pg.float() per tensor, the definition the kernels match.  Inside layer_batch blocks the operand layers run at once, as
        outside a block; the class issues them before the block so that the queue of the small layers stays whole.

        preconditioner_fit="whitening" (nothing of this runs with "hessian").  Steps 2 and 3 give way to the "whitening" route: ONE
        closure call, ONE ordinary backward, no perturbation (nothing to undo in step 7).  The widening / scale / guard pass is that of a step that leaves the
        factors alone: it sees the gradients only (inv is applied once), the probe is not judged because it is finite by
        construction, and a skipped step returns before the probe is drawn: probe_step, factors, parameters, momentum buffers
        and the warm-up counter keep their bits, and the next step draws the stream the skipped one would have drawn.  When the
        coin says update: ONE multi_randn launch (seed uvd_step_rounding_seed(probe_seed0, probe_step), index0 = 0, scale = 1)
        fills the float32 probe buffers on either tail, probe_step advances, and step 4 runs with dX = the probe, dG = the float32
        gradients of this step -- raw, unscaled, widened; not the momentum buffer.  From step 4 on nothing differs: operand
        layers narrow dX / dG by multi_narrow, vector layers of the list route go to multi_vec_precond_update, then the blend,
        step 5, the clip, weight decay and param_rounding.  Nothing on this route differs between the tails before step 6."""
        params = self._params
        update_Q = self._coin()
        fused = self._tail is not None
        mom, wd, S, inv, scaled = self._step_scales()
        groups = self._step_groups(wd)                          # None without param_groups: nothing below changes
        # the routes differ in what they hand to _screen and in what becomes (dX, dG) after it.  vs of "fd", T(randn_T * delta),
        # stays the perturbation to undo after a half-precision widening, whose fp32 copy feeds dX
        route = self._step_route(update_Q)
        closure_returns, grads, second, vs = self._closure_gradients(
            closure, route, scaled, self._randn, self._delta,
            (lambda vs: multi_param_update(params, None, vs, plan=self._tail)) if fused else None)
        undo = vs if route == "fd" else None
        grads, second, vs, bad = self._screen(grads, second, vs, inv, undo)
        if bad:                                                 # before a probe is drawn: probe_step does not move
            return closure_returns
        if route == "whitening":
            with torch.no_grad():
                multi_randn(self._probe, self._next_probe_seed(), plan=self._probe_plan)
            dXs, dGs = self._probe, list(grads)
        elif route == "exact":
            dXs, dGs = vs, second
        elif route == "fd":
            with torch.no_grad():
                if fused:
                    dXs, dGs = self._fd_x, self._fd_h
                    multi_diff_scale([g.contiguous() for g in second], [g.contiguous() for g in grads], dGs, vs, dXs,
                                     self._fd_inv, plan=self._tail)
                else:
                    dGs = [(pg - g) * self._fd_inv for pg, g in zip(second, grads)]
                    dXs = [v * self._fd_inv for v in vs]
        with torch.no_grad():
            if update_Q:
                self._update_factors(dXs, dGs, float(self.lr_preconditioner))
            if mom != 0.0 or self._m_step:
                grads = self._blend(grads, mom)
            pre_grads = self._precondition(grads)
            lr, max_norm = float(self.lr_params), float(self.grad_clip_max_norm)
            clip = not math.isinf(max_norm)
            sr = self._param_sr                             # this step writes the parameters: the seed of its rounding stream
            sr_seed = self._next_param_round_seed() if sr else None
            if fused:
                pre_grads = [g.contiguous() for g in pre_grads]          # (the mirrored formats return transposed views)
                sumsq = multi_sumsq(pre_grads, plan=self._tail) if clip else None
                multi_param_update(params, pre_grads, undo, lr, sumsq, max_norm if clip else None, self._tiny, plan=self._tail,
                                   **self._fused_tail_kwargs(groups, wd, sr, sr_seed))
                return closure_returns
            if self._ops:                                   # float(pg) of the bf16 preconditioned gradients, exact
                pre_grads = [g.float() if g.dtype != _f32 else g for g in pre_grads]
            sq = [torch.sum((g * g).double()) for g in pre_grads] if clip else None
            sumsq = sum(sq[1:], sq[0]) if clip else None    # left to right, in fp64
            coef = self._tail_coefficients(lr, wd, groups, max_norm, sumsq, self._tiny, len(params))
            for k, (p, g) in enumerate(zip(params, pre_grads)):
                if self._reshape:
                    g = g.reshape(p.shape)
                _psgd._torch_param_update_(p, g, None if undo is None else undo[k], *coef[k],
                                           sr_seed if p.dtype == torch.bfloat16 else None, self._param_starts[k] if sr else 0)
        return closure_returns
