"""A stand-in for the TensorFlow names that the reference module touches.  TEST INFRASTRUCTURE ONLY.

The reference (``preconditioned_stochastic_gradient_descent.py``, ``psgd.py`` below) is Python on TensorFlow, and
TensorFlow cannot be installed where this project is built.  Of the ~36 ``tf.*`` names the reference uses, six do the
numerical work (``matmul`` with its transpose flags, ``linalg.triangular_solve``, ``linalg.solve``, ``linalg.band_part``,
``linalg.diag_part``, ``reduce_max`` / ``reduce_sum``); the rest is plumbing.  This package implements exactly those names,
on torch CPU tensors, from TensorFlow's documented API semantics, so that the reference's own program text runs
unmodified and its outputs can be recorded as fixtures (tests/golden/make_golden_tf.py).  Nothing of the reference is
copied here, and nothing in the product package may import this.

    tf = oracle.tf_standin.make("float32" | "float64")

returns one object that plays the role of the ``tensorflow`` module.  The generator puts it into
``sys.modules["tensorflow"]`` of its own process while it loads the reference; there is no other way to reach it.

Strict by construction
  * every function has an explicit signature: an unknown keyword (``adjoint=`` where there is none, a misspelt
    ``transpose_a=``) is a TypeError, never ignored;
  * a name that is not implemented is an AttributeError, on the module object and on its tensors alike;
  * two tensors of different dtypes do not mix, as in TensorFlow; Python scalars take the dtype of the tensor they meet.

Precision switch
  The reference fixes ``dtype = tf.float32`` at import (psgd.py:20).  ``make("float64")`` maps the stand-in's
  ``tf.float32`` to 64-bit storage, so the same program text gives a result without fp32 noise.

Semantics worth naming
  * ``triangular_solve`` reads only the triangle that ``lower`` names; ``adjoint=True`` solves with the transpose of that
    triangle.  ``solve(adjoint=True)`` solves with the transpose.
  * ``band_part(x, 0, -1)`` is the upper triangle, ``(-1, 0)`` the lower one, ``(0, 0)`` the diagonal.
  * ``maximum`` / ``minimum`` propagate NaN; ``reduce_max`` of an empty tensor is -inf.
  * TensorFlow's CPU kernels flush denormal results to zero.  The reference relies on that: its halving loop for ``_tiny``
    (psgd.py:22, :682) ends at the smallest NORMAL number only then.  Floating-point results of ``* /`` are flushed the same way.
  * ``GradientTape`` records only inside its ``with`` block, may be nested (the Hessian-vector product of psgd.py:708-714)
    and, not being persistent, gives one ``gradient`` call.
  * ``function`` is a pass-through that converts its arguments to tensors and enforces the rank and dtype that each
    ``TensorSpec`` states.
"""
import operator

import numpy as np
import torch

VERSION = "tf_standin-1 (torch %s, cpu)" % torch.__version__
PRECISIONS = ("float32", "float64")


class DType:
    """A TensorFlow dtype: a name and the torch dtype that stores it under the precision chosen."""

    def __init__(self, name, storage):
        self.name, self.storage = name, storage
        self.is_floating = storage.is_floating_point

    def __repr__(self):
        return "tf." + self.name


def make(precision="float32"):
    """The object that stands for the ``tensorflow`` module, at the given precision of ``tf.float32``."""
    if precision not in PRECISIONS:
        raise ValueError("tf_standin.make: precision must be one of %r, got %r" % (PRECISIONS, precision))
    return _TF(precision)


def _index(k):
    """One component of a subscript: an int (NumPy ints included), None or a slice of such."""
    if k is None:
        return None
    if isinstance(k, slice):
        f = lambda s: None if s is None else operator.index(s)
        return slice(f(k.start), f(k.stop), f(k.step))
    if isinstance(k, Tensor):
        raise TypeError("tf_standin: a tensor as subscript is not implemented")
    return operator.index(k)


class Tensor:
    """An eager tensor: `_t` is the torch tensor, `dtype` the DType, `_tf` the module object it belongs to."""
    __slots__ = ("_t", "dtype", "_tf")
    __array_priority__ = 1000         # NumPy scalars on the left defer to the reflected operators below
    __hash__ = object.__hash__

    def __init__(self, tf, t, dtype):
        self._tf, self._t, self.dtype = tf, t, dtype

    # ----- plumbing
    @property
    def shape(self):
        return tuple(self._t.shape)

    def numpy(self):
        a = self._t.detach().numpy().copy()
        return a if a.ndim else a[()]

    def __repr__(self):
        return "<tf_standin.Tensor shape=%s dtype=%s>" % (self.shape, self.dtype.name)

    def __bool__(self):
        if self._t.numel() != 1:
            raise ValueError("the truth value of a tensor with more than one element is ambiguous")
        return bool(self._t.item())

    def __len__(self):
        if not self._t.dim():
            raise TypeError("a scalar tensor has no len()")
        return self._t.shape[0]

    def __iter__(self):
        raise TypeError("tf_standin: iterating over a tensor is not implemented")

    def __getitem__(self, key):
        key = tuple(_index(k) for k in key) if isinstance(key, tuple) else _index(key)
        return self._tf._wrap(self._t[key], self.dtype)

    # ----- arithmetic and comparison
    def _pair(self, other):
        tf = self._tf
        if isinstance(other, Tensor):
            if other.dtype is not self.dtype:
                raise TypeError("cannot mix %r and %r tensors in one op" % (self.dtype, other.dtype))
            return other._t
        return tf._convert(other, self.dtype)._t

    def _arith(self, other, fn, flush=False, swap=False):
        o = self._pair(other)
        r = fn(o, self._t) if swap else fn(self._t, o)
        if flush and self.dtype.is_floating:
            r = self._tf._flush(r)
        return self._tf._wrap(r, self.dtype)

    def _compare(self, other, fn):
        return self._tf._wrap(fn(self._t, self._pair(other)), self._tf.bool)

    def __add__(self, o): return self._arith(o, torch.add)
    def __radd__(self, o): return self._arith(o, torch.add, swap=True)
    def __sub__(self, o): return self._arith(o, torch.sub)
    def __rsub__(self, o): return self._arith(o, torch.sub, swap=True)
    def __mul__(self, o): return self._arith(o, torch.mul, flush=True)
    def __rmul__(self, o): return self._arith(o, torch.mul, flush=True, swap=True)
    def __truediv__(self, o): return self._arith(o, torch.true_divide, flush=True)
    def __rtruediv__(self, o): return self._arith(o, torch.true_divide, flush=True, swap=True)
    def __pow__(self, o): return self._arith(o, torch.pow)
    def __neg__(self): return self._tf._wrap(-self._t, self.dtype)
    def __lt__(self, o): return self._compare(o, torch.lt)
    def __le__(self, o): return self._compare(o, torch.le)
    def __gt__(self, o): return self._compare(o, torch.gt)
    def __ge__(self, o): return self._compare(o, torch.ge)
    def __eq__(self, o): return self._compare(o, torch.eq)
    def __ne__(self, o): return self._compare(o, torch.ne)


class Variable(Tensor):
    """tf.Variable: one buffer that assign / assign_add / assign_sub change in place."""
    __slots__ = ("trainable",)

    def __init__(self, tf, t, dtype, trainable):
        super().__init__(tf, t.detach().clone(), dtype)
        self.trainable = bool(trainable)
        if self.trainable and dtype.is_floating:
            self._t.requires_grad_(True)

    def _value(self, value):
        t = self._tf._convert(value, self.dtype)
        if t.dtype is not self.dtype:
            raise TypeError("cannot assign a %r value to a %r variable" % (t.dtype, self.dtype))
        if t.shape != self.shape:
            raise ValueError("cannot assign a value of shape %s to a variable of shape %s" % (t.shape, self.shape))
        return t._t.detach()

    def assign(self, value):
        new = self._value(value)
        with torch.no_grad():
            self._t.copy_(new)
        return self

    def assign_add(self, delta):
        new = self._value(delta)
        with torch.no_grad():
            self._t.add_(new)
        return self

    def assign_sub(self, delta):
        new = self._value(delta)
        with torch.no_grad():
            self._t.sub_(new)
        return self


class TensorSpec:
    def __init__(self, shape, dtype):
        self.shape, self.dtype = (None if shape is None else list(shape)), dtype


class GradientTape:
    """Records the ops of its `with` block on the trainable variables; gradient() may be called once."""

    def __init__(self, tf):
        self._tf, self._used = tf, False

    def __enter__(self):
        self._tf._tapes += 1
        return self

    def __exit__(self, *exc):
        self._tf._tapes -= 1
        return False

    def gradient(self, target, sources, output_gradients=None):
        if self._used:
            raise RuntimeError("A non-persistent GradientTape can only be used to compute one set of gradients")
        self._used = True
        tf = self._tf
        single = isinstance(sources, Tensor)
        srcs = [sources] if single else list(sources)
        tgts = [target] if isinstance(target, Tensor) else list(target)
        outs = None
        if output_gradients is not None:
            ogs = [output_gradients] if isinstance(output_gradients, Tensor) else list(output_gradients)
            if len(ogs) != len(tgts):
                raise ValueError("output_gradients must match target")
            outs = [tf._convert(g, t.dtype)._t for g, t in zip(ogs, tgts)]
        live = [(t._t, None if outs is None else outs[i]) for i, t in enumerate(tgts) if t._t.requires_grad]
        if not live:
            return None if single else [None for _ in srcs]
        grads = torch.autograd.grad([t for t, _ in live], [s._t for s in srcs],
                                    grad_outputs=None if outs is None else [g for _, g in live],
                                    create_graph=tf._tapes > 0, allow_unused=True)
        res = [None if g is None else tf._wrap(g, s.dtype) for g, s in zip(grads, srcs)]
        return res[0] if single else res


class _Namespace:
    """tf.linalg, tf.random, ...: plain attribute holders (assignable, so that a generator can substitute a draw)."""


class _TF:
    """The module object.  Everything the reference may call is a method or attribute below; anything else raises."""

    def __init__(self, precision):
        self.__name__ = "tensorflow"
        self.__version__ = VERSION
        self.precision = precision
        wide = precision == "float64"
        self.float32 = DType("float32", torch.float64 if wide else torch.float32)
        self.float64 = DType("float64", torch.float64)
        self.int32 = DType("int32", torch.int32)
        self.int64 = DType("int64", torch.int64)
        self.bool = DType("bool", torch.bool)
        self._tapes = 0
        self._rng = torch.Generator().manual_seed(0)
        self.Tensor, self.TensorSpec = Tensor, TensorSpec
        lin, rnd, nest, mth = _Namespace(), _Namespace(), _Namespace(), _Namespace()
        lin.triangular_solve, lin.solve, lin.band_part, lin.diag_part = (self._triangular_solve, self._solve, self._band_part,
                                                                         self._diag_part)
        rnd.normal, rnd.uniform, rnd.set_seed = self._normal, self._uniform, self._set_seed
        nest.flatten = self._flatten
        mth.is_inf = self._is_inf
        self.linalg, self.random, self.nest, self.math = lin, rnd, nest, mth

    # ----- conversion
    def _dtype(self, dtype):
        """A dtype argument: one of this object's DTypes, or Python's bool as TensorFlow accepts it."""
        if dtype is bool:
            return self.bool
        if isinstance(dtype, DType) and getattr(self, dtype.name, None) is dtype:
            return dtype
        raise TypeError("not a dtype of this stand-in: %r" % (dtype,))

    def _wrap(self, t, dtype):
        if self._tapes == 0 and t.requires_grad:
            t = t.detach()                       # nothing records outside a tape
        return Tensor(self, t, dtype)

    def _flush(self, t):
        tiny = torch.finfo(t.dtype).tiny
        return torch.where(t.abs() < tiny, torch.zeros((), dtype=t.dtype), t)

    def _np_dtype(self, a):
        name = {"float32": "float32", "float64": "float64", "int32": "int32", "int64": "int64", "bool": "bool"}.get(a.dtype.name)
        if name is None:
            raise TypeError("tf_standin: no dtype for NumPy's %s" % a.dtype)
        return getattr(self, name)

    def _convert(self, value, dtype=None):
        """tf.convert_to_tensor: tensors pass (their dtype must agree), Python and NumPy values take `dtype` or the default
        TensorFlow gives them (bool, int32, float32; a NumPy array its own)."""
        dtype = None if dtype is None else self._dtype(dtype)
        if isinstance(value, Tensor):
            if dtype is not None and value.dtype is not dtype:
                raise TypeError("expected a %r tensor, got %r" % (dtype, value.dtype))
            return value
        if isinstance(value, (list, tuple)) and any(isinstance(x, Tensor) for x in value):
            parts = [self._convert(x, dtype) for x in value]
            return self.stack(parts, axis=0)
        if isinstance(value, (np.ndarray, np.generic)):
            a = np.asarray(value)
            own = self._np_dtype(a)
        else:
            a = np.asarray(value)
            if a.dtype == np.bool_:
                own = self.bool
            elif a.dtype.kind in "iu":
                own = self.int32
            elif a.dtype.kind == "f":
                own = self.float32
            else:
                raise TypeError("tf_standin: cannot convert %r to a tensor" % (value,))
        dt = own if dtype is None else dtype
        if dt.is_floating is False and own.is_floating:
            raise TypeError("cannot convert a floating-point value to %r" % (dt,))
        return Tensor(self, torch.from_numpy(np.array(a, order="C")).to(dt.storage), dt)

    def _dims(self, shape):
        """A shape argument: a list / tuple of ints, or an integer tensor (tf.shape's result)."""
        if isinstance(shape, Tensor):
            if shape.dtype.is_floating:
                raise TypeError("a shape must be integer")
            return [int(x) for x in shape._t.reshape(-1).tolist()]
        return [int(x._t.item()) if isinstance(x, Tensor) else operator.index(x) for x in shape]

    # ----- creation and plumbing
    def constant(self, value, dtype=None):
        return self._convert(value, dtype)

    def Variable(self, initial_value, trainable=True, dtype=None):
        t = self._convert(initial_value, dtype)
        return Variable(self, t._t, t.dtype, trainable)

    def GradientTape(self):
        return GradientTape(self)

    def function(self, func=None, input_signature=None):
        def decorate(fn):
            if input_signature is None:
                return fn
            specs = list(input_signature)

            def checked(*args):
                if len(args) > len(specs):
                    raise TypeError("%s takes %d arguments, %d given" % (fn.__name__, len(specs), len(args)))
                conv = []
                for i, (a, s) in enumerate(zip(args, specs)):
                    t = self._convert(a, s.dtype)
                    if s.shape is not None:
                        if len(t.shape) != len(s.shape) or any(w is not None and w != h for w, h in zip(s.shape, t.shape)):
                            raise ValueError("%s: argument %d has shape %s, the signature states %s"
                                             % (fn.__name__, i, list(t.shape), s.shape))
                    conv.append(t)
                return fn(*conv)
            checked.__name__, checked.__doc__ = fn.__name__, fn.__doc__
            return checked
        return decorate if func is None else decorate(func)

    def print(self, *args):
        print(*[a.numpy() if isinstance(a, Tensor) else a for a in args])

    def is_tensor(self, x):
        return isinstance(x, Tensor)

    def cast(self, x, dtype):
        dt = self._dtype(dtype)
        t = x if isinstance(x, Tensor) else self._convert(x)
        return self._wrap(t._t.to(dt.storage), dt)

    def shape(self, input):
        return Tensor(self, torch.tensor(list(self._convert(input).shape), dtype=torch.int32), self.int32)

    def size(self, input):
        return Tensor(self, torch.tensor(self._convert(input)._t.numel(), dtype=torch.int32), self.int32)

    def eye(self, num_rows, dtype=None):
        dt = self.float32 if dtype is None else self._dtype(dtype)
        n = int(num_rows._t.item()) if isinstance(num_rows, Tensor) else operator.index(num_rows)
        return Tensor(self, torch.eye(n, dtype=dt.storage), dt)

    def ones(self, shape, dtype=None):
        dt = self.float32 if dtype is None else self._dtype(dtype)
        return Tensor(self, torch.ones(self._dims(shape), dtype=dt.storage), dt)

    def zeros(self, shape, dtype=None):
        dt = self.float32 if dtype is None else self._dtype(dtype)
        return Tensor(self, torch.zeros(self._dims(shape), dtype=dt.storage), dt)

    def reshape(self, tensor, shape):
        t = self._convert(tensor)
        return self._wrap(t._t.reshape(self._dims(shape)), t.dtype)

    def transpose(self, a):
        t = self._convert(a)
        return self._wrap(t._t.permute(*reversed(range(t._t.dim()))), t.dtype)

    def squeeze(self, input, axis=None):
        t = self._convert(input)
        return self._wrap(t._t.squeeze() if axis is None else t._t.squeeze(operator.index(axis)), t.dtype)

    def _same(self, values):
        first = next((v for v in values if isinstance(v, Tensor)), None)
        ts = [self._convert(v, None if first is None else first.dtype) for v in values]
        for t in ts:
            if t.dtype is not ts[0].dtype:
                raise TypeError("cannot mix %r and %r tensors in one op" % (ts[0].dtype, t.dtype))
        return ts

    def concat(self, values, axis):
        ts = self._same(list(values))
        if any(t._t.dim() == 0 for t in ts):
            raise ValueError("concat: scalars cannot be concatenated")
        return self._wrap(torch.cat([t._t for t in ts], dim=operator.index(axis)), ts[0].dtype)

    def stack(self, values, axis=0):
        ts = self._same(list(values))
        return self._wrap(torch.stack([t._t for t in ts], dim=operator.index(axis)), ts[0].dtype)

    def add_n(self, inputs):
        ts = self._same(list(inputs))
        acc = ts[0]._t
        for t in ts[1:]:
            acc = acc + t._t
        return self._wrap(acc, ts[0].dtype)

    def cumsum(self, x, axis=0):
        t = self._convert(x)
        return self._wrap(torch.cumsum(t._t, dim=operator.index(axis)).to(t.dtype.storage), t.dtype)

    # ----- element-wise
    def sqrt(self, x):
        t = self._convert(x)
        return self._wrap(torch.sqrt(t._t), t.dtype)

    def abs(self, x):
        t = self._convert(x)
        return self._wrap(torch.abs(t._t), t.dtype)

    def _binary(self, x, y, fn):
        if not isinstance(x, Tensor):
            x = self._convert(x, y.dtype if isinstance(y, Tensor) else None)
        return self._wrap(fn(x._t, x._pair(y)), x.dtype)

    def maximum(self, x, y):
        return self._binary(x, y, torch.maximum)        # NaN in either operand gives NaN

    def minimum(self, x, y):
        return self._binary(x, y, torch.minimum)

    def _is_inf(self, x):
        return self._wrap(torch.isinf(self._convert(x)._t), self.bool)

    # ----- reductions
    def _reduce(self, input_tensor, axis, keepdims, fn, empty):
        t = self._convert(input_tensor)
        if axis is None:
            if t._t.numel() == 0:
                r = torch.full((), empty, dtype=t.dtype.storage)
            else:
                r = fn(t._t)
            if keepdims:
                r = r.reshape([1] * t._t.dim())
        else:
            r = fn(t._t, dim=operator.index(axis), keepdim=bool(keepdims))
        return self._wrap(r, t.dtype)

    def reduce_max(self, input_tensor, axis=None, keepdims=False):
        return self._reduce(input_tensor, axis, keepdims, torch.amax, float("-inf"))

    def reduce_sum(self, input_tensor, axis=None, keepdims=False):
        return self._reduce(input_tensor, axis, keepdims, torch.sum, 0.0)

    # ----- linear algebra
    def _matrix(self, name, x):
        t = self._convert(x)
        if t._t.dim() != 2:
            raise ValueError("%s: a matrix is required, got shape %s" % (name, list(t.shape)))
        return t

    def matmul(self, a, b, transpose_a=False, transpose_b=False):
        a, b = self._matrix("matmul", a), self._matrix("matmul", b)
        if a.dtype is not b.dtype:
            raise TypeError("matmul: cannot mix %r and %r" % (a.dtype, b.dtype))
        x = a._t.t() if transpose_a else a._t
        y = b._t.t() if transpose_b else b._t
        return self._wrap(x @ y, a.dtype)

    def _triangular_solve(self, matrix, rhs, lower=True, adjoint=False):
        a, b = self._matrix("triangular_solve", matrix), self._matrix("triangular_solve", rhs)
        if a.dtype is not b.dtype:
            raise TypeError("triangular_solve: cannot mix %r and %r" % (a.dtype, b.dtype))
        if a.shape[0] != a.shape[1] or a.shape[0] != b.shape[0]:
            raise ValueError("triangular_solve: shapes %s and %s do not fit" % (list(a.shape), list(b.shape)))
        tri = torch.tril(a._t) if lower else torch.triu(a._t)       # the other triangle is never read
        upper = not lower
        if adjoint:
            tri, upper = tri.t(), not upper
        return self._wrap(torch.linalg.solve_triangular(tri, b._t, upper=upper), a.dtype)

    def _solve(self, matrix, rhs, adjoint=False):
        a, b = self._matrix("solve", matrix), self._matrix("solve", rhs)
        if a.dtype is not b.dtype:
            raise TypeError("solve: cannot mix %r and %r" % (a.dtype, b.dtype))
        return self._wrap(torch.linalg.solve(a._t.t() if adjoint else a._t, b._t), a.dtype)

    def _band_part(self, input, num_lower, num_upper):
        t = self._matrix("band_part", input)
        lo, up = operator.index(num_lower), operator.index(num_upper)
        m, n = t.shape
        i, j = torch.arange(m)[:, None], torch.arange(n)[None, :]
        keep = ((i - j <= lo) if lo >= 0 else torch.ones(m, n, dtype=torch.bool)) & \
               ((j - i <= up) if up >= 0 else torch.ones(m, n, dtype=torch.bool))
        return self._wrap(torch.where(keep, t._t, torch.zeros((), dtype=t.dtype.storage)), t.dtype)

    def _diag_part(self, input):
        t = self._matrix("diag_part", input)
        return self._wrap(torch.diagonal(t._t), t.dtype)

    # ----- tf.random, tf.nest
    def _set_seed(self, seed):
        self._rng.manual_seed(operator.index(seed))

    def _normal(self, shape, mean=0.0, stddev=1.0, dtype=None, seed=None):
        dt = self.float32 if dtype is None else self._dtype(dtype)
        if seed is not None:
            raise TypeError("tf_standin: random.normal(seed=) is not implemented")
        x = Tensor(self, torch.randn(self._dims(shape), generator=self._rng, dtype=dt.storage), dt)
        return x * stddev + mean

    def _uniform(self, shape, minval=0, maxval=None, dtype=None, seed=None):
        dt = self.float32 if dtype is None else self._dtype(dtype)
        if seed is not None or not dt.is_floating:
            raise TypeError("tf_standin: random.uniform is implemented for floating dtypes without seed=")
        hi = 1 if maxval is None else maxval
        x = Tensor(self, torch.rand(self._dims(shape), generator=self._rng, dtype=dt.storage), dt)
        return x * (hi - minval) + minval

    def _flatten(self, structure):
        if isinstance(structure, dict):
            return [x for k in sorted(structure) for x in self._flatten(structure[k])]
        if isinstance(structure, (list, tuple)):
            return [x for s in structure for x in self._flatten(s)]
        return [structure]

