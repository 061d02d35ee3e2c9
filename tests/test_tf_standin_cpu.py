"""oracle/tf_standin: every numerical op against an independent definition (NumPy and scipy.linalg, never torch's function
of the same name), the strictness that keeps a dropped keyword from manufacturing a false (dis)agreement, in-place
variables, and tape-in-tape against a closed-form Hessian-vector product.  The reference's program text runs on this
stand-in to make tests/golden/tf/, so it is the thing that could be wrong unnoticed."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import tf_standin

PRECISIONS = ["float32", "float64"]


@pytest.fixture(params=PRECISIONS)
def tf(request):
    return tf_standin.make(request.param)


def tol(tf, n=64):
    """n roundings of the storage precision"""
    return n * (2.0 ** -52 if tf.precision == "float64" else 2.0 ** -23)


def close(tf, got, want, scale=1.0, n=64):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want), initial=0.0) <= tol(tf, n) * scale * max(1.0, np.max(np.abs(want), initial=0.0))


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def tri_matrix(n, seed):
    """a full non-symmetric matrix whose two triangles (each with the diagonal) are both well conditioned"""
    a = 0.3 * rnd((n, n), seed) / np.sqrt(n)
    return (a + np.diag(1.0 + np.arange(n, dtype=np.float32) / n)).astype(np.float32)


def test_precision_switch(tf):
    x = tf.constant(np.float32(1.0)) / 3
    assert x.dtype is tf.float32 and tf.float32.name == "float32"
    assert x.numpy().dtype == (np.float64 if tf.precision == "float64" else np.float32)
    assert tf.constant(np.ones(2)).dtype is tf.float64 and tf.constant(1.5).dtype is tf.float32 and tf.constant(3).dtype is tf.int32
    with pytest.raises(ValueError):
        tf_standin.make("float16")


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("adjoint", [True, False])
def test_triangular_solve(tf, lower, adjoint):
    n, k = 7, 3
    A, B = tri_matrix(n, 1), rnd((n, k), 2)
    X = tf.linalg.triangular_solve(tf.constant(A), tf.constant(B), lower=lower, adjoint=adjoint).numpy()
    T = (np.tril(A) if lower else np.triu(A)).astype(np.float64)
    op = T.T if adjoint else T
    want = sla.solve_triangular(T, B.astype(np.float64), lower=lower, trans="T" if adjoint else "N")
    close(tf, X, want)
    close(tf, op @ X.astype(np.float64), B)                                            # the residual ||op(A) X - B||
    # the triangle that `lower` does not name is never read: garbage there changes nothing
    G = A.copy()
    G[np.triu_indices(n, 1) if lower else np.tril_indices(n, -1)] = np.float32(1e6)
    Xg = tf.linalg.triangular_solve(tf.constant(G), tf.constant(B), lower=lower, adjoint=adjoint).numpy()
    assert np.array_equal(X, Xg)
    # and the four combinations are four different answers on this matrix (a dropped flag cannot hide)
    other = tf.linalg.triangular_solve(tf.constant(A), tf.constant(B), lower=lower, adjoint=not adjoint).numpy()
    assert np.max(np.abs(other - X)) > 1e-2


def test_triangular_solve_defaults_are_tensorflows(tf):
    A, B = tri_matrix(5, 3), rnd((5, 2), 4)
    X = tf.linalg.triangular_solve(tf.constant(A), tf.constant(B)).numpy()               # lower=True, adjoint=False
    close(tf, X, sla.solve_triangular(np.tril(A).astype(np.float64), B.astype(np.float64), lower=True))


@pytest.mark.parametrize("adjoint", [False, True])
def test_solve(tf, adjoint):
    A = (np.eye(6) + 0.3 * rnd((6, 6), 5)).astype(np.float32)
    B = rnd((6, 2), 6)
    X = tf.linalg.solve(tf.constant(A), tf.constant(B), adjoint=adjoint).numpy()
    A64 = A.astype(np.float64)
    close(tf, X, sla.solve(A64.T if adjoint else A64, B.astype(np.float64)))
    close(tf, (A64.T if adjoint else A64) @ X, B)
    assert np.max(np.abs(X - tf.linalg.solve(tf.constant(A), tf.constant(B), adjoint=not adjoint).numpy())) > 1e-2


@pytest.mark.parametrize("shape", [(4, 7), (7, 4)])
def test_band_part(tf, shape):
    A = rnd(shape, 7)
    i, j = np.indices(shape)
    for (lo, up), keep in (((0, -1), j >= i), ((-1, 0), j <= i), ((0, 0), i == j)):
        got = tf.linalg.band_part(tf.constant(A), lo, up).numpy()
        assert np.array_equal(got, np.where(keep, A, 0))
    assert np.array_equal(tf.linalg.band_part(tf.constant(A), 0, -1).numpy(), np.triu(A))
    assert np.array_equal(tf.linalg.band_part(tf.constant(A), -1, 0).numpy(), np.tril(A))


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
def test_matmul(tf, ta, tb):
    A, B = rnd((3, 5), 8), rnd((5, 4), 9)
    a, b = (A.T.copy() if ta else A), (B.T.copy() if tb else B)
    got = tf.matmul(tf.constant(a), tf.constant(b), transpose_a=ta, transpose_b=tb).numpy()
    want = np.einsum("ik,kj->ij", A.astype(np.float64), B.astype(np.float64))
    assert got.shape == (3, 4)
    close(tf, got, want)
    if ta != tb:                                  # a dropped flag is a shape error on non-square input, not a wrong number
        with pytest.raises((RuntimeError, ValueError)):
            tf.matmul(tf.constant(a), tf.constant(b))


def test_diag_part(tf):
    for shape in ((5, 5), (6, 3), (3, 6)):
        A = rnd(shape, 10)
        got = tf.linalg.diag_part(tf.constant(A)).numpy()
        assert np.array_equal(got, np.array([A[k, k] for k in range(min(shape))]))


def test_reductions(tf):
    A = rnd((4, 6), 11)
    A64 = A.astype(np.float64)
    assert tf.reduce_max(tf.constant(A)).numpy() == A.max() and tf.reduce_max(tf.constant(A)).shape == ()
    assert np.array_equal(tf.reduce_max(tf.constant(A), axis=1).numpy(), A.max(axis=1))
    assert np.array_equal(tf.reduce_max(tf.constant(A), axis=0, keepdims=True).numpy(), A.max(axis=0, keepdims=True))
    close(tf, tf.reduce_sum(tf.constant(A)).numpy(), A64.sum())
    close(tf, tf.reduce_sum(tf.constant(A), axis=1).numpy(), A64.sum(axis=1))
    close(tf, tf.reduce_sum(tf.constant(A), axis=0, keepdims=True).numpy(), A64.sum(axis=0, keepdims=True))
    # an empty tensor: -inf and 0, as TensorFlow gives (psgd.py:411 meets it at N = r)
    assert tf.reduce_max(tf.constant(np.zeros((0, 1), np.float32))).numpy() == -np.inf
    assert tf.reduce_sum(tf.constant(np.zeros((0, 1), np.float32))).numpy() == 0.0


def test_shape_plumbing(tf):
    A, B = rnd((2, 3), 12), rnd((4, 3), 13)
    assert np.array_equal(tf.concat([tf.constant(A), tf.constant(B)], 0).numpy(), np.concatenate([A, B], 0))
    assert np.array_equal(tf.concat([tf.constant(A), tf.constant(A)], axis=1).numpy(), np.concatenate([A, A], 1))
    assert np.array_equal(tf.concat([tf.constant(A[0]), [0.0]], axis=0).numpy(), np.append(A[0], np.float32(0)))   # psgd.py:237
    assert np.array_equal(tf.stack((tf.constant(A[0]), tf.constant(A[1]))).numpy(), A)
    assert tf.squeeze(tf.constant(A[:, :1])).shape == (2,) and tf.squeeze(tf.constant(A[:1, :1])).shape == ()
    assert np.array_equal(tf.reshape(tf.constant(A), [-1, 1]).numpy(), A.reshape(-1, 1))                          # row-major
    assert np.array_equal(tf.reshape(tf.constant(A), tf.shape(tf.constant(A.T.copy()))).numpy(), A.reshape(3, 2))
    assert np.array_equal(tf.transpose(tf.constant(A)).numpy(), A.T)
    assert np.array_equal(tf.cumsum([np.int32(3), np.int32(4), np.int32(5)]).numpy(), [3, 7, 12])
    close(tf, tf.cumsum(tf.constant(A), axis=1).numpy(), np.cumsum(A.astype(np.float64), axis=1))
    x = tf.constant(A)
    assert np.array_equal(x[1:].numpy(), A[1:]) and np.array_equal(x[0, -1].numpy(), A[0, -1])
    assert np.array_equal(x[:, :2].numpy(), A[:, :2]) and x[0][:, None].shape == (3, 1)
    assert int(tf.size(x).numpy()) == 6 and list(tf.shape(x).numpy()) == [2, 3] and x.shape == (2, 3)
    assert bool(tf.shape(x)[0] < tf.shape(x)[1]) and not bool(tf.shape(x)[0] == tf.shape(x)[1])
    assert np.array_equal(tf.eye(tf.size(x[0]), dtype=x.dtype).numpy(), np.eye(3))
    assert tf.nest.flatten([x, [x, (x,)], {"b": 2, "a": 1}])[3:] == [1, 2] and tf.is_tensor(x) and not tf.is_tensor([x])


def test_maximum_minimum_propagate_nan(tf):
    nan, one = tf.constant(np.float32("nan")), tf.constant(np.float32(1.0))
    for fn in (tf.maximum, tf.minimum):
        assert np.isnan(fn(nan, one).numpy()) and np.isnan(fn(one, nan).numpy()) and np.isnan(fn(nan, 1.0).numpy())
    assert tf.maximum(one, 2.0).numpy() == 2.0 and tf.minimum(one, 2.0).numpy() == 1.0
    assert bool(tf.math.is_inf(tf.constant(1, dtype=tf.float32) / 0)) and not bool(tf.math.is_inf(one))


def test_denormal_results_flush_to_zero(tf):
    """the halving loop of psgd.py:22 ends at the smallest normal number"""
    info = np.finfo(np.float64 if tf.precision == "float64" else np.float32)
    x = tf.constant(info.tiny, dtype=tf.float32)
    assert x.numpy() == info.tiny and (x / 2).numpy() == 0.0 and (x * 0.5).numpy() == 0.0 and (x * 2 / 2).numpy() == info.tiny


def test_unknown_keyword_raises(tf):
    A, B = tf.constant(tri_matrix(4, 14)), tf.constant(rnd((4, 2), 15))
    for call in (lambda: tf.matmul(A, B, adjoint=True), lambda: tf.matmul(A, B, transpose=True),
                 lambda: tf.linalg.triangular_solve(A, B, upper=True), lambda: tf.linalg.triangular_solve(A, B, transpose_a=True),
                 lambda: tf.linalg.solve(A, B, lower=True), lambda: tf.linalg.band_part(A, 0, -1, name="x"),
                 lambda: tf.reduce_sum(A, dim=0), lambda: tf.reduce_max(A, axes=0), lambda: tf.concat([A, A], dim=0),
                 lambda: tf.random.normal([2], std=2.0), lambda: tf.random.uniform([], dtypes=tf.float32),
                 lambda: tf.Variable(1.0, trainables=False), lambda: tf.constant(1.0, type=tf.float32),
                 lambda: tf.function(input_signatures=()), lambda: tf.cast(A, dtypes=tf.float32), lambda: tf.eye(2, dtyp=tf.float32)):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(TypeError):
        tf.constant(1.0, dtype=np.float32)                      # not one of the stand-in's dtypes
    with pytest.raises(TypeError):
        tf.constant(np.ones(2)) + tf.constant(np.ones(2, np.float32))      # float64 with float32: TensorFlow does not mix them


def test_unknown_attribute_raises(tf):
    for obj, name in ((tf, "einsum"), (tf, "tensordot"), (tf.linalg, "inv"), (tf.linalg, "cholesky"), (tf.random, "gamma"),
                      (tf.math, "is_nan"), (tf.constant(1.0), "trainable"), (tf.constant(1.0), "assign"), (tf.Variable(1.0), "T")):
        with pytest.raises(AttributeError):
            getattr(obj, name)


def test_random_draws(tf):
    tf.random.set_seed(3)
    a = tf.random.normal([2000], stddev=3.0, dtype=tf.float32).numpy()
    tf.random.set_seed(3)
    b = tf.random.normal([2000], dtype=tf.float32).numpy()
    assert np.allclose(a, 3.0 * b, rtol=1e-6) and abs(np.std(b) - 1.0) < 0.1                # stddev= scales a unit draw
    u = tf.random.uniform([2000]).numpy()
    assert u.min() >= 0.0 and u.max() < 1.0 and tf.random.uniform([]).shape == ()


def test_variable_assign_mutates_in_place(tf):
    v = tf.Variable(np.array([1.0, 2.0, 3.0], np.float32), trainable=False)
    alias, snapshot = v, v.numpy()
    assert v.assign_sub(tf.constant(np.ones(3, np.float32))) is v
    assert np.array_equal(alias.numpy(), [0.0, 1.0, 2.0]) and np.array_equal(snapshot, [1.0, 2.0, 3.0])
    v.assign_add([1.0, 1.0, 1.0])
    v.assign(v * 2)
    assert np.array_equal(alias.numpy(), [2.0, 4.0, 6.0]) and alias is v and not v.trainable and tf.Variable(1.0).trainable
    with pytest.raises(ValueError):
        v.assign(tf.constant(np.ones(2, np.float32)))
    flag = tf.Variable(True, dtype=bool, trainable=False)
    assert bool(flag) and flag.dtype is tf.bool
    h = tf.Variable(0.25, dtype=tf.float32, trainable=False)
    assert (tf.constant(0.5) * h).numpy() == 0.125 and bool(tf.constant(0.1) < h)


def test_function_enforces_the_rank_of_its_signature(tf):
    @tf.function(input_signature=(tf.TensorSpec(shape=[None, None], dtype=tf.float32), tf.TensorSpec(shape=[], dtype=tf.float32)))
    def f(a, s=tf.constant(2.0)):
        return a * s
    A = tf.constant(rnd((2, 3), 16))
    assert np.array_equal(f(A).numpy(), 2 * A.numpy()) and np.array_equal(f(A, tf.constant(3.0)).numpy(), 3 * A.numpy())
    with pytest.raises(ValueError):
        f(A[0])                                                # a vector where a matrix is stated
    with pytest.raises(ValueError):
        f(A, A)                                                # a matrix where a scalar is stated
    with pytest.raises(TypeError):
        f(tf.constant(np.ones((2, 2))))                        # float64 where float32 is stated


def test_tape_in_tape_gives_the_exact_hessian_vector_product(tf):
    """loss = sum(c p^2 / 2 + b p + e p^4 / 4) over two parameters: grad = c p + b + e p^3, H v = (c + 3 e p^2) v."""
    shapes = [(3, 2), (5,)]
    arr = lambda seed: [rnd(s, seed + i) for i, s in enumerate(shapes)]
    p0, c, b, e, v = arr(20), arr(30), arr(40), arr(50), arr(60)
    params = [tf.Variable(x) for x in p0]
    frozen = tf.Variable(np.float32(2.0), trainable=False)
    cs, bs, es, vs = ([tf.constant(x) for x in xs] for xs in (c, b, e, v))
    with tf.GradientTape() as g2:
        with tf.GradientTape() as g1:
            loss = tf.add_n([tf.reduce_sum(0.5 * c_ * p * p + b_ * p + 0.25 * e_ * p * p * p * p)
                             for p, c_, b_, e_ in zip(params, cs, bs, es)]) * frozen / frozen
        grads = g1.gradient(loss, params)
    hvs = g2.gradient(grads, params, vs)
    f = lambda xs: [x.astype(np.float64) for x in xs]
    for g, h, p_, c_, b_, e_, v_ in zip(grads, hvs, f(p0), f(c), f(b), f(e), f(v)):
        close(tf, g.numpy(), c_ * p_ + b_ + e_ * p_ ** 3, scale=20)
        close(tf, h.numpy(), (c_ + 3 * e_ * p_ * p_) * v_, scale=20)
    with pytest.raises(RuntimeError):
        g1.gradient(loss, params)                              # not persistent: one gradient call
    # nothing records outside a tape, and a variable that the loss does not touch has no gradient
    outside = params[0] * params[0]
    with tf.GradientTape() as g3:
        inside = tf.reduce_sum(params[0] * params[0])
    assert not outside._t.requires_grad
    g = g3.gradient(inside, params)
    close(tf, g[0].numpy(), 2 * p0[0].astype(np.float64))
    assert g[1] is None
