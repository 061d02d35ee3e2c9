"""Regenerates the reference-made fixtures of tests/golden/tf/ FROM THE REFERENCE ITSELF.

    python tests/golden/make_golden_tf.py [--reference DIR] [--out tests/golden/tf]
                                          [--backend {tensorflow,standin}] [--precision {float32,float64}]

A tool for wherever the reference's source is at hand (DIR, or $PSGD_REFERENCE_DIR); never imported by the product.  It loads
the reference's preconditioned_stochastic_gradient_descent.py unmodified (psgd.py below), feeds it the INPUTS of every
committed oracle-made fixture (tests/golden/*.npz: same seeds, same arrays) and writes the reference's own outputs to
tests/golden/tf/<case>.npz, plus dense_hello_first_step.npz.  tests/test_golden.py compares the oracle with those files, and
tests/test_reference_fixtures_gpu.py the HIP kernels.  The files are data: arrays and metadata strings, no reference source.

What `import tensorflow` (psgd.py:18) resolves to is the backend:
  standin     oracle/tf_standin: the ~36 tf.* names the reference touches, written from TensorFlow's documented semantics on
              torch CPU tensors.  It is placed in sys.modules["tensorflow"] of this process only while the reference loads.
              Default where TensorFlow is not importable.
  tensorflow  TensorFlow's own kernels.  Not yet run anywhere this project is built (no wheel); kept for wherever it can be.
Both precisions are recorded: float32 is the reference as written (dtype = tf.float32, psgd.py:20); float64 is the same
program text with the stand-in's tf.float32 mapped to 64-bit storage, i.e. the reference's formulas, op order and branch logic
without fp32 noise (always made by the stand-in).  --precision re-makes one half and keeps the other half of an existing file.

File layout: for every output X of the reference, X_f32 (float32) and X_f64_minus_f32 (float32: the float64 result minus
the widened float32 one; X_f64 = X_f32 + that, good to 2^-24 of the difference of the two runs, which keeps every file far
below 1 MiB) -- or X_same_as_input naming the input array that both runs returned bit for bit (the factor that an update
leaves alone).  read_fixture() below undoes this and returns X_f32 / X_f64.  Metadata: backend and version of either half,
and the SHA-256 of the reference file that ran.

Covered: UVd math (both factor branches, the balance branch, ranks 1 .. 40, N < r, matrix g), whole UVd.step calls with the
exact and with the finite-difference Hessian-vector product, Kron dense (x) dense and the sparse dispatch formats (with and
without ql[1, -1]), sparse LU, the dense preconditioner on tensor lists, and the dense 2 x 2 first step of hello_psgd.py.

The reference draws its branch decisions from tf.random.uniform([]) (psgd.py:562, :588, :703) and its probe vectors from
tf.random.normal (:713, :721).  To drive every branch deterministically the script substitutes those two calls, for the
duration of one call into the reference, by functions that hand out pre-chosen numbers (0.0 -> branch taken, 1.0 -> not
taken; the fixture's unit-normal vectors times the stddev= the reference asks for); nothing else is touched.
"""
import argparse
import glob
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE_FILE = "preconditioned_stochastic_gradient_descent.py"
DEFAULT_REFERENCE = os.environ.get("PSGD_REFERENCE_DIR", "/root/reference")
HELLO = "dense_hello_first_step.npz"


def reference_sha256(ref_dir):
    with open(os.path.join(ref_dir, REFERENCE_FILE), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def have_tensorflow():
    return importlib.util.find_spec("tensorflow") is not None


class deep_recursion:
    """psgd.py:22 and :682 halve 1.0 recursively down to tiny: 1022 frames in float64, more than Python allows by default."""

    def __enter__(self):
        self.limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(self.limit, 4000))

    def __exit__(self, *exc):
        sys.setrecursionlimit(self.limit)


def load_reference(ref_dir, backend="tensorflow", precision="float32"):
    """(reference module, the tf it runs on).  The stand-in is in sys.modules["tensorflow"] only while the reference loads."""
    path = os.path.join(ref_dir, REFERENCE_FILE)
    spec = importlib.util.spec_from_file_location("psgd_reference_%s_%s" % (backend, precision), path)
    mod = importlib.util.module_from_spec(spec)
    if backend == "tensorflow":
        if precision != "float32":
            raise ValueError("TensorFlow runs the reference as written, in float32; float64 is the stand-in's")
        import tensorflow as tf
        spec.loader.exec_module(mod)       # raises ModuleNotFoundError above when TensorFlow is absent
        return mod, tf
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import tf_standin
    tf = tf_standin.make(precision)
    saved = sys.modules.get("tensorflow")
    sys.modules["tensorflow"] = tf
    try:
        with deep_recursion():
            spec.loader.exec_module(mod)
    finally:
        if saved is None:
            del sys.modules["tensorflow"]
        else:
            sys.modules["tensorflow"] = saved
    return mod, tf


class Coins:
    """tf.random.uniform([]) replacement for one call: returns the queued scalars in order."""

    def __init__(self, tf, values):
        self.tf, self.values, self.saved = tf, list(values), None

    def __enter__(self):
        self.saved = self.tf.random.uniform
        tf, values = self.tf, self.values

        def uniform(shape, *a, **k):
            assert list(shape) == [] and values, "unexpected random draw in the reference"
            return tf.constant(values.pop(0), dtype=tf.float32)
        self.tf.random.uniform = uniform
        return self

    def __exit__(self, *exc):
        self.tf.random.uniform = self.saved
        assert not self.values, "the reference drew fewer numbers than expected"


def uvd_case(ref, tf, z):
    U, V, d = (tf.Variable(z[k]) for k in ("U", "V", "d"))
    g, v, h = (tf.constant(z[k]) for k in ("g", "v", "h"))
    pre0 = ref.precond_grad_UVd_math(U, V, d, g).numpy()
    coins = [0.0 if bool(z["balance"]) else 1.0, 0.0 if bool(z["update_U"]) else 1.0]      # psgd.py:562 then :588
    with Coins(tf, coins):
        ref.update_precond_UVd_math_(U, V, d, v, h, tf.constant(float(z["step"]), tf.float32),
                                     tf.constant(float(z["tiny"]), tf.float32))
    pre1 = ref.precond_grad_UVd_math(U, V, d, g).numpy()
    return dict(pre_grad_before=pre0, U_new=U.numpy(), V_new=V.numpy(), d_new=d.numpy(), pre_grad_after=pre1)


def kron_case(ref, tf, z):
    c = lambda k: tf.constant(z[k])
    Ql_new, Qr_new = ref.update_precond_kron(c("Ql"), c("Qr"), c("dX"), c("dG"), tf.constant(float(z["step"]), tf.float32))
    pre = ref.precond_grad_kron(c("Ql"), c("Qr"), c("G"))
    return dict(Ql_new=Ql_new.numpy(), Qr_new=Qr_new.numpy(), pre_grad=pre.numpy())


def splu_case(ref, tf, z):
    c = lambda k: tf.constant(z[k])
    pre = ref.precond_grad_splu(c("L12"), c("l3"), c("U12"), c("u3"), [c("g")])[0]
    new = ref.update_precond_splu(c("L12"), c("l3"), c("U12"), c("u3"), [c("dx")], [c("dg")], float(z["step"]))
    return dict(pre_grad=pre.numpy(), L12_new=new[0].numpy(), l3_new=new[1].numpy(), U12_new=new[2].numpy(),
                u3_new=new[3].numpy())


class Normals:
    """tf.random.normal replacement for one UVd.step call: hands out the fixture's probe vectors, one per parameter,
    in parameter order (psgd.py:713 draws them with tf.random.normal(param.shape))."""

    def __init__(self, tf, arrays):
        self.tf, self.arrays, self.saved = tf, list(arrays), None

    def __enter__(self):
        self.saved = self.tf.random.normal
        tf, arrays = self.tf, self.arrays

        def normal(shape, *a, **k):
            x = arrays.pop(0)
            assert tuple(shape) == tuple(x.shape) and not a, "unexpected probe-vector draw in the reference"
            assert set(k) <= {"stddev", "dtype"}, "unexpected keyword in the reference's probe-vector draw"
            return tf.constant(x) * k["stddev"] if "stddev" in k else tf.constant(x)      # psgd.py:721 / :713
        self.tf.random.normal = normal
        return self

    def __exit__(self, *exc):
        self.tf.random.normal = self.saved
        assert not self.arrays, "the reference drew fewer probe vectors than expected"


UVD_STEP_SHAPES = [(2, 30), (30, 30), (30,), (30, 1), (1,)]        # rnn_xor_UVd_preconditioner.py:28-31


def uvd_step_case(ref, tf, z, exact=True):
    """One UVd.step of the reference itself (psgd.py:692-764) on the fixture's inputs: the closure is the separable
    loss sum(c p^2 / 2 + b p + e p^4 / 4) (TensorFlow differentiates it twice on its own, or once at two points when
    exact=False), the probe vectors and the three coin flips (:703 update, :562 balance, :588 which factor) are the fixture's."""
    def unfl(x):
        out, i = [], 0
        for s in UVD_STEP_SHAPES:
            n = int(np.prod(s))
            out.append(np.reshape(x[i:i + n], s))
            i += n
        return out
    params = [tf.Variable(x) for x in unfl(z["p"])]
    cs, bs, es = ([tf.constant(x) for x in unfl(z[k])] for k in ("c", "b", "e"))
    max_norm = float(z["grad_clip_max_norm"])
    opt = ref.UVd(params, rank_of_modification=int(z["rank"]), preconditioner_init_scale=1.0,
                  lr_params=float(z["lr_params"]), lr_preconditioner=float(z["lr_preconditioner"]),
                  grad_clip_max_norm=(None if np.isinf(max_norm) else max_norm),
                  preconditioner_update_probability=1.0, exact_hessian_vector_product=exact)
    opt._U.assign(z["U"]); opt._V.assign(z["V"]); opt._d.assign(z["d"])
    tf.random.set_seed(0)                      # (the closure draws nothing; Note 1 of psgd.py:645-651 asks for it all the same)

    def closure():
        return tf.add_n([tf.reduce_sum(0.5 * c * p * p + b * p + 0.25 * e * p * p * p * p)
                         for p, c, b, e in zip(params, cs, bs, es)])
    coins = [0.0, 0.0 if bool(z["balance"]) else 1.0, 0.0 if bool(z["update_U"]) else 1.0]
    with Coins(tf, coins), Normals(tf, unfl(z["vs"])):
        loss = opt.step(closure)
    p_new = np.concatenate([np.reshape(p.numpy(), [-1]) for p in params], 0)
    return dict(loss=np.asarray(loss.numpy()), p_new=p_new, U_new=opt._U.numpy(), V_new=opt._V.numpy(), d_new=opt._d.numpy())


def uvd_fd_step_case(ref, tf, z):
    """The finite-difference branch of UVd.step (psgd.py:715-727, :734-736, :760-762); Normals hands out the perturbation."""
    return uvd_step_case(ref, tf, z, exact=False)


def dense_case(ref, tf, z):
    """update_precond_dense / precond_grad_dense (psgd.py:26-63) on the fixture's lists of mixed-shape tensors."""
    n = int(z["n_tensors"])
    lst = lambda k: [tf.constant(z["%s_%d" % (k, i)]) for i in range(n)]
    Q = tf.constant(z["Q"])
    Qn = ref.update_precond_dense(Q, lst("dx"), lst("dg"), step=float(z["step"]))
    gs = lst("g")
    pre = ref.precond_grad_dense(Q, gs)
    assert [tuple(p.shape) for p in pre] == [tuple(g.shape) for g in gs]               # :57-61 restores the shapes
    return dict(Q_new=Qn.numpy(), pre_grad=np.concatenate([np.reshape(p.numpy(), [-1]) for p in pre], 0))


def dense_hello_case(ref, tf):
    """hello_psgd.py:7-12,25-26 first iteration with v = (1, 0) (KAT-R of SURVEY Appendix C)."""
    Q = tf.constant(0.1 * np.eye(2, dtype=np.float32))
    dxs = [tf.constant(1.0), tf.constant(0.0)]
    dgs = [tf.constant(802.0), tf.constant(400.0)]
    Qn = ref.update_precond_dense(Q, dxs, dgs, step=0.2)
    pre = ref.precond_grad_dense(Qn, [tf.constant(-4.0), tf.constant(0.0)])
    return dict(Q_new=Qn.numpy(), pre_grad=np.array([p.numpy() for p in pre]))


FAMILIES = (("uvdstep_", uvd_step_case), ("uvdfd_", uvd_fd_step_case), ("uvd_", uvd_case), ("kron_", kron_case),
            ("splu_", splu_case), ("dense_", dense_case))


def input_fixtures():
    return sorted(glob.glob(os.path.join(HERE, "*.npz")))


def run_case(name, ref, tf):
    """The reference's outputs (NumPy arrays, in the precision `tf` runs at) for the fixture file `name`."""
    if name == HELLO:
        return dense_hello_case(ref, tf)
    z = np.load(os.path.join(HERE, name))
    fn = next(f for prefix, f in FAMILIES if name.startswith(prefix))
    return fn(ref, tf, z)


def encode(name, out32, out64):
    """The arrays of one fixture file from the outputs of the two runs (layout: the module docstring)."""
    z = np.load(os.path.join(HERE, name)) if name != HELLO else None
    rec = {}
    for k in out32:
        a32, a64 = np.asarray(out32[k], dtype=np.float32), np.asarray(out64[k], dtype=np.float64)
        assert a32.shape == a64.shape, (name, k)
        src = k[:-len("_new")] if k.endswith("_new") else None
        if z is not None and src in z.files and z[src].shape == a32.shape and a32.size and \
                np.array_equal(a32, z[src]) and np.array_equal(a64, z[src].astype(np.float64)):
            rec[k + "_same_as_input"] = src
        else:
            rec[k + "_f32"] = a32
            rec[k + "_f64_minus_f32"] = (a64 - a32.astype(np.float64)).astype(np.float32)
    return rec


def read_fixture(path):
    """A file of tests/golden/tf/ as a dict: X_f32 and X_f64 for every output X, and the metadata strings."""
    t = np.load(path)
    out = {}
    for k in t.files:
        if k.endswith("_f64_minus_f32"):
            x = k[:-len("_f64_minus_f32")]
            out[x + "_f64"] = t[x + "_f32"].astype(np.float64) + t[k].astype(np.float64)
        elif k.endswith("_same_as_input"):
            x, src = k[:-len("_same_as_input")], str(t[k])
            a = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(path))), os.path.basename(path)))[src]
            out[x + "_f32"], out[x + "_f64"] = a.astype(np.float32), a.astype(np.float64)
        elif k.endswith("_f32"):
            out[k] = t[k]
        else:
            out[k] = str(t[k])
    return out


def generate(ref_dir, backend="standin", precision="float64", names=None):
    """{file name: {output: array}} of the reference at one precision, in memory (the regeneration check of
    tests/test_golden.py runs this)."""
    ref, tf = load_reference(ref_dir, backend, precision)
    names = [os.path.basename(p) for p in input_fixtures()] + [HELLO] if names is None else names
    with deep_recursion():
        return {name: run_case(name, ref, tf) for name in names}, tf.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=DEFAULT_REFERENCE)
    ap.add_argument("--out", default=os.path.join(HERE, "tf"))
    ap.add_argument("--backend", choices=("tensorflow", "standin"), default="tensorflow" if have_tensorflow() else "standin",
                    help="what runs the float32 half (the float64 half is always the stand-in's)")
    ap.add_argument("--precision", choices=("float32", "float64"), default=None,
                    help="re-make only this half and keep the other from the existing files (default: both)")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    sha = reference_sha256(args.reference)
    halves = {}
    if args.precision in (None, "float32"):
        halves["f32"] = generate(args.reference, args.backend, "float32") + (args.backend,)
    if args.precision in (None, "float64"):
        halves["f64"] = generate(args.reference, "standin", "float64") + ("standin",)
    names = [os.path.basename(p) for p in input_fixtures()] + [HELLO]
    for name in names:
        path = os.path.join(args.out, name)
        old = read_fixture(path) if len(halves) < 2 else None
        if old is not None and old["reference_sha256"] != sha:
            sys.exit("make_golden_tf.py: %s was made from another reference file; re-make both halves" % name)
        outs, meta = {}, dict(generator="tests/golden/make_golden_tf.py", reference_sha256=sha)
        for h in ("f32", "f64"):
            if h in halves:
                cases, version, backend = halves[h]
                outs[h] = cases[name]
                meta[h + "_backend"], meta[h + "_version"] = backend, version
            else:
                outs[h] = {k[:-4]: v for k, v in old.items() if k.endswith("_" + h)}
                meta[h + "_backend"], meta[h + "_version"] = old[h + "_backend"], old[h + "_version"]
        np.savez_compressed(path, **encode(name, outs["f32"], outs["f64"]), **meta)
        print("wrote", name)
    print("reference fixtures written to", args.out, "(%s)" % ", ".join("%s: %s %s" % (h, v[2], v[1]) for h, v in halves.items()))


if __name__ == "__main__":
    main()
