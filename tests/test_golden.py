"""Golden vectors (tests/golden/*.npz, made by tests/golden/make_golden.py from the fp64 oracle).
CPU: the oracle still reproduces them (fp64, to 1e-13: BLAS summation order may differ between
hosts) and within rounding in fp32; and it agrees with what the reference's own program text gives for the same
inputs (tests/golden/tf/*.npz, made by tests/golden/make_golden_tf.py on a stand-in for TensorFlow's ops).
GPU: the HIP path matches them to the stated tolerances."""
import glob
import os

import numpy as np
import pytest

from oracle import psgd_oracle as orc
from tests.uvd_cases import rel_err

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UVD = sorted(glob.glob(os.path.join(HERE, "uvd_*.npz")))
KRON = sorted(glob.glob(os.path.join(HERE, "kron_*.npz")))
SPLU = sorted(glob.glob(os.path.join(HERE, "splu_*.npz")))
STEP = sorted(glob.glob(os.path.join(HERE, "uvdstep_*.npz")))
SPLU_KEYS = ("L12", "l3", "U12", "u3")
UVD_STEP_SHAPES = [(2, 30), (30, 30), (30,), (30, 1), (1,)]        # rnn_xor_UVd_preconditioner.py:28-31 -> 1021 parameters


@pytest.mark.parametrize("path", UVD, ids=os.path.basename)
def test_oracle_reproduces_uvd_golden(path):
    z = np.load(path)
    q = {k: z[k].astype(np.float64) for k in ("U", "V", "d", "g", "v", "h")}
    assert rel_err(orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"]), z["pre_grad_before"]) < 1e-13
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], float(z["step"]), float(z["tiny"]),
                                 balance=bool(z["balance"]), update_U=bool(z["update_U"]))
    for k in ("U", "V", "d"):
        assert rel_err(q[k], z[k + "_new"]) < 1e-13, k
    # the fp32 run of the same op sequence stays within fp32 rounding of the golden
    p = {k: z[k].copy() for k in ("U", "V", "d", "g", "v", "h")}
    orc.update_precond_UVd_math_(p["U"], p["V"], p["d"], p["v"], p["h"], float(z["step"]), float(z["tiny"]),
                                 balance=bool(z["balance"]), update_U=bool(z["update_U"]))
    for k in ("U", "V", "d"):
        assert rel_err(p[k], z[k + "_new"]) < 1e-5
    assert rel_err(orc.precond_grad_UVd_math(p["U"], p["V"], p["d"], p["g"]), z["pre_grad_after"]) < 1e-5


@pytest.mark.parametrize("path", KRON, ids=os.path.basename)
def test_oracle_reproduces_kron_golden(path):
    z = np.load(path)
    f = lambda k: z[k].astype(np.float64)
    a, b = orc.update_precond_kron(f("Ql"), f("Qr"), f("dX"), f("dG"), float(z["step"]))
    assert rel_err(a, z["Ql_new"]) < 1e-13 and rel_err(b, z["Qr_new"]) < 1e-13
    assert rel_err(orc.precond_grad_kron(f("Ql"), f("Qr"), f("G")), z["pre_grad"]) < 1e-13


def _step_oracle(z, dt):
    f = lambda k: z[k].astype(dt)
    p, c, b, e, vs = f("p"), f("c"), f("b"), f("e"), f("vs")
    loss = np.sum(0.5 * c * p * p + b * p + 0.25 * e * p ** 4)
    grad, hv = c * p + b + e * p ** 3, (c + 3.0 * e * p * p) * vs
    U, V, d = f("U"), f("V"), f("d")
    unfl = lambda x: orc.uvd_unflatten(x, UVD_STEP_SHAPES)
    new = orc.uvd_step(unfl(p), unfl(grad), unfl(hv), unfl(vs), U, V, d, float(z["lr_params"]), float(z["lr_preconditioner"]),
                       float(z["grad_clip_max_norm"]), float(z["tiny"]), balance=bool(z["balance"]), update_U=bool(z["update_U"]))
    return loss, orc.uvd_flatten(new, dt), U, V, d


@pytest.mark.parametrize("path", STEP, ids=os.path.basename)
def test_oracle_reproduces_uvd_step_golden(path):
    z = np.load(path)
    loss, p_new, U, V, d = _step_oracle(z, np.float64)
    assert abs(loss - float(z["loss"])) < 1e-12 * abs(float(z["loss"]))
    for got, key in ((p_new, "p_new"), (U, "U_new"), (V, "V_new"), (d, "d_new")):
        assert rel_err(got, z[key]) < 1e-13, key
    assert rel_err(p_new, z["p"].astype(np.float64)) > 1e-3            # the step moved the parameters
    loss32, p32, U32, V32, d32 = _step_oracle(z, np.float32)           # fp32 run of the same op sequence
    for got, key in ((p32, "p_new"), (U32, "U_new"), (V32, "V_new"), (d32, "d_new")):
        assert rel_err(got, z[key]) < 1e-5, key


@pytest.mark.gpu
@pytest.mark.parametrize("path", STEP, ids=os.path.basename)
def test_hip_uvd_step_matches_golden(path, hip_lib, monkeypatch):
    """class UVd of the product on the fixture: same separable loss as a torch closure (autograd makes grads and Hv),
    the probe vectors and the three coin flips are the fixture's (injected where the step draws them)."""
    import torch
    import preconditioned_stochastic_gradient_descent as shim
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as mod
    z = np.load(path)
    dev = torch.device("cuda:0")

    def unfl(x):
        return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in orc.uvd_unflatten(x, UVD_STEP_SHAPES)]
    params = [t.requires_grad_(True) for t in unfl(z["p"])]
    cs, bs, es, vs = unfl(z["c"]), unfl(z["b"]), unfl(z["e"]), unfl(z["vs"])
    max_norm = float(z["grad_clip_max_norm"])
    opt = shim.UVd(params, rank_of_modification=int(z["rank"]), lr_params=float(z["lr_params"]),
                   lr_preconditioner=float(z["lr_preconditioner"]), grad_clip_max_norm=(None if np.isinf(max_norm) else max_norm))
    assert opt._param_sizes == [60, 900, 30, 30, 1] and opt._U.shape == (1021, 10)
    for t, k in ((opt._U, "U"), (opt._V, "V"), (opt._d, "d")):
        t.copy_(torch.from_numpy(z[k]).to(dev))
    coins = [True, bool(z["balance"]), bool(z["update_U"])]            # psgd.py:703, :562, :588 in the order they are drawn
    monkeypatch.setattr(mod, "_draw_branch", lambda p, gen: coins.pop(0))
    queue = list(vs)
    monkeypatch.setattr(torch, "randn_like", lambda t, **k: queue.pop(0))

    def closure():
        return sum(torch.sum(0.5 * c * p * p + b * p + 0.25 * e * p ** 4) for p, c, b, e in zip(params, cs, bs, es))
    loss = opt.step(closure)
    monkeypatch.undo()
    assert not coins and not queue
    assert abs(float(loss) - float(z["loss"])) < 1e-5 * abs(float(z["loss"]))
    p_new = np.concatenate([p.detach().reshape(-1).cpu().numpy() for p in params])
    assert rel_err(p_new, z["p_new"]) < 1e-5
    for t, k in ((opt._U, "U_new"), (opt._V, "V_new"), (opt._d, "d_new")):
        assert rel_err(t.cpu().numpy(), z[k]) < 1e-5, k


@pytest.mark.parametrize("path", SPLU, ids=os.path.basename)
def test_oracle_reproduces_splu_golden(path):
    z = np.load(path)
    f = lambda k: z[k].astype(np.float64)
    new = orc.update_precond_splu(f("L12"), f("l3"), f("U12"), f("u3"), [f("dx")], [f("dg")], float(z["step"]))
    for k, a in zip(SPLU_KEYS, new):
        assert rel_err(a, z[k + "_new"]) < 1e-13, k
    assert rel_err(orc.precond_grad_splu(f("L12"), f("l3"), f("U12"), f("u3"), [f("g")])[0], z["pre_grad"]) < 1e-13
    new32 = orc.update_precond_splu(z["L12"], z["l3"], z["U12"], z["u3"], [z["dx"]], [z["dg"]], float(z["step"]))
    for k, a in zip(SPLU_KEYS, new32):
        assert rel_err(a, z[k + "_new"]) < 1e-5, k


@pytest.mark.gpu
@pytest.mark.parametrize("path", SPLU, ids=os.path.basename)
def test_hip_matches_splu_golden(path, hip_lib):
    import torch
    import preconditioned_stochastic_gradient_descent as psgd
    z = np.load(path)
    c = lambda k: torch.from_numpy(z[k]).cuda()
    new = psgd.update_precond_splu(c("L12"), c("l3"), c("U12"), c("u3"), [c("dx")], [c("dg")], float(z["step"]))
    for k, a in zip(SPLU_KEYS, new):
        assert rel_err(a.cpu().numpy(), z[k + "_new"]) < 1e-5, k
    out = psgd.precond_grad_splu(c("L12"), c("l3"), c("U12"), c("u3"), [c("g")])[0]
    assert rel_err(out.cpu().numpy(), z["pre_grad"]) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("path", UVD, ids=os.path.basename)
def test_hip_matches_uvd_golden(path, hip_lib):
    import torch
    import preconditioned_stochastic_gradient_descent as psgd
    z = np.load(path)
    t = {k: torch.from_numpy(z[k]).cuda() for k in ("U", "V", "d", "g", "v", "h")}
    out0 = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"])
    assert rel_err(out0.cpu().numpy(), z["pre_grad_before"]) < 1e-5
    psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], float(z["step"]), float(z["tiny"]),
                                  balance=bool(z["balance"]), update_U=bool(z["update_U"]))
    for k in ("U", "V", "d"):
        assert rel_err(t[k].cpu().numpy(), z[k + "_new"]) < 1e-5, k
    out1 = psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"])
    assert rel_err(out1.cpu().numpy(), z["pre_grad_after"]) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("path", KRON, ids=os.path.basename)
def test_hip_matches_kron_golden(path, hip_lib):
    import torch
    import preconditioned_stochastic_gradient_descent as psgd
    z = np.load(path)
    c = lambda k: torch.from_numpy(z[k]).cuda()
    a, b = psgd.update_precond_kron(c("Ql"), c("Qr"), c("dX"), c("dG"), float(z["step"]))
    assert rel_err(a.cpu().numpy(), z["Ql_new"]) < 1e-5 and rel_err(b.cpu().numpy(), z["Qr_new"]) < 1e-5
    out = psgd.precond_grad_kron(c("Ql"), c("Qr"), c("G"))
    assert rel_err(out.cpu().numpy(), z["pre_grad"]) < 1e-5


# ----------------------------------------------------------------------------- reference-made fixtures
# tests/golden/tf/*.npz are outputs of the REFERENCE'S OWN PROGRAM TEXT for the inputs of the fixtures above, made by
# tests/golden/make_golden_tf.py: executed on oracle/tf_standin (TensorFlow's documented op semantics on torch CPU tensors;
# TensorFlow's own kernels have not been run), once as written in float32 and once with tf.float32 mapped to 64-bit.
from tests.golden import make_golden as gen_in          # noqa: E402
from tests.golden import make_golden_tf as gen_tf       # noqa: E402

TF_DIR = os.path.join(HERE, "tf")
TF_NAMES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(TF_DIR, "*.npz")))
F32_BAR = 1e-5                    # BASELINE north_star: fp32 reference against the fp64 oracle
# fp64 oracle against the float64 run of the reference, per family: ten times the largest rel_err measured over the family's
# files, rounded up to a power of ten (profiles/reference_parity.txt holds the figures); none may exceed REF_CAP.
REF_CAP = 1e-9
F64_BARS = {"dense": 1e-13, "kron": 1e-13, "splu": 1e-13, "uvd": 1e-13, "uvdstep": 1e-14, "uvdfd": 1e-12}


def family_of(name):
    return name.split("_", 1)[0]


def oracle_outputs(name, dt=np.float64):
    """What the oracle gives, in dtype dt, for the inputs of fixture `name`, under the keys of the reference-made file."""
    if name == gen_tf.HELLO:
        a = lambda x: np.array(x, dtype=dt)
        Q = orc.update_precond_dense(a(np.float32(0.1)) * np.eye(2, dtype=dt), [a(1.0), a(0.0)], [a(802.0), a(400.0)], 0.2)
        return dict(Q_new=Q, pre_grad=np.array([float(x) for x in orc.precond_grad_dense(Q, [a(-4.0), a(0.0)])]))
    z = np.load(os.path.join(HERE, name))
    f = lambda k: z[k].astype(dt)
    fam = family_of(name)
    if fam == "dense":
        lst = lambda k: [f("%s_%d" % (k, i)) for i in range(int(z["n_tensors"]))]
        pre = orc.precond_grad_dense(f("Q"), lst("g"))
        assert [x.shape for x in pre] == [x.shape for x in lst("g")]
        return dict(Q_new=orc.update_precond_dense(f("Q"), lst("dx"), lst("dg"), float(z["step"])),
                    pre_grad=np.concatenate([np.reshape(x, -1) for x in pre]))
    if fam in ("uvdstep", "uvdfd"):
        loss, p_new, U, V, d = _step_oracle(z, dt) if fam == "uvdstep" else gen_in.uvd_fd_step(z, dt)
        return dict(loss=np.asarray(loss), p_new=p_new, U_new=U, V_new=V, d_new=d)
    if fam == "uvd":
        q = {k: f(k) for k in ("U", "V", "d", "g", "v", "h")}
        out = dict(pre_grad_before=orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"]))
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], float(z["step"]), float(z["tiny"]),
                                     balance=bool(z["balance"]), update_U=bool(z["update_U"]))
        out.update(U_new=q["U"], V_new=q["V"], d_new=q["d"], pre_grad_after=orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"]))
        return out
    if fam == "kron":
        a, b = orc.update_precond_kron(f("Ql"), f("Qr"), f("dX"), f("dG"), float(z["step"]))
        return dict(Ql_new=a, Qr_new=b, pre_grad=orc.precond_grad_kron(f("Ql"), f("Qr"), f("G")))
    assert fam == "splu"
    new = orc.update_precond_splu(f("L12"), f("l3"), f("U12"), f("u3"), [f("dx")], [f("dg")], float(z["step"]))
    out = {k + "_new": a for k, a in zip(SPLU_KEYS, new)}
    out["pre_grad"] = orc.precond_grad_splu(f("L12"), f("l3"), f("U12"), f("u3"), [f("g")])[0]
    return out


def worst_rel_err(got, want, suffix):
    """The largest norm-wise relative error over the outputs of one fixture (empty outputs, as l3 at N = r, must be empty)."""
    worst = 0.0
    for k, a in got.items():
        b = want[k + suffix]
        assert np.shape(a) == b.shape, k
        if b.size:
            worst = max(worst, rel_err(a, b))
    return worst


def test_fixtures_present():
    assert len(UVD) == 9 and len(KRON) == 16 and len(SPLU) == 7 and len(STEP) == 2
    assert len(glob.glob(os.path.join(HERE, "dense_*.npz"))) == 2 and len(glob.glob(os.path.join(HERE, "uvdfd_*.npz"))) == 1
    # the six sparse dispatch formats of psgd.py:86-104 are all there, at the demo's shapes
    fmts = sorted(os.path.basename(p)[len("kron_fmt_"):].rsplit("_", 1)[0] for p in KRON if "kron_fmt_" in p)
    assert fmts == ["dense_norm", "dense_scale", "norm_dense", "norm_scale", "scale_dense", "scale_norm"]
    # and the four of them that hold a normalization factor once more with ql[1, -1] != 0
    bias = sorted(os.path.basename(p)[len("kron_bias_"):].rsplit("_", 1)[0] for p in KRON if "kron_bias_" in p)
    assert bias == ["dense_norm", "norm_dense", "norm_scale", "scale_norm"]
    for p in KRON:
        for tag in ("kron_fmt_", "kron_bias_"):
            if tag in p:
                z = np.load(p)
                assert tag + orc.kron_format(z["Ql"].shape, z["Qr"].shape) in p
                for q in (z["Ql"], z["Qr"]):
                    if q.shape[0] == 2 and q.shape[1] != 2:                    # the normalization factor
                        assert (q[1, -1] != 0) == (tag == "kron_bias_")
    # the reference has run on every one of them, in both precisions, and says from which file
    inputs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "*.npz")))
    assert len(inputs) == 37 and TF_NAMES == sorted(inputs + [gen_tf.HELLO])
    shas = set()
    for name in TF_NAMES:
        t = gen_tf.read_fixture(os.path.join(TF_DIR, name))
        outs = sorted(k[:-4] for k in t if k.endswith("_f32"))
        assert outs and outs == sorted(k[:-4] for k in t if k.endswith("_f64")), name
        assert t["f32_backend"] in ("standin", "tensorflow") and t["f64_backend"] == "standin" and t["f32_version"] and t["f64_version"]
        shas.add(t["reference_sha256"])
    assert len(shas) == 1 and len(shas.pop()) == 64


def test_reference_bars_are_capped():
    assert sorted(F64_BARS) == sorted({family_of(n) for n in TF_NAMES}) and max(F64_BARS.values()) <= REF_CAP


@pytest.mark.parametrize("name", TF_NAMES)
def test_oracle_matches_reference_fixtures(name):
    """The fp64 oracle against the reference's own outputs: against its float64 run at the family's measured bar (<= 1e-9, four
    orders under the 1e-5 of every fp32 GPU test: the sharp comparison, which a wrong transpose flag, adjoint=, band_part
    triangle, misplaced tiny or inverted branch in the oracle cannot pass), and against its float32 run at 1e-5."""
    t = gen_tf.read_fixture(os.path.join(TF_DIR, name))
    got = oracle_outputs(name)
    assert sorted(got) == sorted(k[:-4] for k in t if k.endswith("_f64")), "the oracle and the reference name other outputs"
    e64, e32 = worst_rel_err(got, t, "_f64"), worst_rel_err(got, t, "_f32")
    print("reference parity %-40s fp64 %.3e  fp32 %.3e" % (name, e64, e32))
    assert e64 < F64_BARS[family_of(name)]
    assert e32 < F32_BAR


REFERENCE_DIR = gen_tf.DEFAULT_REFERENCE
HAVE_REFERENCE = os.path.isfile(os.path.join(REFERENCE_DIR, gen_tf.REFERENCE_FILE))


@pytest.fixture(scope="module")
def regenerated():
    return gen_tf.generate(REFERENCE_DIR, "standin", "float64")[0]


@pytest.mark.skipif(not HAVE_REFERENCE, reason="the reference's source is not on this machine (PSGD_REFERENCE_DIR)")
@pytest.mark.parametrize("name", TF_NAMES)
def test_reference_fixtures_regenerate(name, regenerated):
    """Where the reference's source is at hand: it is the file whose SHA-256 the fixtures record, and running it again on the
    stand-in (in memory, nothing is written) reproduces the committed float64 outputs to 1e-12."""
    t = gen_tf.read_fixture(os.path.join(TF_DIR, name))
    assert t["reference_sha256"] == gen_tf.reference_sha256(REFERENCE_DIR)
    assert worst_rel_err(regenerated[name], t, "_f64") < 1e-12
