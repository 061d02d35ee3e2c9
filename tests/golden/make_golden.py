"""Generates the committed golden vectors in this directory.

These are NOT outputs of the reference itself: they are outputs of the fp64 run of the CPU oracle
(oracle/psgd_oracle.py).  The reference's own outputs for the same inputs are in tests/golden/tf/
(make_golden_tf.py); run that after this whenever a case is added or its inputs change.
They freeze the oracle (any later edit that changes its results fails the golden tests) and give
the GPU tests inputs/outputs that do not depend on NumPy's RNG stream.

    python tests/golden/make_golden.py        (run from the repository root)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import psgd_oracle as orc          # noqa: E402
from tests.uvd_cases import make_uvd_problem   # noqa: E402
from tests.splu_cases import make_splu_problem  # noqa: E402
from tests.kron_cases import illcond_factor     # noqa: E402

TINY32 = float(np.finfo(np.float32).tiny)


def uvd_case(name, N, r, seed, uv_gain, d_spread, balance, update_U, g_cols=1):
    p = make_uvd_problem(N, r, seed=seed, uv_gain=uv_gain, d_spread=d_spread)
    if balance:
        p["U"] *= 6.0
    if g_cols > 1:                                                  # a matrix g (psgd.py:623): d broadcasts over its columns
        p["g"] = np.random.default_rng(1000 + seed).standard_normal((N, g_cols)).astype(np.float32)
    q = {k: v.astype(np.float64) for k, v in p.items()}
    pre0 = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])
    orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], 0.01, TINY32, balance=balance, update_U=update_U)
    pre1 = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])
    np.savez_compressed(os.path.join(HERE, name + ".npz"), U=p["U"], V=p["V"], d=p["d"], g=p["g"], v=p["v"], h=p["h"],
                        step=0.01, tiny=TINY32, balance=balance, update_U=update_U,
                        pre_grad_before=pre0, U_new=q["U"], V_new=q["V"], d_new=q["d"], pre_grad_after=pre1)


def kron_case(name, M, N, seed):
    rng = np.random.default_rng(seed)
    tri = lambda n: np.triu(rng.standard_normal((n, n)) * 0.05, 1) + np.diag(np.exp(0.3 * rng.standard_normal(n)))
    Ql, Qr = (tri(M) * 2.0).astype(np.float32), tri(N).astype(np.float32)
    dX = rng.standard_normal((M, N)).astype(np.float32)
    dG = (np.diag(np.exp(rng.uniform(-1, 1, M))) @ dX @ np.diag(np.exp(rng.uniform(-1, 1, N)))).astype(np.float32)
    G = rng.standard_normal((M, N)).astype(np.float32)
    f = lambda a: a.astype(np.float64)
    Ql_new, Qr_new = orc.update_precond_kron(f(Ql), f(Qr), f(dX), f(dG), 0.01)
    pre = orc.precond_grad_kron(f(Ql), f(Qr), f(G))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), Ql=Ql, Qr=Qr, dX=dX, dG=dG, G=G, step=0.01,
                        Ql_new=Ql_new, Qr_new=Qr_new, pre_grad=pre)


def splu_case(name, N, r, seed, step, demo_init=False):
    p = make_splu_problem(N, r, seed=seed, init_like_demo=demo_init)
    q = {k: v.astype(np.float64) for k, v in p.items()}
    pre = orc.precond_grad_splu(q["L12"], q["l3"], q["U12"], q["u3"], [q["g"]])[0]
    new = orc.update_precond_splu(q["L12"], q["l3"], q["U12"], q["u3"], [q["dx"]], [q["dg"]], step)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **p, step=step, pre_grad=pre, L12_new=new[0], l3_new=new[1],
                        U12_new=new[2], u3_new=new[3])


def _sparse_factor(shape, n, scale):
    """Initial factors as demo_usage_of_all_preconditioners.py:68-78 builds them."""
    if shape[0] == shape[1]:
        return scale * np.eye(n)                                   # dense
    if shape[0] == 2:
        return scale * np.stack([np.ones(n), np.zeros(n)], 0)      # normalization: [diagonal; last column]
    return scale * np.ones((1, n))                                 # scaling


def kron_sparse_case(name, shape_l, shape_r, scale_l, seed, bias=None):
    """The six sparse dispatch formats (psgd.py:198-391) at the shapes of demo_usage_of_all_preconditioners.py:68-78
    (R = 5; I, J, K = 10, 20, 50).  Factors: the demo's initial ones advanced by two oracle updates so that the
    normalization factor's last column and the dense factor's upper triangle are populated.
    bias (kron_bias_*): the value of ql[1, -1], the entry of the normalization factor that the docstrings of psgd.py:205 / :335
    leave out of Ql but that :219 / :232 / :241 (and :350 / :355 / :364) read and write like any other; the updates above
    leave it at 0, so the existing kron_fmt_* cases never see it."""
    M, N = shape_l[1], shape_r[1]
    assert orc.kron_format(shape_l, shape_r) == name.split("_", 2)[2].rsplit("_", 1)[0]
    rng = np.random.default_rng(seed)
    Ql, Qr = _sparse_factor(shape_l, M, scale_l), _sparse_factor(shape_r, N, 1.0)
    for _ in range(2):
        x = rng.standard_normal((M, N))
        Ql, Qr = orc.update_precond_kron(Ql, Qr, x, x * np.exp(rng.uniform(-1, 1, (M, 1))) * np.exp(rng.uniform(-1, 1, (1, N))), 0.1)
    if bias is not None:
        for q in (Ql, Qr):
            if q.shape[0] == 2 and q.shape[1] != 2:
                q[1, -1] = bias
    Ql, Qr = Ql.astype(np.float32), Qr.astype(np.float32)
    dX = rng.standard_normal((M, N)).astype(np.float32)
    dG = (np.diag(np.exp(rng.uniform(-1, 1, M))) @ dX @ np.diag(np.exp(rng.uniform(-1, 1, N)))).astype(np.float32)
    G = rng.standard_normal((M, N)).astype(np.float32)
    f = lambda a: a.astype(np.float64)
    Ql_new, Qr_new = orc.update_precond_kron(f(Ql), f(Qr), f(dX), f(dG), 0.1)     # step of the demo (:91)
    pre = orc.precond_grad_kron(f(Ql), f(Qr), f(G))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), Ql=Ql, Qr=Qr, dX=dX, dG=dG, G=G, step=0.1,
                        Ql_new=Ql_new, Qr_new=Qr_new, pre_grad=pre)


UVD_STEP_SHAPES = [(2, 30), (30, 30), (30,), (30, 1), (1,)]        # rnn_xor_UVd_preconditioner.py:28-31 -> 1021 parameters


def uvd_step_loss_terms(p, c, b, e):
    """The closure of the UVd.step fixture: loss = sum(c p^2 / 2 + b p + e p^4 / 4) over all parameters, so that
    grad = c p + b + e p^3 and H v = (c + 3 e p^2) v are known in closed form (inputs = explicit v, grads, Hv)."""
    loss = np.sum(0.5 * c * p * p + b * p + 0.25 * e * p ** 4)
    return loss, c * p + b + e * p ** 3, c + 3.0 * e * p * p


def uvd_step_case(name, seed, balance, update_U, max_norm):
    """One exact-Hv UVd.step (psgd.py:692-764) on the 1021-parameter layout: inputs are the parameters, the loss
    coefficients, the probe vector the step 'draws', the preconditioner state and the branch decisions."""
    rng = np.random.default_rng(seed)
    N, r = 1021, 10
    q = make_uvd_problem(N, r, seed=seed, uv_gain=2.0, d_spread=0.3)
    p = (0.3 * rng.standard_normal(N)).astype(np.float32)
    c = np.exp(rng.uniform(-2, 2, N)).astype(np.float32)
    b = (0.5 * rng.standard_normal(N)).astype(np.float32)
    e = np.exp(rng.uniform(-1, 1, N)).astype(np.float32)
    vs = rng.standard_normal(N).astype(np.float32)
    f = lambda a: a.astype(np.float64)
    loss, grad, hdiag = uvd_step_loss_terms(f(p), f(c), f(b), f(e))
    U, V, d = f(q["U"]), f(q["V"]), f(q["d"])
    unfl = lambda x: orc.uvd_unflatten(x, UVD_STEP_SHAPES)
    new = orc.uvd_step(unfl(f(p)), unfl(grad), unfl(hdiag * f(vs)), unfl(f(vs)), U, V, d, 0.05, 0.02, max_norm, TINY32,
                       balance=balance, update_U=update_U)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), p=p, c=c, b=b, e=e, vs=vs, U=q["U"], V=q["V"], d=q["d"],
                        rank=r, lr_params=0.05, lr_preconditioner=0.02, grad_clip_max_norm=max_norm, tiny=TINY32,
                        balance=balance, update_U=update_U, loss=loss, grad=grad, Hv=hdiag * f(vs),
                        p_new=orc.uvd_flatten(new, np.float64), U_new=U, V_new=V, d_new=d)


def uvd_fd_grad(p, c, b, e):
    """The gradient of the closure above as reverse-mode differentiation of 0.5*c*p*p + b*p + 0.25*e*p*p*p*p forms it (torch
    autograd on the CPU, in the dtype of the inputs): the finite-difference branch subtracts two such gradients, which
    amplifies their last-bit differences by 1 / sqrt(eps), so the fixture's maker and its tests evaluate the closure the way
    an optimizer does instead of the closed form c p + b + e p^3."""
    import torch
    pt = torch.from_numpy(np.ascontiguousarray(p)).requires_grad_(True)
    c, b, e = (torch.from_numpy(np.ascontiguousarray(x)) for x in (c, b, e))
    loss = torch.sum(0.5 * c * pt * pt + b * pt + 0.25 * e * pt * pt * pt * pt)
    return loss.item(), torch.autograd.grad(loss, pt)[0].numpy()


def uvd_fd_step(z, dt):
    """One finite-difference UVd.step (psgd.py:715-727, :734-736, :760-762) of the oracle on the inputs of an uvdfd_* fixture in
    dtype dt: returns (loss, p_new, U_new, V_new, d_new).  The probe vector is delta * vs with delta = sqrt(eps(dt)) (:683, :721)."""
    f = lambda k: z[k].astype(dt)
    p, c, b, e = f("p"), f("c"), f("b"), f("e")
    delta = orc.delta_param_scale_of(dt)
    v = f("vs") * delta                                                # :721 stddev * N(0, 1)
    loss, grad = uvd_fd_grad(p, c, b, e)                               # :717-720
    p_pert = p + v                                                     # :722
    _, grad_pert = uvd_fd_grad(p_pert, c, b, e)                        # :723-726
    hv = grad_pert - grad                                              # :727
    U, V, d = f("U"), f("V"), f("d")
    unfl = lambda x: orc.uvd_unflatten(x, UVD_STEP_SHAPES)
    new = orc.uvd_step(unfl(p_pert), unfl(grad), unfl(hv), unfl(v), U, V, d, float(z["lr_params"]), float(z["lr_preconditioner"]),
                       float(z["grad_clip_max_norm"]), float(z["tiny"]), balance=bool(z["balance"]), update_U=bool(z["update_U"]),
                       exact=False, delta_param_scale=delta)
    return loss, orc.uvd_flatten(new, dt), U, V, d


def uvd_fd_step_case(name, seed, balance, update_U, max_norm):
    """One UVd.step with exact_hessian_vector_product=False on the 1021-parameter layout.  Inputs as uvd_step_case; `vs` is the
    UNIT normal draw that the step scales by sqrt(eps) of its dtype.  A smaller gradient than in the exact cases (p, b ~ 0.1)
    keeps the rounding of the difference of two gradients, eps |g| / (delta |H v|), small in fp32."""
    rng = np.random.default_rng(seed)
    N, r = 1021, 10
    q = make_uvd_problem(N, r, seed=seed, uv_gain=2.0, d_spread=0.3)
    p = (0.1 * rng.standard_normal(N)).astype(np.float32)
    c = np.exp(rng.uniform(-1, 1, N)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    e = np.exp(rng.uniform(-1, 1, N)).astype(np.float32)
    vs = rng.standard_normal(N).astype(np.float32)
    inputs = dict(p=p, c=c, b=b, e=e, vs=vs, U=q["U"], V=q["V"], d=q["d"], rank=r, lr_params=0.05, lr_preconditioner=0.01,
                  grad_clip_max_norm=max_norm, tiny=TINY32, balance=balance, update_U=update_U)
    z = {k: np.asarray(v) for k, v in inputs.items()}
    loss, p_new, U, V, d = uvd_fd_step(z, np.float64)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **inputs, loss=loss, p_new=p_new, U_new=U, V_new=V, d_new=d)


def dense_case(name, N, shapes, seed, step):
    """update_precond_dense / precond_grad_dense (psgd.py:26-63) on lists of mixed-shape tensors that add up to N entries:
    Q upper triangular with cond ~ 30, dg = c .* dx with c ~ LogUniform[1/e, e].  dx_i, dg_i, g_i are the list entries."""
    assert sum(int(np.prod(s)) for s in shapes) == N
    rng = np.random.default_rng(seed)
    Q = illcond_factor(rng, N, cond=30.0).astype(np.float32)
    dxs = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    dgs = [(np.exp(rng.uniform(-1, 1, s)) * x).astype(np.float32) for s, x in zip(shapes, dxs)]
    gs = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    f = lambda xs: [x.astype(np.float64) for x in xs]
    Q_new = orc.update_precond_dense(Q.astype(np.float64), f(dxs), f(dgs), step)
    pre = orc.precond_grad_dense(Q.astype(np.float64), f(gs))
    lists = {"%s_%d" % (k, i): x for k, xs in (("dx", dxs), ("dg", dgs), ("g", gs)) for i, x in enumerate(xs)}
    np.savez_compressed(os.path.join(HERE, name + ".npz"), Q=Q, **lists, n_tensors=len(shapes), step=step, Q_new=Q_new,
                        pre_grad=np.concatenate([np.reshape(x, -1) for x in pre]))


if __name__ == "__main__":
    uvd_case("uvd_n1021_r10_updU", 1021, 10, 1, 2.0, 0.3, False, True)     # rnn_xor model size (KAT-IDX)
    uvd_case("uvd_n1021_r10_updV_bal", 1021, 10, 2, 2.0, 0.3, True, False)
    uvd_case("uvd_n4096_r20_updU", 4096, 20, 3, 1.0, 0.0, False, True)     # reference init scales (psgd.py:687-690)
    uvd_case("uvd_n777_r1_updV", 777, 1, 4, 2.0, 0.2, False, False)
    kron_case("kron_lenet_w2_151x16", 151, 16, 5)                           # mnist_with_lenet5.py:13
    kron_case("kron_lenet_w5_85x10", 85, 10, 6)                             # mnist_with_lenet5.py:16
    kron_case("kron_wide_16x40", 16, 40, 7)                                 # M < N branch (psgd.py:189-190)
    kron_case("kron_1x1_3x3", 1, 3, 8)                                      # 1x1 dense factor (NMT demo :124)
    # sparse dispatch formats, demo_usage_of_all_preconditioners.py:68-70 (example 1) and :73-75 (example 2); R = 5
    kron_sparse_case("kron_fmt_dense_norm_5x10", (5, 5), (2, 10), 0.1, 21)
    kron_sparse_case("kron_fmt_scale_dense_5x20", (1, 5), (20, 20), 0.1, 22)
    kron_sparse_case("kron_fmt_scale_norm_5x50", (1, 5), (2, 50), 0.1, 23)
    kron_sparse_case("kron_fmt_norm_dense_5x10", (2, 5), (10, 10), 0.1, 24)
    kron_sparse_case("kron_fmt_dense_scale_5x20", (5, 5), (1, 20), 0.1, 25)
    kron_sparse_case("kron_fmt_norm_scale_5x50", (2, 5), (1, 50), 0.1, 26)
    uvd_step_case("uvdstep_n1021_r10_updU_clip", 31, False, True, 1.0)       # rnn_xor_UVd_preconditioner.py:33-36 (clip 1.0)
    uvd_step_case("uvdstep_n1021_r10_updV_bal_noclip", 32, True, False, np.inf)
    splu_case("splu_n400_r10_demo_init", 400, 10, 9, 0.1, demo_init=True)   # demo_usage_of_all_preconditioners.py:45-51,61
    splu_case("splu_n1021_r7", 1021, 7, 10, 0.01)                           # odd rank (alignment head path)
    splu_case("splu_n2048_r20", 2048, 20, 11, 0.1)
    # ---- shapes that reach the routes built since round 1 (inputs: the same makers; tests/golden/tf/ holds the reference's outputs)
    dense_case("dense_n5", 5, [(2, 2), (1,)], 41, 0.1)                       # no dense fixture before; a scalar-sized tail entry
    dense_case("dense_n67", 67, [(3, 7), (5,), (40, 1), ()], 42, 0.01)       # crosses the 64 / 65 route switch, partial 64-row block
    uvd_case("uvd_n300_r40_updU_bal", 300, 40, 43, 2.0, 0.3, True, True)     # ranks 33 .. 64: the whole-matrix wide kernels
    uvd_case("uvd_n300_r40_updV", 300, 40, 44, 2.0, 0.3, False, False)
    uvd_case("uvd_n7_r10_updU", 7, 10, 45, 0.5, 0.3, False, True)            # fewer rows than the rank
    uvd_case("uvd_n515_r33_updV_g3", 515, 33, 46, 2.0, 0.3, False, False, g_cols=3)   # a partial 64-row tile, matrix g
    uvd_case("uvd_n1021_r10_updU_g5", 1021, 10, 47, 2.0, 0.3, False, True, g_cols=5)  # g [N, 5]: a group of four columns + one
    splu_case("splu_n273_r41", 273, 41, 48, 0.01)                            # the rank of the round-5 lane-index bug, partial last tile
    splu_case("splu_n12_r12", 12, 12, 49, 0.1)                               # no tail
    splu_case("splu_n65_r64", 65, 64, 50, 0.01)                              # one-row tail at the widest native rank
    splu_case("splu_n140_r70", 140, 70, 51, 0.1)                             # column chunks above rank 64
    kron_case("kron_odd_33x129", 33, 129, 52)                                # both sides of the M < N association branch (psgd.py:189),
    kron_case("kron_odd_129x33", 129, 33, 53)                                # odd sizes that leave partial tiles
    kron_sparse_case("kron_bias_dense_norm_5x10", (5, 5), (2, 10), 0.1, 54, bias=0.37)    # ql[1, -1] != 0 (psgd.py:237 / :360)
    kron_sparse_case("kron_bias_norm_dense_5x10", (2, 5), (10, 10), 0.1, 55, bias=-0.21)
    kron_sparse_case("kron_bias_scale_norm_5x50", (1, 5), (2, 50), 0.1, 56, bias=0.29)
    kron_sparse_case("kron_bias_norm_scale_5x50", (2, 5), (1, 50), 0.1, 57, bias=-0.33)
    uvd_fd_step_case("uvdfd_n1021_r10_updU_clip", 58, False, True, 1.0)      # the finite-difference branch (psgd.py:715-727)
    print(sorted(f for f in os.listdir(HERE) if f.endswith(".npz")))
