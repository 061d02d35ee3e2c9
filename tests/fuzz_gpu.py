"""Randomised parity sweep on the GPU: many random shapes per entry-point family against independent fp64 torch
restatements (oracle/psgd_oracle_torch.py and local block formulas).  TEST INFRASTRUCTURE (it imports oracle/).
tests/test_fuzz_gpu.py runs the six-family rotation of run() for a few seconds; tests/test_fuzz_families_gpu.py runs a fixed
number of cases of the other families through run_cases(); longer sweeps over all of them: python tests/fuzz_gpu.py [seconds]"""
import hashlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_stochastic_gradient_descent as psgd  # noqa: E402
from oracle import psgd_oracle_torch as ref64  # noqa: E402
from psgd_tf_amd import _lib  # noqa: E402

TINY = 1.1754943508222875e-38
dev = torch.device("cuda:0")


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    d = torch.linalg.vector_norm(b)
    return float(torch.linalg.vector_norm(a - b) / (d if d > 0 else 1.0))


def tri(n, g, off):
    return torch.triu(torch.randn(n, n, device=dev, generator=g) * off, 1) + torch.diag(torch.exp(0.3 * torch.randn(n, device=dev, generator=g)))


def randint(lo, hi, g):
    return int(torch.randint(lo, hi, (1,), generator=g, device=dev))


def long_side_shape(g, it, mult=1):
    """Rarely, a layer with one long side ([2048, 8200] x [64, 1100], either way round: the inverse tiers, the 8192 cap, the
    rectangular gradient split) or, more rarely still, both sides in [3000, 6200] (the inverse route with the products first);
    else None.  Sides rounded down to `mult`."""
    if it % 61 == 40:
        M, N = randint(3000, 6201, g), randint(3000, 6201, g)
    elif it % 23 == 11:
        M, N = randint(2048, 8201, g), randint(64, 1101, g)
        if it % 2:
            M, N = N, M
    else:
        return None
    return M // mult * mult, N // mult * mult


LARGE_KRON = [0]      # Kron cases with a side >= 4096 (reported by the command line)


def fuzz_kron(g, it):
    big = it % 7 == 0
    M = int(torch.randint(1, 2600 if big else 700, (1,), generator=g, device=dev))
    N = int(torch.randint(1, 2600 if big else 700, (1,), generator=g, device=dev))
    if it % 28 == 27 or (os.environ.get("FUZZ_BIG") == "1" and it % 3 == 2):   # both factors from 2048 on: the solves through explicit inverses
        M = int(torch.randint(2048, 3000, (1,), generator=g, device=dev))
        N = int(torch.randint(2049, 3000, (1,), generator=g, device=dev))
    M, N = long_side_shape(g, it) or (M, N)
    LARGE_KRON[0] += max(M, N) >= 4096
    off = 0.5 / max(M, N) ** 0.5
    Ql, Qr = tri(M, g, off) * 1.7, tri(N, g, off)
    dX = torch.randn(M, N, device=dev, generator=g)
    dG = torch.exp(torch.empty(M, 1, device=dev).uniform_(-1, 1, generator=g)) * dX * torch.exp(torch.empty(1, N, device=dev).uniform_(-1, 1, generator=g))
    G = torch.randn(M, N, device=dev, generator=g)
    if it % 3 == 0:                                   # data of any magnitude (the plane formats carry their own scales)
        s = 10.0 ** float(torch.empty(1, device=dev).uniform_(-12, 12, generator=g))
        G, dX, dG = G * s, dX * s, dG / s
    e1 = rel(psgd.precond_grad_kron(Ql, Qr, G), ref64.precond_grad_dense_dense(Ql.double(), Qr.double(), G.double()))
    a, b = psgd.update_precond_kron(Ql, Qr, dX, dG, 0.01)
    a64, b64 = ref64.update_precond_dense_dense(Ql.double(), Qr.double(), dX.double(), dG.double(), 0.01, TINY)
    e2 = max(rel(a, a64), rel(b, b64))
    return "kron %dx%d" % (M, N), max(e1, e2), 1e-5


def fuzz_kron_bf16(g, it):
    M = 8 * int(torch.randint(1, 330, (1,), generator=g, device=dev))
    N = 8 * int(torch.randint(1, 330, (1,), generator=g, device=dev))
    if it % 3 == 1:                                   # not multiples of 8: the zero-padded path
        M, N = M - int(torch.randint(0, 8, (1,), generator=g, device=dev)), N - int(torch.randint(0, 8, (1,), generator=g, device=dev))
        M, N = max(M, 1), max(N, 1)
    if it % 5 == 0:
        M, N = 256 * int(torch.randint(4, 17, (1,), generator=g, device=dev)), 256 * int(torch.randint(4, 17, (1,), generator=g, device=dev))
    off = 0.5 / max(M, N) ** 0.5
    Ql, Qr = tri(M, g, off), tri(N, g, off)
    G = torch.randn(M, N, device=dev, generator=g).to(torch.bfloat16)
    out = psgd.precond_grad_kron(Ql, Qr, G)
    return "kron-bf16 %dx%d" % (M, N), rel(out, ref64.precond_grad_dense_dense(Ql.double(), Qr.double(), G.double())), 2e-2


def fuzz_kron_bf16_update(g, it):
    M = 8 * int(torch.randint(1, 200, (1,), generator=g, device=dev))
    N = 8 * int(torch.randint(1, 200, (1,), generator=g, device=dev))
    if it % 6 == 0:
        M, N = 64 * int(torch.randint(8, 40, (1,), generator=g, device=dev)), 64 * int(torch.randint(8, 40, (1,), generator=g, device=dev))
    if it % 30 == 29:                                 # the fp32 solves through explicit inverses
        M, N = 64 * int(torch.randint(32, 44, (1,), generator=g, device=dev)), 64 * int(torch.randint(33, 44, (1,), generator=g, device=dev))
    sk = 0
    if it % 4 == 1:                                   # the gradient products as stream-K launches on shapes their default rule skips
        M = 256 * int(torch.randint(1, 10, (1,), generator=g, device=dev))
        N = M if it % 8 == 1 else 256 * int(torch.randint(1, 10, (1,), generator=g, device=dev))
        sk = 2 + (it // 4) % 2                        # 2: whole-tile rounds + ranges, 3: ranges only
    big = long_side_shape(g, it, 8)
    if big:
        M, N, sk = big[0], big[1], 0
        LARGE_KRON[0] += max(M, N) >= 4096
    off = 0.5 / max(M, N) ** 0.5
    Ql, Qr = tri(M, g, off) * 1.7, tri(N, g, off)
    dX = torch.randn(M, N, device=dev, generator=g)
    dG = torch.exp(torch.empty(M, 1, device=dev).uniform_(-1, 1, generator=g)) * dX * torch.exp(torch.empty(1, N, device=dev).uniform_(-1, 1, generator=g))
    dX, dG = dX.to(torch.bfloat16), dG.to(torch.bfloat16)
    if sk:
        _lib.load().psgd_kron_bf16_set_tuning(4, sk)
    try:
        a, b = psgd.update_precond_kron(Ql, Qr, dX, dG, 0.01)
    finally:
        if sk:
            _lib.load().psgd_kron_bf16_set_tuning(4, 1)
    a64, b64 = ref64.update_precond_dense_dense(Ql.double(), Qr.double(), dX.double(), dG.double(), 0.01, TINY)
    # the stated bf16 bar (2e-2) applies to the increment the bf16 GEMMs produce; on the factors it is step (0.01) times that
    rho = (torch.diagonal(Ql).max() / torch.diagonal(Qr).max()).double().sqrt()
    e_inc = max(rel(a.double() - Ql.double() / rho, a64 - Ql.double() / rho), rel(b.double() - Qr.double() * rho, b64 - Qr.double() * rho))
    e_fac = max(rel(a, a64), rel(b, b64))
    return "kron-bf16-upd %dx%d%s" % (M, N, " sk%d" % sk if sk else ""), max(e_inc, 100.0 * e_fac), 2e-2


_SPARSE_KINDS = (("dense", "norm"), ("dense", "scale"), ("norm", "dense"), ("norm", "scale"), ("scale", "dense"), ("scale", "norm"))


def fuzz_kron_sparse(g, it):
    """The six sparse dispatch formats (psgd.py:80-152) on random shapes, incl. embedding-like ones (a long non-dense side:
    row-blocked column reductions, split-K gradient), against the numpy fp64 oracle."""
    import numpy as np
    from oracle import psgd_oracle as orc
    kl, kr = _SPARSE_KINDS[int(torch.randint(0, 6, (1,), generator=g, device=dev))]
    long_side = it % 3 == 0

    def dim(kind):
        hi = 700 if kind == "dense" else (9000 if long_side else 400)
        return int(torch.randint(3, hi, (1,), generator=g, device=dev))       # (below 3 the shapes of the three kinds coincide)
    M, N = dim(kl), dim(kr)

    def fac(kind, n):
        if kind == "dense":
            return tri(n, g, 0.5 / n ** 0.5) * 1.3
        if kind == "norm":
            q = torch.stack([torch.exp(0.2 * torch.randn(n, device=dev, generator=g)), 0.1 * torch.randn(n, device=dev, generator=g)])
            q[1, -1] = 0.0
            return q
        return torch.exp(0.2 * torch.randn(1, n, device=dev, generator=g))
    Ql, Qr = fac(kl, M), fac(kr, N)
    dX = torch.randn(M, N, device=dev, generator=g)
    dG = torch.exp(torch.empty(M, 1, device=dev).uniform_(-1, 1, generator=g)) * dX * torch.exp(torch.empty(1, N, device=dev).uniform_(-1, 1, generator=g))
    G = torch.randn(M, N, device=dev, generator=g)
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    out = psgd.precond_grad_kron(Ql, Qr, G)
    e1 = rel(out, torch.from_numpy(orc.precond_grad_kron(n64(Ql), n64(Qr), n64(G))).to(dev))
    a, b = psgd.update_precond_kron(Ql, Qr, dX, dG, 0.01)
    a64, b64 = orc.update_precond_kron(n64(Ql), n64(Qr), n64(dX), n64(dG), 0.01)
    e2 = max(rel(a, torch.from_numpy(a64).to(dev)), rel(b, torch.from_numpy(b64).to(dev)))
    return "kron-sparse %s(x)%s %dx%d" % (kl, kr, M, N), max(e1, e2), 3e-5


GRAM_KINDS = ("cyclic", "reversal", "smallpivot", "cond1e2")      # the kinds of tests/uvd_cases.py that keep the hard bars


def gram_problem(N, r, it):
    """Every fifth UVd case (it % 5 == 2) of rank 2 and above: a problem whose K = I + V'U forces row exchanges in the r x r solves or
    is ill-conditioned (tests/uvd_cases.py: make_uvd_problem_with_gram), the kind in rotation.  Rank 1 stays with its usual problem: K
    is a scalar there, there is no row to exchange, and `smallpivot` (K = 1e-6) costs the fp32 NumPy oracle itself 1.4e-5, more than
    the hard bar.  Seeded from (it, N, r): the family's generator has made its usual draws before, so the cases around it stay what
    they were.  fuzz_uvd draws its ranks above 32 at it % 15 == 3, never a multiple of 5 plus 2: outside FUZZ_ONLY=wide the chosen
    Grams stay at ranks 2 .. 32; the ranks above have them in tests/test_uvd_gram_conditioning_gpu.py.
    Returns (kind, (U, V, d, g, v, h))."""
    import numpy as np
    from tests.uvd_cases import gram_kinds, make_uvd_problem_with_gram
    kind = GRAM_KINDS[(it // 5) % len(GRAM_KINDS)]
    seed = 7919 * it + 31 * r + N
    p = make_uvd_problem_with_gram(N, r, gram_kinds(r, np.random.default_rng(seed))[kind], seed + 1)
    return kind, tuple(torch.from_numpy(p[k]).to(dev) for k in ("U", "V", "d", "g", "v", "h"))


_WIDE_ONLY = os.environ.get("FUZZ_ONLY") == "wide"     # only ranks 33 .. 64 of the two low-rank preconditioners (round 5's kernels)


def fuzz_uvd(g, it):
    r = int(torch.randint(1, 33, (1,), generator=g, device=dev))
    if it % 15 == 3:                                  # wide rank: whole-matrix kernels to 64, column chunks above (uvd_wide.py)
        r = int(torch.randint(33, 80, (1,), generator=g, device=dev))
    if _WIDE_ONLY:
        r = int(torch.randint(33, 65, (1,), generator=g, device=dev))
    N = int(torch.randint(max(r, 2), 400000 if it % 4 == 0 else 20000, (1,), generator=g, device=dev))
    # from the reference's init scale (gain 2) to ||U V'|| = O(1) (gain ~ sqrt(r)), V correlated with U every third case
    gain = 2.0 if it % 3 else float(torch.empty(1, device=dev).uniform_(0.5, 1.5, generator=g)) * r ** 0.5
    sc = gain * (1.0 / (N * r)) ** 0.5
    U, V = torch.randn(N, r, device=dev, generator=g) * sc, torch.randn(N, r, device=dev, generator=g) * sc
    if it % 3 == 0 and N > 4 * r:
        V = (0.5 * U @ torch.linalg.qr(torch.randn(r, r, device=dev, generator=g))[0] + 0.7 * V).contiguous()
    d = torch.exp(0.3 * torch.randn(N, 1, device=dev, generator=g))
    gr, v = torch.randn(N, 1, device=dev, generator=g), torch.randn(N, 1, device=dev, generator=g)
    h = v * torch.exp(torch.empty(N, 1, device=dev).uniform_(-4.6, 4.6, generator=g))
    kind = ""
    if it % 5 == 2 and r > 1:
        kind, (U, V, d, gr, v, h) = gram_problem(N, r, it)
    U64, V64, d64 = U.double(), V.double(), d.double()
    U0, V0, d0 = U.clone(), V.clone(), d.clone()
    upd = bool(it % 2)
    bal = it % 5 == 0
    out = psgd.update_precond_UVd_math_and_precond_grad(U, V, d, v, h, gr, 0.01, TINY, balance=bal, update_U=upd)
    ref64.update_precond_UVd_math_(U64, V64, d64, v.double(), h.double(), 0.01, TINY, balance=bal, update_U=upd)
    e = max(rel(out, ref64.precond_grad_UVd_math(U64, V64, d64, gr.double())), rel(U, U64), rel(V, V64), rel(d, d64))
    if it % 2 == 0:                                   # the two reference-named calls and IpUVtmatvec on a matrix
        psgd.update_precond_UVd_math_(U, V, d, v, h, 0.01, TINY, balance=False, update_U=not upd)
        ref64.update_precond_UVd_math_(U64, V64, d64, v.double(), h.double(), 0.01, TINY, balance=False, update_U=not upd)
        e = max(e, rel(psgd.precond_grad_UVd_math(U, V, d, gr), ref64.precond_grad_UVd_math(U64, V64, d64, gr.double())),
                rel(U, U64), rel(V, V64), rel(d, d64))
        X = torch.cat([gr, v, d], 1).contiguous()
        e = max(e, rel(psgd.IpUVtmatvec(U, V, X), ref64.IpUVtmatvec(U.double(), V.double(), X.double())))
        # precond_grad_UVd_math on a matrix g (three columns): psgd_uvd_apply_cols_f32 up to rank 32, the column chunks above
        e = max(e, rel(psgd.precond_grad_UVd_math(U, V, d, X), ref64.precond_grad_UVd_math(U64, V64, d64, X.double())))
    tol = 2e-5 if r > 32 else 1e-5
    if not e < tol and not kind:                      # (the gram cases keep the hard bars)
        # Before calling it a failure: how far does the fp64 update itself move when its fp32 inputs are perturbed by
        # 1e-7 (relative, every element)?  The HIP path rounds intermediates such as t = d .* h to fp32, as the reference
        # does; on the rare input where the map amplifies that (seen at r = 1: 16-19 x against 1-4 x normally,
        # tools/uvd_r1_probe.py) the distance to the all-fp64 result is that amplification, not a defect.
        sens = 0.0
        for _ in range(4):
            pert = lambda x: x.double() * (1 + 1e-7 * torch.randn(x.shape, device=dev, dtype=torch.float64))
            Up, Vp, dp = pert(U0), pert(V0), pert(d0)
            Ur, Vr, dr = U0.double(), V0.double(), d0.double()
            ref64.update_precond_UVd_math_(Up, Vp, dp, pert(v), pert(h), 0.01, TINY, balance=bal, update_U=upd)
            ref64.update_precond_UVd_math_(Ur, Vr, dr, v.double(), h.double(), 0.01, TINY, balance=bal, update_U=upd)
            sens = max(sens, max(rel(Up, Ur), rel(Vp, Vr), rel(dp, dr)) / 1e-7)
        tol = max(tol, 5e-7 * sens)
        print("uvd N=%d r=%d: err %.2e, the fp64 update moves %.0f x a 1e-7 input perturbation -> bar %.1e" % (N, r, e, sens, tol),
              flush=True)
    return "uvd N=%d r=%d%s" % (N, r, " gram-" + kind if kind else ""), e, tol


def splu_apply64(L12, l3, U12, u3, x, r):
    L1, L2, U1, U2 = L12[:r], L12[r:], U12[:, :r], U12[:, r:]
    Ug1 = U1 @ x[:r] + U2 @ x[r:]
    Qg1 = L1 @ Ug1
    Qg2 = L2 @ Ug1 + l3 * (u3 * x[r:])
    Lt1 = L1.t() @ Qg1 + L2.t() @ Qg2
    return torch.cat([U1.t() @ Lt1, U2.t() @ Lt1 + u3 * (l3 * Qg2)], 0)


def _rel_np(a, b):
    import numpy as np
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


def fuzz_splu(g, it):
    r = int(torch.randint(1, 33, (1,), generator=g, device=dev))
    if it % 5 == 2:                                   # ranks 33 .. 64: the native kernels on 64-row tiles (round 5); above: column chunks
        r = int(torch.randint(33, 72, (1,), generator=g, device=dev))
    if _WIDE_ONLY:
        r = int(torch.randint(33, 65, (1,), generator=g, device=dev))
    N = int(torch.randint(r, 300000 if it % 4 == 0 else 20000, (1,), generator=g, device=dev))
    sc = 0.3 / r ** 0.5
    L12 = torch.randn(N, r, device=dev, generator=g) * (sc * 3 * (r / N) ** 0.5)
    U12 = torch.randn(r, N, device=dev, generator=g) * (sc * 3 * (r / N) ** 0.5)
    L12[:r] = torch.tril(torch.randn(r, r, device=dev, generator=g) * sc, -1) + torch.eye(r, device=dev)
    U12[:, :r] = torch.triu(torch.randn(r, r, device=dev, generator=g) * sc, 1) + torch.eye(r, device=dev)
    l3 = torch.exp(torch.empty(N - r, 1, device=dev).uniform_(-0.5, 0.5, generator=g))
    u3 = torch.exp(torch.empty(N - r, 1, device=dev).uniform_(-0.5, 0.5, generator=g)) * 0.7
    x = torch.randn(N, 1, device=dev, generator=g)
    dg = x * torch.exp(torch.empty(N, 1, device=dev).uniform_(-2, 2, generator=g))
    gr = torch.randn(N, 1, device=dev, generator=g)
    e1 = rel(psgd.precond_grad_splu(L12, l3, U12, u3, [gr])[0], splu_apply64(L12.double(), l3.double(), U12.double(), u3.double(), gr.double(), r))
    new = psgd.update_precond_splu(L12, l3, U12, u3, [x], [dg], 0.05)
    # the updated factors must still give a symmetric positive P consistent with their own fp64 apply
    e2 = rel(psgd.precond_grad_splu(*new, [gr])[0], splu_apply64(*[t.double() for t in new], gr.double(), r))
    # the four factors against the numpy fp64 oracle, bars of tests/test_splu_gpu.py: 1e-5 on each non-empty factor, 2e-3 on its
    # increment over the rho-balanced base (reported on the 1e-5 scale), exact zeros in the strict triangles of L1 / U1
    import numpy as np
    from oracle import psgd_oracle as orc
    n64 = lambda t: t.cpu().numpy().astype(np.float64)
    q = [n64(t) for t in (L12, l3, U12, u3)]
    ref = orc.update_precond_splu(*q, [n64(x)], [n64(dg)], 0.05)
    rho = np.sqrt(max(np.max(np.diag(q[0][:r])), np.max(q[1], initial=-np.inf)) /
                  max(np.max(np.diag(q[2][:, :r])), np.max(q[3], initial=-np.inf)))
    base = (q[0] / rho, q[1] / rho, q[2] * rho, q[3] * rho)
    e3 = e4 = 0.0
    for got, want, b0 in zip(new, ref, base):
        if want.size == 0:
            continue
        got = n64(got)
        e3 = max(e3, _rel_np(got, want))
        e4 = max(e4, _rel_np(got - b0, want - b0))
    if bool(torch.triu(new[0][:r], 1).any()) or bool(torch.tril(new[2][:, :r], -1).any()):
        print("splu N=%d r=%d: a strict triangle of L1 / U1 is not zero" % (N, r), flush=True)
        e3 = float("inf")
    return "splu N=%d r=%d" % (N, r), max(e1, e2, e3, e4 * (1e-5 / 2e-3)), 1e-5


# ------------------------------------------------------------------------------------------------ dense (psgd_dense.hip)
_DENSE_EDGES = (("edge64", 64, 47), ("edge256", 256, 12), ("edge1024", 1024, 3), ("route64", 64, 2))   # class, multiple, k < this


def _split_list(flat, g):
    """flat [N] as a list of 1 .. 4 tensors of random shapes (the list arguments of psgd.py:34-35 / :48-53)"""
    n = flat.numel()
    k = min(randint(1, 5, g), n)
    cuts = sorted(set([0, n] + [randint(1, n, g) for _ in range(k - 1)])) if n > 1 else [0, n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m, kind = hi - lo, randint(0, 4, g)
        p = [q for q in (2, 3, 4, 5) if m % q == 0]
        shape = ((m,), (m, 1), (1, m), (p[0], m // p[0]) if p else (m,))[kind]
        parts.append(flat[lo:hi].reshape(shape).clone())
    return parts


def dense_update64(Q, dx, dg, step):
    """psgd.py:34-42 in fp64 torch ops (G formed, O(N^3)); the solve reads the upper triangle of Q only, as the reference's does"""
    a = Q @ dg
    b = torch.linalg.solve_triangular(Q.t(), dx, upper=False)
    grad = torch.triu(a @ a.t() - b @ b.t())
    return Q - ((step / (grad.abs().max() + TINY)) * grad) @ Q


DENSE_RATIOS = []      # (case, err_native / err_torch on Q_new, on the increment, on the apply) of the c = 2.0 cases


def fuzz_dense(g, it):
    """update_precond_dense and precond_grad_dense on N in [1, 3000]: tile, workgroup and route edges, an upper-triangular or a full
    Q, Q at an unaligned address, list arguments, data of any magnitude; bars of tests/test_dense_gpu.py (Q_new 1e-5, its increment
    2e-3, the apply 1e-5, exact zeros below the diagonal of an upper-triangular Q).  Reported: the largest error / bar."""
    N = randint(1, 3001, g)
    tags = []
    if it % 3 == 0:                                   # on a tile / workgroup / route edge, or up to four off it
        name, mult, khi = _DENSE_EDGES[(it // 3) % 4]
        N = mult * randint(1, khi, g) + randint(-4, 5, g)
        tags.append(name)
    unaligned = it % 4 == 1
    if unaligned:                                     # N % 4 == 0 at an address that is not: update_large<1> / apply_large<1>
        N = max(4, N // 4 * 4)
        tags.append("unaligned")
    upper = it % 2 == 0
    c = (0.3, 1.0, 2.0)[randint(0, 3, g)]
    step = (0.01, 0.1)[randint(0, 2, g)]
    Q = torch.triu(torch.randn(N, N, device=dev, generator=g) * (c / N ** 0.5), 1) \
        + torch.diag(torch.exp(torch.empty(N, device=dev).uniform_(-1.6, 1.6, generator=g)))
    if not upper:
        Q = Q + torch.tril(torch.randn(N, N, device=dev, generator=g) * (0.3 / N ** 0.5), -1)
    dx, dg, gr = (torch.randn(N, device=dev, generator=g) for _ in range(3))
    if (it + it // 3) % 3 == 1:                       # one case in three, moving through the residues of the other switches
        s = 10.0 ** float(torch.empty(1, device=dev).uniform_(-12, 12, generator=g))
        dx, dg = dx * s, dg / s * torch.exp(torch.empty(N, device=dev).uniform_(-2, 2, generator=g))
        tags.append("s=%.0e" % s)
    if unaligned:
        buf = torch.zeros(N * N + 4, device=dev)
        off = randint(1, 4, g)
        Qv = buf[off:off + N * N].view(N, N)
        Qv.copy_(Q)
        Q = Qv
        if Q.data_ptr() % 16 == 0 or not Q.is_contiguous():
            raise RuntimeError("fuzz_dense: the view at offset %d is aligned" % off)
    dxs, dgs, grs = _split_list(dx, g), _split_list(dg, g), _split_list(gr, g)
    Q0 = Q.clone()
    Q64, dx64, dg64, gr64 = Q.double(), dx.double()[:, None], dg.double()[:, None], gr.double()[:, None]
    ref_q, ref_p = dense_update64(Q64, dx64, dg64, step), Q64.t() @ (Q64 @ gr64)

    def errs(route):
        psgd.set_dense_route(route)
        try:
            qn = psgd.update_precond_dense(Q, dxs, dgs, step)
            pg = psgd.precond_grad_dense(Q, grs)
        finally:
            psgd.set_dense_route("native")
        if [tuple(p.shape) for p in pg] != [tuple(t.shape) for t in grs] or qn.shape != Q.shape:
            return qn, (float("inf"),) * 3
        return qn, (rel(qn, ref_q), rel(qn.double() - Q64, ref_q - Q64), rel(torch.cat([p.reshape(-1) for p in pg]), ref_p))
    bars = (1e-5, 2e-3, 1e-5)
    qn, e_nat = errs("native")
    worst = max(e / b for e, b in zip(e_nat, bars))
    name = "dense N=%d %s c=%.1f step=%.2f%s" % (N, "upper" if upper else "full", c, step, "".join(" " + t for t in tags))
    if upper and bool(torch.tril(qn, -1).any()):
        print(name + ": the strict lower triangle is not zero", flush=True)
        worst = float("inf")
    if not torch.equal(Q, Q0):
        print(name + ": Q was modified", flush=True)
        worst = float("inf")
    if c == 2.0:
        # The least benign Q, where the blocked solve's explicit block inverses matter most: the torch-op route on the same inputs.
        # err_native <= 2 err_torch + bar is implied by the bars above (its floor IS the bar), so it cannot fail on its own: what
        # it adds is the record of err_native / err_torch in DENSE_RATIOS (profiles/fuzz_families.txt).
        _, e_tor = errs("torch")
        DENSE_RATIOS.append((name,) + tuple(n / t if t > 0 else float("inf") for n, t in zip(e_nat, e_tor)))
        worst = max([worst] + [n / (2 * t + b) for n, t, b in zip(e_nat, e_tor, bars)])
    return name + " [Q %.1e inc %.1e apply %.1e]" % e_nat, worst, 1.0


# ------------------------------------------------------------------------------------------------ bf16-state UVd (psgd_uvd_bf16.hip)
def uvd_bf16_tile_rows(r):
    """rows per tile of psgd_uvd_bf16.hip at rank r (make_geo): 256 at ranks 1 .. 8, 16 and 29 .. 32; 136 .. 240 at the others"""
    m = min(256 // r, 32)
    return 256 // (8 * m) * (8 * m)


def fuzz_uvd_bf16(g, it):
    """The apply, the update and the fused call on a bf16-stored state, inputs as in fuzz_uvd with U, V, d rounded to bf16 first, the
    fp64 oracle on the widened values; bars of tests/test_uvd_bf16_gpu.py.  Reported: the largest error / bar."""
    import numpy as np
    from tests.uvd_cases import check_bf16_state
    r = randint(1, 33, g)
    hi = 400000 if it % 4 == 0 else 20000
    N = randint(max(r, 2), hi, g)
    edge = ""
    if it % 3 == 1:                                   # a partial last tile of 1 .. 63 rows behind whole tiles of 64, 256 and the family's own
        mult = (64, 256, uvd_bf16_tile_rows(r))[(it // 3) % 3]
        N = mult * randint(1, max(2, hi // mult), g) + randint(1, 64, g)
        edge = " edge%s" % ("TR%d" % mult if (it // 3) % 3 == 2 else mult)
    gain = 2.0 if it % 3 else float(torch.empty(1, device=dev).uniform_(0.5, 1.5, generator=g)) * r ** 0.5
    sc = gain * (1.0 / (N * r)) ** 0.5
    U, V = torch.randn(N, r, device=dev, generator=g) * sc, torch.randn(N, r, device=dev, generator=g) * sc
    if it % 3 == 0 and N > 4 * r:
        V = (0.5 * U @ torch.linalg.qr(torch.randn(r, r, device=dev, generator=g))[0] + 0.7 * V).contiguous()
    d = torch.exp(0.3 * torch.randn(N, 1, device=dev, generator=g))
    gr, v = torch.randn(N, 1, device=dev, generator=g), torch.randn(N, 1, device=dev, generator=g)
    h = v * torch.exp(torch.empty(N, 1, device=dev).uniform_(-4.6, 4.6, generator=g))
    if it % 5 == 2 and r > 1:
        kind, (U, V, d, gr, v, h) = gram_problem(N, r, it)
        edge += " gram-" + kind
    upd, bal = bool(it % 2), it % 5 == 0
    rounding = "stochastic" if (it // 2) % 2 else "nearest"
    fused = (it // 4) % 2 == 0
    seed = randint(0, 2 ** 31, g)
    bf = torch.bfloat16
    Ub, Vb, db = U.to(bf), V.to(bf), d.to(bf)
    name = "uvd-bf16 N=%d r=%d %s%s %s %s%s" % (N, r, "U" if upd else "V", " bal" if bal else "", rounding,
                                               "fused" if fused else "two-call", edge)
    e_apply = rel(psgd.precond_grad_UVd_math(Ub, Vb, db, gr), ref64.precond_grad_UVd_math(Ub.double(), Vb.double(), db.double(), gr.double()))
    U64, V64, d64 = Ub.double(), Vb.double(), db.double()
    ref64.update_precond_UVd_math_(U64, V64, d64, v.double(), h.double(), 0.01, TINY, balance=bal, update_U=upd)
    Uw, Vw, dw = Ub.float(), Vb.float(), db.float()   # the yardstick of the code shares: the fp32 kernels on the widened inputs
    psgd.update_precond_UVd_math_(Uw, Vw, dw, v, h, 0.01, TINY, balance=bal, update_U=upd)
    Ut, Vt, dt = Ub.clone(), Vb.clone(), db.clone()
    kw = dict(balance=bal, update_U=upd, rounding=rounding, rounding_seed=seed)
    if fused:
        out = psgd.update_precond_UVd_math_and_precond_grad(Ut, Vt, dt, v, h, gr, 0.01, TINY, **kw)
    else:
        psgd.update_precond_UVd_math_(Ut, Vt, dt, v, h, 0.01, TINY, **kw)
        out = psgd.precond_grad_UVd_math(Ut, Vt, dt, gr)
    e_grad = rel(out, ref64.precond_grad_UVd_math(Ut.double(), Vt.double(), dt.double(), gr.double()))
    worst = max(e_apply, e_grad) / 1e-5
    written = {"d", "U" if upd else "V"} | ({"U", "V"} if bal else set())
    for k, a, b in (("U", Ut, Ub), ("V", Vt, Vb)):
        if k not in written and not torch.equal(a.view(torch.int16), b.view(torch.int16)):
            print(name + ": %s was written" % k, flush=True)
            worst = float("inf")
    if any(t.dtype != bf for t in (Ut, Vt, dt)):
        worst = float("inf")
    n64 = lambda t: t.double().cpu().numpy()
    try:
        pn, pw, w = check_bf16_state(name, dict(U=n64(Ut), V=n64(Vt), d=n64(dt)), dict(U=n64(U64), V=n64(V64), d=n64(d64)),
                                     dict(U=Uw.cpu().numpy(), V=Vw.cpu().numpy(), d=dw.cpu().numpy()), written, rounding)
        worst = max(worst, w, pn / (2 * pw + 1e-4))   # nearest: codes off RNE(y64); stochastic: codes that are neither floor nor ceil
    except AssertionError as ex:
        print(name + ": element bound missed: %s" % (ex,), flush=True)
        worst = float("inf")
    return name + " [apply %.1e grad %.1e]" % (e_apply, e_grad), worst, 1.0


def run(budget, seed=1):
    _lib.load()
    g = torch.Generator(device=dev).manual_seed(seed)
    fams = [fuzz_kron, fuzz_kron_bf16, fuzz_kron_bf16_update, fuzz_uvd, fuzz_splu, fuzz_kron_sparse]
    if _WIDE_ONLY:
        fams = [fuzz_uvd, fuzz_splu]
    t0, it, worst, bad = time.time(), 0, {}, []
    while time.time() - t0 < budget:
        f = fams[it % len(fams)]
        name, err, tol = f(g, it // len(fams))           # the family's own counter: its `it % k` switches see every residue
        fam = name.split()[0]
        if err > worst.get(fam, (0, ""))[0]:
            worst[fam] = (err, name)
        if not (err < tol):
            bad.append((name, err))
            print("FAIL", name, err, flush=True)
        it += 1
    return it, bad, worst


FAMILIES = {"kron": fuzz_kron, "kron-bf16": fuzz_kron_bf16, "kron-bf16-upd": fuzz_kron_bf16_update, "uvd": fuzz_uvd, "splu": fuzz_splu,
            "kron-sparse": fuzz_kron_sparse, "dense": fuzz_dense, "uvd-bf16": fuzz_uvd_bf16}


def _tally(name, err, tol, worst, bad):
    """the bookkeeping of run()'s loop body (run() itself stays as it was: earlier recorded sweeps remain comparable)"""
    fam = name.split()[0]
    if err > worst.get(fam, (0, ""))[0]:
        worst[fam] = (err, name)
    if not (err < tol):
        bad.append((name, err))
        print("FAIL", name, err, flush=True)


def run_cases(families, n_per_family, seed, log=None):
    """Exactly n_per_family cases of each family (names of FAMILIES), each family on a generator of its own seeded from (seed, name)
    and its own counter it = 0 .. n - 1: which cases run depends on nothing but the arguments.  Returns (cases, bad, worst) as run()
    does; log (a list) receives every case's (name, err, tol)."""
    _lib.load()
    cases, worst, bad = 0, {}, []
    for fam in families:
        key = int.from_bytes(hashlib.sha256(("%d/%s" % (seed, fam)).encode()).digest()[:7], "little")
        g = torch.Generator(device=dev).manual_seed(key)
        for it in range(n_per_family):
            name, err, tol = FAMILIES[fam](g, it)
            _tally(name, err, tol, worst, bad)
            if log is not None:
                log.append((name, err, tol))
            cases += 1
    return cases, bad, worst


def run_all(budget, seed=1):
    """the command line's sweep: run()'s rotation over every family of FAMILIES"""
    _lib.load()
    g = torch.Generator(device=dev).manual_seed(seed)
    fams = [fuzz_uvd, fuzz_splu] if _WIDE_ONLY else list(FAMILIES.values())
    t0, it, worst, bad = time.time(), 0, {}, []
    while time.time() - t0 < budget:
        _tally(*fams[it % len(fams)](g, it // len(fams)), worst, bad)
        it += 1
    return it, bad, worst


if __name__ == "__main__":
    cases, bad, worst = run_all(float(sys.argv[1]) if len(sys.argv) > 1 else 120.0, int(os.environ.get("FUZZ_SEED", "1")))
    print("cases", cases, "failures", len(bad), "kron cases with a side >= 4096:", LARGE_KRON[0])
    for fam, (e, n) in worst.items():
        print("worst %-10s %.3e  (%s)" % (fam, e, n))
    sys.exit(1 if bad else 0)
