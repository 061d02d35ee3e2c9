"""Seeded synthetic UVd problems shared by the CPU and GPU tests (SURVEY 8d inputs)."""
import numpy as np

TINY32 = float(np.finfo(np.float32).tiny)


def make_uvd_problem(N, r, seed=0, uv_gain=1.0, d_spread=0.0):
    """U, V ~ N(0,1) * uv_gain * (N r)^-1/2 (psgd.py:687-689), d = exp(d_spread * N(0,1))
    (d = 1 at d_spread = 0, psgd.py:690), g, v ~ N(0,1) (psgd.py:713), h = c .* v with
    c ~ LogUniform[1e-2, 1e2] (a diagonal SPD Hessian).  All fp32 arrays; d,g,v,h are [N,1]."""
    rng = np.random.default_rng(seed)
    scale = uv_gain * (1.0 / (N * r)) ** 0.5
    U = (rng.standard_normal((N, r)) * scale).astype(np.float32)
    V = (rng.standard_normal((N, r)) * scale).astype(np.float32)
    d = np.exp(d_spread * rng.standard_normal((N, 1))).astype(np.float32)
    g = rng.standard_normal((N, 1)).astype(np.float32)
    v = rng.standard_normal((N, 1)).astype(np.float32)
    c = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=(N, 1)))
    h = (c * v).astype(np.float32)
    return dict(U=U, V=V, d=d, g=g, v=v, h=h)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))


def bf16_grid(y):
    """(floor, ceil, round-to-nearest-even, spacing) of fp64 values on the bf16 grid (normal range)"""
    y = np.asarray(y, dtype=np.float64)
    _, ex = np.frexp(np.where(y == 0, 1.0, y))
    s = np.ldexp(1.0, ex - 1 - 7)
    q = y / s
    return np.floor(q) * s, np.ceil(q) * s, np.round(q) * s, s


def to_bf16_np(x):
    """fp32 array -> the fp32 array of its bf16 roundings (round to nearest even)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).float().numpy()


def check_bf16_state(tag, stored, y64, widen32, written, rounding):
    """A bf16-stored UVd state against the fp64 oracle's y64 (dicts of arrays under "U", "V", "d"; stored: the codes widened to
    fp64; widen32: the fp32 kernels' result on the widened inputs; written: the tensors the call rewrote).  Asserts the element
    bound |stored - y64| <= 2^-7 |y64| + 1e-5 rms(y64) on every tensor; returns the pooled shares (p_native, p_widen) over the
    written tensors of codes that differ from RNE_bf16(y64) (stochastic: that are neither floor nor ceil of y64) and the largest
    err / bound met."""
    bad_n = bad_w = total = 0
    worst = 0.0
    for k in ("U", "V", "d"):
        s, y = stored[k], y64[k]
        rms = float(np.sqrt(np.mean(y * y)))
        err = np.abs(s - y)
        bound = 2.0 ** -7 * np.abs(y) + 1e-5 * rms
        assert np.all(err <= bound), (tag, k, float(np.max(err - bound)))
        if err.size:
            worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
        if k not in written:
            continue
        lo, hi, rne, _ = bf16_grid(y)
        if rounding == "nearest":
            bad_n += int(np.sum(s != rne))
        else:
            bad_n += int(np.sum((s != lo) & (s != hi)))
        bad_w += int(np.sum(to_bf16_np(widen32[k]).astype(np.float64) != rne))
        total += y.size
    return bad_n / total, bad_w / total, worst


# ------------------------------------------------------------------------------------------------ problems with a chosen K = I + V'U
def _columns(rng, N, d_spread):
    """d, g, v, h as make_uvd_problem draws them"""
    d = np.exp(d_spread * rng.standard_normal((N, 1))).astype(np.float32)
    g = rng.standard_normal((N, 1)).astype(np.float32)
    v = rng.standard_normal((N, 1)).astype(np.float32)
    c = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), size=(N, 1)))
    return d, g, v, (c * v).astype(np.float32)


def make_uvd_problem_with_gram(N, r, A, seed, d_spread=0.3):
    """The dict of make_uvd_problem with U = Q and V = Q (A - I)', Q'Q = I: K = I + V'U = A up to the fp32 rounding of U and V
    (psgd.py:574-578 solves with K and K').  N >= r: Q [N, r] from the QR of a Gaussian.  N < r: V'U has rank <= N, so A - I may have
    at most N non-zero columns; Q then has orthonormal columns at those positions and zero columns elsewhere."""
    A = np.asarray(A, dtype=np.float64)
    assert A.shape == (r, r)
    rng = np.random.default_rng(seed)
    if N >= r:
        Q = np.linalg.qr(rng.standard_normal((N, r)))[0]
    else:
        J = np.flatnonzero(np.any(A - np.eye(r) != 0, axis=0))
        assert len(J) <= N, "A - I has %d non-zero columns, U and V only %d rows" % (len(J), N)
        Q = np.zeros((N, r))
        Q[:, J] = np.linalg.qr(rng.standard_normal((N, len(J))))[0]
    U = Q.astype(np.float32)
    V = (Q @ (A - np.eye(r)).T).astype(np.float32)
    d, g, v, h = _columns(rng, N, d_spread)
    return dict(U=U, V=V, d=d, g=g, v=v, h=h)


def exact_gram_rows(N, r):
    """r distinct rows of [0, N) for make_uvd_problem_exact_gram: the first and the last row, both sides of the 64- and 256-row tile
    boundaries, the rest spread evenly -- the partial sums of the Gram cross waves, workgroups and the partial last tile."""
    assert N >= r
    rows = []
    for x in [0, N - 1, 63, 64, 255, 256, N - 2, 127, 128] + [int(t) for t in np.linspace(1, N - 3, 4 * r)]:
        if 0 <= x < N and x not in rows:
            rows.append(x)
    for x in range(N):
        if len(rows) >= r:
            break
        if x not in rows:
            rows.append(x)
    return rows[:r]


def make_uvd_problem_exact_gram(N, r, A, rows, seed=0, d_spread=0.3):
    """U has e_k in row rows[k], V has row k of (A - I)' there, zeros elsewhere: with small dyadic entries in A every product and sum of
    V'U is exact, so K == A bit for bit in any summation order."""
    A = np.asarray(A, dtype=np.float64)
    assert A.shape == (r, r) and len(rows) == r and len(set(rows)) == r and 0 <= min(rows) and max(rows) < N
    assert np.array_equal(A * 64, np.round(A * 64)) and np.max(np.abs(A)) <= 2, "entries of A: small multiples of 1/64"
    U = np.zeros((N, r), dtype=np.float32)
    V = np.zeros((N, r), dtype=np.float32)
    B = (A - np.eye(r)).T
    for k, n in enumerate(rows):
        U[n, k] = 1.0
        V[n, :] = B[k]
    d, g, v, h = _columns(np.random.default_rng(seed), N, d_spread)
    return dict(U=U, V=V, d=d, g=g, v=v, h=h)


GRAM_KINDS = ("cyclic", "reversal", "smallpivot", "cond1e2", "cond1e3", "cond1e4")
GRAM_COND = {"cond1e2": 1e2, "cond1e3": 1e3, "cond1e4": 1e4}
# the bf16-state cases: rounding U, V to bf16 moves K by ~1e-4, more than the smallest singular value of cond1e4
GRAM_KINDS_BF16 = ("cyclic", "reversal", "smallpivot", "cond1e2", "cond1e3")


def gram_kinds(r, rng):
    """Named r x r matrices A for make_uvd_problem_with_gram:
      cyclic      the identity rolled by one row + 0.05 N(0,1): r - 1 row exchanges, every pivot sits off its own row
      reversal    the anti-identity + 0.05 N(0,1): r // 2 exchanges
      smallpivot  I + 0.3 N(0,1) with A[0,0] = 1e-6: elimination without pivoting blows up, with it the solve is benign
      cond1eK     W1 diag(logspace(0, -K, r)) W2' with random orthogonal W1, W2: condition number 1eK"""
    out = {}
    out["cyclic"] = np.roll(np.eye(r), 1, axis=0) + 0.05 * rng.standard_normal((r, r))
    out["reversal"] = np.eye(r)[::-1] + 0.05 * rng.standard_normal((r, r))
    A = np.eye(r) + 0.3 * rng.standard_normal((r, r))
    A[0, 0] = 1e-6
    out["smallpivot"] = A
    for name, c in GRAM_COND.items():
        W1 = np.linalg.qr(rng.standard_normal((r, r)))[0]
        W2 = np.linalg.qr(rng.standard_normal((r, r)))[0]
        out[name] = W1 @ np.diag(np.logspace(0.0, -np.log10(c), r)) @ W2.T
    return out


def embed_gram(A, r):
    """A in the trailing block of the r x r identity (N < r: A - I may have only N non-zero columns)"""
    m = A.shape[0]
    out = np.eye(r)
    out[r - m:, r - m:] = A
    return out


def exact_gram_kinds(r):
    """Dyadic matrices for make_uvd_problem_exact_gram.  H = the Sylvester Hadamard matrix of the largest power of two m <= r.
      ties       H / 4 in the leading m x m block, the identity behind it: at every step all candidates of the pivot column that are
                 not zero have the same size (the Schur complements of H are Hadamard matrices again)
      ties_late  ties with A[m - 1, 0] = 1/2: one forced exchange first, ties from then on
      singular   ties with row 3 (r >= 4) set to zero: K is exactly singular
      zeropivot  the identity rolled by one row, nothing added: every diagonal entry is exactly zero, so an elimination that does not
                 exchange rows divides by zero at its first step (the solves run in fp64: a pivot that is merely small, as in
                 `smallpivot` or `cyclic`, costs such an elimination ~1e-12, far inside bars set for fp32 storage)"""
    m = 1
    while 2 * m <= r:
        m *= 2
    H = np.ones((1, 1))
    while H.shape[0] < m:
        H = np.block([[H, H], [H, -H]])
    ties = np.eye(r)
    ties[:m, :m] = H / 4.0
    late = ties.copy()
    late[m - 1, 0] = 0.5
    sing = ties.copy()
    sing[min(3, r - 1), :] = 0.0
    return {"ties": ties, "ties_late": late, "singular": sing, "zeropivot": np.roll(np.eye(r), 1, axis=0)}


def lu_exchanges(K):
    """row exchanges of LAPACK's partially pivoted LU of K (scipy.linalg.lu_factor)"""
    import scipy.linalg
    piv = scipy.linalg.lu_factor(np.asarray(K, dtype=np.float64))[1]
    return int(np.sum(piv != np.arange(len(piv))))


def gram_of(p, bf16=False):
    """K = I + V'U in fp64 from the fp32 U, V of a problem (bf16: from their bf16 roundings)"""
    U, V = (to_bf16_np(p[k]) if bf16 else p[k] for k in ("U", "V"))
    return np.eye(U.shape[1]) + V.astype(np.float64).T @ U.astype(np.float64)


# The cases of tests/test_uvd_gram_conditioning_gpu.py, checked without a GPU by tests/test_uvd_gram_cases_cpu.py.
GRAM_SHAPES_LE32 = [(257, 2), (1021, 7), (257, 8), (1021, 9), (257, 17), (1021, 32)]
GRAM_SHAPES_WIDE = [(2049, 33), (2049, 40), (2049, 41), (2049, 48), (2049, 56), (2049, 57), (2049, 64)]
GRAM_SHAPES_CHUNK = [(2049, 65), (2049, 100)]
GRAM_SHAPE_FEW_ROWS = (31, 57)
EXACT_SHAPES = [(257, 8), (1021, 16), (257, 32), (2049, 40), (2049, 64)]
# The bf16-state cases of the exact maker (ranks to 32): its entries 0, +-1/4, 1/2, 3/4, +-1, 5/4 are bf16 numbers, K stays exact.
# All but r rows of its U and V are zero, so nearly every rewritten element is a pure increment: a handful (k ~ 3 .. 6) of fp32
# roundings on a value of its own size, not on a small addition to a base.  Such an element lands on another bf16 code than
# RNE(fp64 value) with probability k 2^-24 / 2^-8 .. 2^-7, about 2e-5 .. 2e-4 -- in the fp32 kernels on the widened inputs as in the
# native ones -- which is the size of the floor 1e-4 in p_native <= 2 p_widen + 1e-4.  For that rule to compare shares and not
# single codes, the count N r must put the margin (p + 1e-4) N r several standard deviations sqrt(5 p N r) of the two counts apart:
# N r >= 2e5 gives 4 or more for every p in that range.  Hence N = 32771, 16387, 8197 (odd: a partial last tile), still milliseconds.
EXACT_SHAPES_BF16 = [(32771, 8), (16387, 16), (8197, 32)]
EXACT_KINDS_BF16 = ("ties", "ties_late", "zeropivot")


def gram_case(N, r, kind):
    """The problem of one (N, r, kind): its seed depends on nothing but the three.  N < r: the kind at size N in the trailing block."""
    seed = 1000 * r + N + 7 * GRAM_KINDS.index(kind)
    m = min(N, r)
    A = gram_kinds(m, np.random.default_rng(seed))[kind]
    return make_uvd_problem_with_gram(N, r, embed_gram(A, r), seed + 1)


def exact_case(N, r, kind):
    return make_uvd_problem_exact_gram(N, r, exact_gram_kinds(r)[kind], exact_gram_rows(N, r), seed=N + r)
