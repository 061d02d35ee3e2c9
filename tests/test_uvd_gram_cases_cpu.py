"""The inputs of tests/test_uvd_gram_conditioning_gpu.py are what they claim to be (no GPU): for every (shape, kind) that file runs,
K = I + V'U in fp64 from the fp32 U, V the maker returns -- and from their bf16 roundings for the cases the bf16-state tests use --
has at least the intended number of row exchanges in LAPACK's partially pivoted LU, for K and for K' (psgd.py:577-578 solves with
both), and the intended condition number within a factor 2.  A condition on the makers, not a measurement of the kernels: a later
edit to tests/uvd_cases.py cannot silently turn the inputs benign."""
import numpy as np
import pytest

from tests import uvd_cases as uc

SHAPES = [(1021, 1)] + uc.GRAM_SHAPES_LE32 + uc.GRAM_SHAPES_WIDE + uc.GRAM_SHAPES_CHUNK + [uc.GRAM_SHAPE_FEW_ROWS]


def _kinds(r):
    return [k for k in uc.GRAM_KINDS if r > 1 or k.startswith("cond")]       # r = 1: K is a scalar


def _check(K, m, kind, tag):
    """m = the size of the block that carries the kind (min(N, r))"""
    ex = min(uc.lu_exchanges(K), uc.lu_exchanges(K.T))
    cond = float(np.linalg.cond(K))
    if kind == "cyclic":
        assert ex >= m - 1, (tag, ex)
    elif kind == "reversal":
        assert ex >= m // 2, (tag, ex)
    elif kind == "smallpivot":
        assert ex >= 1 and 10.0 <= cond <= 3e3, (tag, ex, cond)       # benign for a pivoted solve ...
        assert abs(K[-m, -m]) < 1e-2 * np.max(np.abs(K[-m:, -m])), tag   # ... with a first pivot two orders below its column
    elif m > 1:
        want = uc.GRAM_COND[kind]
        assert want / 2 <= cond <= want * 2, (tag, cond)
    return ex, cond


@pytest.mark.parametrize("N,r", SHAPES)
def test_gram_cases_are_what_they_claim(N, r):
    for kind in _kinds(r):
        p = uc.gram_case(N, r, kind)
        assert p["U"].dtype == np.float32 and p["U"].shape == (N, r) and p["V"].shape == (N, r)
        _check(uc.gram_of(p), min(N, r), kind, (N, r, kind))
        if N >= r:                                                    # U = Q has orthonormal columns
            assert np.max(np.abs(p["U"].astype(np.float64).T @ p["U"].astype(np.float64) - np.eye(r))) < 1e-5


@pytest.mark.parametrize("N,r", uc.GRAM_SHAPES_LE32)
def test_gram_cases_survive_the_bf16_rounding(N, r):
    """the bf16-state tests round U, V to bf16 first: the same conditions on the K of the rounded codes"""
    for kind in uc.GRAM_KINDS_BF16:
        _check(uc.gram_of(uc.gram_case(N, r, kind), bf16=True), r, kind, (N, r, kind, "bf16"))


def test_cond1e4_does_not_survive_the_bf16_rounding():
    """why cond1e4 is not among GRAM_KINDS_BF16: at every shape the rounding moves K by more than its smallest singular value 1e-4
    (3e-4 .. 1.2e-3 in the 2-norm), so the condition number of the K of the rounded codes is whatever the rounding errors make it
    (4.0e3 at r = 2, 2.8e5 at r = 7, 2.4e4 at r = 32): not within a factor 2 of 1e4"""
    assert set(uc.GRAM_KINDS) - set(uc.GRAM_KINDS_BF16) == {"cond1e4"}
    conds = []
    for N, r in uc.GRAM_SHAPES_LE32:
        p = uc.gram_case(N, r, "cond1e4")
        K, Kb = uc.gram_of(p), uc.gram_of(p, bf16=True)
        assert 5e3 <= np.linalg.cond(K) <= 2e4
        assert np.linalg.norm(Kb - K, 2) > 2 * np.linalg.svd(K, compute_uv=False)[-1], (N, r)
        conds.append(float(np.linalg.cond(Kb)))
    assert any(not 5e3 <= c <= 2e4 for c in conds), conds


@pytest.mark.parametrize("N,r", uc.EXACT_SHAPES_BF16)
def test_exact_cases_survive_the_bf16_rounding(N, r):
    """the exact maker's U, V are bf16 numbers: the bf16-state tests get K == A bit for bit, with zeropivot's r - 1 exchanges and an
    exactly zero diagonal, and the tied candidates of ties / ties_late"""
    assert r <= 32 and set(uc.EXACT_KINDS_BF16) == {"ties", "ties_late", "zeropivot"}
    for kind in uc.EXACT_KINDS_BF16:
        p = uc.exact_case(N, r, kind)
        for k in ("U", "V"):
            assert np.array_equal(uc.to_bf16_np(p[k]), p[k]), (kind, k)
        Kb = uc.gram_of(p, bf16=True)
        assert np.array_equal(Kb, uc.exact_gram_kinds(r)[kind]), kind
    assert not np.diag(Kb).any() and uc.lu_exchanges(Kb) == r - 1 and uc.lu_exchanges(Kb.T) == r - 1


def test_with_gram_reproduces_A():
    rng = np.random.default_rng(3)
    for N, r in ((300, 12), (64, 64)):
        A = rng.standard_normal((r, r))
        p = uc.make_uvd_problem_with_gram(N, r, A, seed=5)
        assert np.max(np.abs(uc.gram_of(p) - A)) < 2e-6 * np.max(np.abs(A))
    with pytest.raises(AssertionError):                               # N < r: A - I of full column rank cannot be V'U
        uc.make_uvd_problem_with_gram(5, 8, rng.standard_normal((8, 8)), seed=1)


@pytest.mark.parametrize("N,r", uc.EXACT_SHAPES)
def test_exact_gram_is_exact(N, r):
    rows = uc.exact_gram_rows(N, r)
    assert rows[0] == 0 and rows[1] == N - 1 and {63, 64, 255, 256} <= set(rows) and len(set(rows)) == r
    kinds = uc.exact_gram_kinds(r)
    for kind, A in kinds.items():
        p = uc.exact_case(N, r, kind)
        assert np.array_equal(uc.gram_of(p), A), kind                 # bit for bit
        for perm in (np.arange(N)[::-1], np.random.default_rng(1).permutation(N)):     # ... in any summation order
            K32 = np.eye(r, dtype=np.float32)
            for n in perm[np.isin(perm, rows)]:                         # (the other rows of U are zero)
                K32 += np.outer(p["V"][n], p["U"][n])
            assert np.array_equal(K32.astype(np.float64), A), kind
    m = 1 << (r.bit_length() - 1)
    T = kinds["ties"]
    assert np.all(np.abs(T[:m, :m]) == 0.25)
    # ties: at every elimination step the candidates of the pivot column that are not zero are all of one size
    M = T.copy()
    tied = 0
    for k in range(m - 1):
        col = np.abs(M[k:m, k])
        nz = col[col > 0]
        assert len(nz) >= 1 and np.all(nz == nz[0])
        tied += len(nz) > 1
        j = k + int(np.argmax(col))
        M[[k, j]] = M[[j, k]]
        M[k + 1:] -= np.outer(M[k + 1:, k] / M[k, k], M[k])
    assert tied >= m // 2
    L = kinds["ties_late"]
    assert np.argmax(np.abs(L[:, 0])) == m - 1 and uc.lu_exchanges(L) >= 1
    assert np.linalg.cond(T) < 2 and np.linalg.cond(L) < 2
    Z = kinds["zeropivot"]
    assert not np.diag(Z).any() and uc.lu_exchanges(Z) == r - 1 and uc.lu_exchanges(Z.T) == r - 1
    S = kinds["singular"]
    assert not S[min(3, r - 1)].any() and np.linalg.matrix_rank(S) == r - 1
