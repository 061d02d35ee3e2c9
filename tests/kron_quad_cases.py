"""The QUAD Kronecker update's reference (include/psgd_kron_quad_hip.h restated in plain torch; run in float64, or in float32 for
the drift rule) and test inputs.  Bars: README, "Parity" -- relative, norm-wise over the matrix (err) and over each tile (tile_err).

exact_problem() makes inputs on which every intermediate of the apply and of the update is an fp32 number, so that the kernels must
reproduce the float64 reference bit for bit in any summation order (exact_bounds() is the condition, checked on the CPU)."""
import torch

STEP, DECAY = 0.1, 0.95
STATE_BAR, INCREMENT_BAR, APPLY_BAR, L_BAR = 1e-5, 2e-3, 1e-5, 1e-5
T = 64                                # PSGD_KRON_QUAD_TILE
# (M, N, seed): an odd seed starts L above ell (the blend arm of the max), an even one below it; the seeds are those for which
# problem()'s tie condition holds
CASES = [(1, 1, 0), (1, 7, 1), (7, 1, 2), (3, 5, 3), (T - 1, T + 1, 4), (T, T, 5), (T + 1, 2 * T + 3, 6), (33, 515, 7),
         (2 * T + 3, 5, 8),
         # leading dimensions that are multiples of 4, so that g2r() takes 16-byte loads: partial edge tiles beside full ones;
         # full tiles only, 2 x 2 and 3 x 3; M > N; a K of 4 (mod 16), where 16-byte steps end in a dword tail
         (T + 4, 2 * T + 4, 10), (2 * T, 3 * T, 11), (2 * T + 4, T + 8, 12), (T, T + 20, 13)]
# (M, N, seed, column of G scaled by 3): the right side's j lies past kLipT = 1024, in the second trip of k_lipschitz's loops
LIP_CASE = (5, 1024 + 76, 9, 1024 + 37)

# exact arithmetic: L starts at EXACT_L0 on both sides, decay = 1, so L stays and c = EXACT_STEP / (2 EXACT_L0) = 1/4 exactly
EXACT_STEP, EXACT_L0, EXACT_DECAY = 2048.0, 4096.0, 1.0
EXACT_C = EXACT_STEP / (2 * EXACT_L0)
EXACT_LIMIT = float(2 ** 24)
# (M, N, seed) of exact_problem(): apply and update
EXACT_CASES = [(1, 1, 0), (3, 5, 1), (T - 1, T + 1, 2), (T, T, 3), (T + 1, 2 * T + 3, 4), (T + 4, 2 * T + 4, 5), (2 * T, 3 * T, 6),
               (2 * T + 4, T + 8, 7), (T, T + 20, 8)]
# (M, N, seed, shift) of shift_problem(): apply only, factors that are not symmetric
SHIFT_CASES = [(T + 4, 2 * T + 4, 20, 1), (T + 4, 2 * T + 4, 21, -1)]


def quad_apply_ref(Ql, Qr, G):
    return Ql @ (Ql @ G @ Qr) @ Qr


def quad_terms(Ql, Qr, G):
    A = Ql @ G @ Qr
    return (A @ A.T, float(G.shape[1])), (A.T @ A, float(G.shape[0]))


def quad_bound(T_):
    s = T_.abs().max()
    if s == 0:
        return torch.zeros((), dtype=T_.dtype)
    Ts = T_ / s
    x = Ts[:, int(torch.argmax((Ts * Ts).sum(0)))]
    y = Ts @ x
    return s * (Ts @ (y / y.norm())).norm()


def quad_update_ref(Ql, Qr, L, G, step=STEP, decay=DECAY):
    """(new Ql, new Qr, new L) from the old state; in the dtype of its inputs"""
    out, Ln = [], []
    for (T_, t2), Q, L0 in zip(quad_terms(Ql, Qr, G), (Ql, Qr), L):
        ell = quad_bound(T_) + t2
        L1 = torch.maximum(decay * L0 + (1 - decay) * ell, ell)
        c = step / (2 * L1)
        P1 = Q - c * (T_ @ Q - t2 * Q)
        P2 = P1 - c * (P1 @ T_ - t2 * P1)
        out.append((P2 + P2.T) / 2)
        Ln.append(L1)
    return out[0], out[1], torch.stack(Ln)


def _spd(n, gen):
    X = torch.randn(n, n, generator=gen)
    return torch.eye(n) + 0.3 * (X + X.T) / 2 / n ** 0.5


_cache = {}


def problem(M, N, seed, col=None):
    """float32 Ql, Qr, L, G and float64 out, new_Ql, new_Qr, new_L, out_new; made once, never modified.  col: a column of G that
    is scaled by 3, which makes it the right side's choice of j."""
    if (M, N, seed, col) not in _cache:
        gen = torch.Generator().manual_seed(7000 + seed)
        G = torch.randn(M, N, generator=gen)
        G[0, :] *= 1.5
        G[:, 0] *= 1.5
        if col is not None:
            G[:, col] *= 3.0
        Ql, Qr = _spd(M, gen), _spd(N, gen)
        terms = quad_terms(Ql.double(), Qr.double(), G.double())
        for T_, _ in terms:               # a condition on the inputs: no near-tie in the choice of j
            top = torch.sort((T_ * T_).sum(0), descending=True).values[:2]
            assert len(top) < 2 or float(top[0] - top[1]) >= 0.01 * float(top[0]), (M, N, seed)
        ell = torch.stack([quad_bound(T_) + t2 for T_, t2 in terms])
        p = dict(Ql=Ql, Qr=Qr, G=G, L=((2.0 if seed % 2 else 0.5) * ell).float())
        d = {k: t.double() for k, t in p.items()}
        p["out"] = quad_apply_ref(d["Ql"], d["Qr"], d["G"])
        p["new_Ql"], p["new_Qr"], p["new_L"] = quad_update_ref(d["Ql"], d["Qr"], d["L"], d["G"])
        p["out_new"] = quad_apply_ref(p["new_Ql"], p["new_Qr"], d["G"])
        _cache[(M, N, seed, col)] = p
    return _cache[(M, N, seed, col)]


def _sparse_sym(n, gen):
    """identity plus, per row, one symmetric pair of off-diagonal entries drawn from {-1, 0, 1}: about two per row"""
    Q = torch.eye(n)
    if n > 1:
        other = (torch.arange(n) + torch.randint(1, n, (n,), generator=gen)) % n
        value = torch.randint(-1, 2, (n,), generator=gen).float()
        for i in range(n):
            Q[i, other[i]] = Q[other[i], i] = value[i]
    return Q


def _sparse_int(M, N, gen):
    """M x N with min(3, N) entries per row from {-2, -1, 1, 2} and one more in every column they left empty"""
    pick = lambda count: torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (count,), generator=gen)]
    G = torch.zeros(M, N)
    for i in range(M):
        cols = torch.randperm(N, generator=gen)[:min(3, N)]
        G[i, cols] = pick(len(cols))
    empty = torch.nonzero(G.abs().sum(0) == 0).flatten()
    G[torch.randint(0, M, (len(empty),), generator=gen), empty] = pick(len(empty))
    return G


def exact_problem(M, N, seed):
    """problem()'s keys on sparse small-integer inputs (out_new left out), with step, decay and L = [L0, L0] such that the step
    coefficient is the power of two EXACT_C; made once, never modified"""
    key = ("exact", M, N, seed)
    if key not in _cache:
        gen = torch.Generator().manual_seed(9000 + seed)
        p = dict(Ql=_sparse_sym(M, gen), Qr=_sparse_sym(N, gen), G=_sparse_int(M, N, gen), L=torch.full((2,), EXACT_L0))
        d = {k: t.double() for k, t in p.items()}
        p["step"], p["decay"] = EXACT_STEP, EXACT_DECAY
        p["out"] = quad_apply_ref(d["Ql"], d["Qr"], d["G"])
        p["new_Ql"], p["new_Qr"], p["new_L"] = quad_update_ref(d["Ql"], d["Qr"], d["L"], d["G"], EXACT_STEP, EXACT_DECAY)
        _cache[key] = p
    return _cache[key]


def exact_bounds(p, c=EXACT_C):
    """{stage: the largest magnitude any partial sum of that stage can reach, in units of the stage's least significant bit}:
    the chain on |Ql|, |G|, |Qr| with sums in place of differences.  Below 2^24 everywhere, every partial sum of every stage is
    an fp32 number in ANY summation order."""
    Ql, Qr, G = (p[k].double().abs() for k in ("Ql", "Qr", "G"))
    A = Ql @ G @ Qr
    b = {"apply": float((Ql @ A @ Qr).max())}             # |Q| >= I element-wise: the chain's prefixes are no larger
    for side, T_, Q, t2 in (("l", A @ A.T, Ql, float(G.shape[1])), ("r", A.T @ A, Qr, float(G.shape[0]))):
        TQ = T_ @ Q + t2 * Q
        P1 = Q + c * TQ
        P1T = P1 @ T_ + t2 * P1
        P2 = P1 + c * P1T
        b.update({"T" + side: float(T_.max()), "TQ" + side: float(TQ.max()), "P1T" + side: float(P1T.max()) / c,
                  "P2" + side: float(P2.max()) / c ** 2, "sym" + side: float((P2 + P2.T).max()) / c ** 2})
    return b


def shift_problem(M, N, seed, shift):
    """apply only: Ql and Qr are the cyclic-shift permutations by `shift` (not symmetric), G is dense; out is G with its rows and
    columns rotated by two -- one non-zero term per sum, so exact for any G"""
    key = ("shift", M, N, seed, shift)
    if key not in _cache:
        G = torch.randn(M, N, generator=torch.Generator().manual_seed(9500 + seed))
        Ql, Qr = torch.roll(torch.eye(M), shift, 1), torch.roll(torch.eye(N), shift, 1)
        # (Ql X)[i] = X[i + shift], (X Qr)[:, j] = X[:, j - shift]
        _cache[key] = dict(Ql=Ql, Qr=Qr, G=G, out=torch.roll(G, (-2 * shift, 2 * shift), (0, 1)).double())
    return _cache[key]


def err(x, ref):
    d, n = float((x.detach().double().cpu() - ref).norm()), float(ref.norm())
    return d / n if n else d


def tile_err(x, ref):
    """the largest err() over the T x T tiles of the matrix, edge tiles included"""
    x = x.detach().double().cpu()
    return max(err(x[i:i + T, j:j + T], ref[i:i + T, j:j + T]) for i in range(0, ref.shape[0], T) for j in range(0, ref.shape[1], T))
