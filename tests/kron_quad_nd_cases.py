"""The three-factor QUAD update's reference (include/psgd_kron_quad_nd_hip.h restated with torch.tensordot; run in float64) and
test inputs, made as tests/kron_quad_cases.py makes them.  Bars and quad_bound are that module's."""
import torch

from tests import kron_quad_cases as qc

# (A, B, C, seed): an odd seed starts L above ell, an even one below it; problem()'s tie condition holds for these seeds
CASES = [(1, 1, 1, 0), (2, 3, 5, 1), (3, 65, 9, 0), (4, 68, 20, 1), (5, 7, 16, 0), (65, 3, 2, 1), (70, 66, 3, 0), (6, 64, 64, 1),
         (3, 4, 130, 0), (2, 130, 1, 1)]
BIT_CASES = [(65, 131, 0), (68, 132, 1)]    # (B, C, seed) of qc.problem(): [1, B, C] against the two-factor update on [B, C]


def mode_product(X, Q, k):
    """X xk Q: the mode-k unfolding of the result is Q X_(k)"""
    return torch.movedim(torch.tensordot(Q, X, dims=([1], [k])), 0, k)


def nd_apply_ref(Qs, G):
    for k, Q in enumerate(Qs):
        G = mode_product(mode_product(G, Q, k), Q, k)
    return G


def nd_terms(Qs, G):
    X = G
    for k, Q in enumerate(Qs):
        X = mode_product(X, Q, k)
    unfold = [torch.movedim(X, k, 0).reshape(X.shape[k], -1) for k in range(3)]
    return [(U @ U.T, float(G.numel() // G.shape[k])) for k, U in enumerate(unfold)]


def nd_update_ref(Qs, L, G, step=qc.STEP, decay=qc.DECAY):
    """([new Qa, new Qb, new Qc], new L) from the old state; in the dtype of its inputs"""
    out, Ln = [], []
    for (T_, t2), Q, L0 in zip(nd_terms(Qs, G), Qs, L):
        ell = qc.quad_bound(T_) + t2
        L1 = torch.maximum(decay * L0 + (1 - decay) * ell, ell)
        c = step / (2 * L1)
        P1 = Q - c * (T_ @ Q - t2 * Q)
        P2 = P1 - c * (P1 @ T_ - t2 * P1)
        out.append((P2 + P2.T) / 2)
        Ln.append(L1)
    return out, torch.stack(Ln)


_cache = {}


def problem(A, B, C, seed):
    """float32 Qs (a list of three), L, G and float64 out, new_Qs, new_L, out_new; made once, never modified"""
    if (A, B, C, seed) not in _cache:
        gen = torch.Generator().manual_seed(7300 + seed)
        G = torch.randn(A, B, C, generator=gen)
        G[0] *= 1.5
        G[:, 0] *= 1.5
        G[:, :, 0] *= 1.5
        Qs = [qc._spd(n, gen) for n in (A, B, C)]
        dQ, dG = [Q.double() for Q in Qs], G.double()
        terms = nd_terms(dQ, dG)
        for T_, _ in terms:                   # a condition on the inputs: no near-tie in the choice of j, on any side
            top = torch.sort((T_ * T_).sum(0), descending=True).values[:2]
            assert len(top) < 2 or float(top[0] - top[1]) >= 0.01 * float(top[0]), (A, B, C, seed)
        ell = torch.stack([qc.quad_bound(T_) + t2 for T_, t2 in terms])
        p = dict(Qs=Qs, G=G, L=((2.0 if seed % 2 else 0.5) * ell).float())
        p["out"] = nd_apply_ref(dQ, dG)
        p["new_Qs"], p["new_L"] = nd_update_ref(dQ, p["L"].double(), dG)
        p["out_new"] = nd_apply_ref(p["new_Qs"], dG)
        _cache[(A, B, C, seed)] = p
    return _cache[(A, B, C, seed)]
