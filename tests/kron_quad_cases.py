"""The QUAD Kronecker update's reference (include/psgd_kron_quad_hip.h restated in plain torch; run in float64, or in float32 for
the drift rule) and test inputs.  Bars: README, "Parity" -- relative and norm-wise."""
import torch

STEP, DECAY = 0.1, 0.95
STATE_BAR, INCREMENT_BAR, APPLY_BAR, L_BAR = 1e-5, 2e-3, 1e-5, 1e-5
T = 64                                # PSGD_KRON_QUAD_TILE
# (M, N, seed): an odd seed starts L above ell (the blend arm of the max), an even one below it; the seeds are those for which
# problem()'s tie condition holds
CASES = [(1, 1, 0), (1, 7, 1), (7, 1, 2), (3, 5, 3), (T - 1, T + 1, 4), (T, T, 5), (T + 1, 2 * T + 3, 6), (33, 515, 7),
         (2 * T + 3, 5, 8)]


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


def problem(M, N, seed):
    """float32 Ql, Qr, L, G and float64 out, new_Ql, new_Qr, new_L, out_new; made once, never modified"""
    if (M, N, seed) not in _cache:
        gen = torch.Generator().manual_seed(7000 + seed)
        G = torch.randn(M, N, generator=gen)
        G[0, :] *= 1.5
        G[:, 0] *= 1.5
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
        _cache[(M, N, seed)] = p
    return _cache[(M, N, seed)]


def err(x, ref):
    d, n = float((x.detach().double().cpu() - ref).norm()), float(ref.norm())
    return d / n if n else d
