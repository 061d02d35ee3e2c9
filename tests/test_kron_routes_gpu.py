"""fp64 parity of the Kron dense (x) dense update and apply on both sides of every route threshold, and on the layer shapes of
transformers (one long side).  The fp32 update and apply, the bf16-operand update and apply pick their routes by shape
(psgd_kron_dd_route_flags reports the choice); each route is compared with the fp64 torch restatement
(oracle/psgd_oracle_torch.py) on the device, at the suite's bars:

  fp32 apply and updated factors 1e-5 (relative, norm-wise); fp32 increments Q_new - Q_balanced 2e-3 (the check with teeth:
  step 0.01 dilutes an error of the factor); bf16 operands 2e-2 on the apply and the increments, BF16_UPD_STATE_TOL on the factors.

test_route_table_straddles_its_thresholds pins the table to the code: every boundary pair lies on the two sides of the flag it
names, so a moved threshold fails there, by name, instead of leaving both shapes on one side unnoticed."""
import numpy as np
import pytest
import torch

from oracle import psgd_oracle_torch as ref64
from psgd_tf_amd import _lib
from tests.kron_cases import illcond_factor
from tests.test_kron_gpu import BF16_UPD_STATE_TOL, INCR_TOL, TOL

pytestmark = pytest.mark.gpu

BF16_TOL = 2e-2
TINY = float(np.finfo(np.float32).tiny)
STEP = 0.01

# (M, N, why, families); every entry also runs transposed unless it is square or "one" is among its families.
#   upd: fp32 update (a) and bf16 apply (e) -- every entry but the apply splits;  ill: ill-conditioned fp32 update (b) and the
#   bf16-operand update (c);  mag: one data-magnitude variant (f);  teeth: a zeroed 128 x 128 tile must fail the bars.
# Every entry runs the fp32 apply (d).
TABLE = [
    # solves through explicit inverses: the three tiers of kron_inv_route, one short of each side
    (1023, 2048, "inverse tier (1024, 2048): small side one short", "upd ill"),
    (1024, 2047, "inverse tier (1024, 2048): large side one short", "upd ill"),
    (1024, 2048, "inverse tier (1024, 2048)", "upd ill teeth"),
    (511, 2560, "inverse tier (512, 2560): small side one short", "upd ill"),
    (512, 2559, "inverse tier (512, 2560): large side one short", "upd ill"),
    (512, 2560, "inverse tier (512, 2560); gradient split in 6 chunks", "upd ill"),
    (255, 4096, "inverse tier (256, 4096): small side one short", "upd ill"),
    (256, 4095, "inverse tier (256, 4096): large side one short", "upd ill"),
    (256, 4096, "inverse tier (256, 4096); advertised layer", "upd ill mag"),
    # the 8192 cap of the inverse route: above it, substitution with matrix scales
    (256, 8192, "inverse route at the cap", "upd ill"),
    (256, 8193, "one past the cap: substitution", "upd ill"),
    (1024, 8192, "inverse route at the cap; advertised layer", "upd ill"),
    (1024, 8193, "one past the cap: substitution", "upd ill"),
    # stream order of the inverse route
    (2048, 8192, "M N = 4096^2: inversions first", "upd ill"),
    (2049, 8192, "M N > 4096^2: products first", "upd ill"),
    (4096, 4096, "inversions first, products on a third stream", "upd ill"),
    (4096, 4097, "products first, ragged", "upd ill teeth"),
    (3072, 6144, "products first", "upd ill"),
    (6144, 6144, "products first", "upd ill mag"),
    # layers the README advertises, and ragged relatives (K not a multiple of a chunk)
    (1024, 4096, "MLP layer; apply split at exactly 256 output tiles", "upd mag teeth"),
    (768, 3072, "advertised layer", "upd"),
    (1536, 3072, "advertised layer", "upd"),
    (896, 3584, "advertised layer", "upd"),
    (768, 4096, "advertised layer", "upd"),
    (1280, 5120, "advertised layer", "upd mag"),
    (2048, 4096, "advertised layer", "upd"),
    (1000, 4100, "ragged MLP layer", "upd mag"),
    (384, 4100, "ragged, small side below every inverse tier", "upd"),
    (1030, 2070, "ragged inverse tier", "upd ill"),
    # rectangular gradient split: ratio 2, the chunk tiers, the 256-tile cap of the smaller triangle
    (1024, 1536, "gradient split, ratio 2", "upd"),
    (1024, 1535, "no gradient split, ratio < 2", "upd"),
    (1024, 3072, "gradient split in 4 chunks", "upd teeth"),
    (512, 3584, "gradient split in 8 chunks", "upd"),
    (2816, 4224, "gradient split, 253 tiles in the smaller triangle", "upd"),
    (2817, 4226, "no gradient split, 276 tiles", "upd mag"),
    # splits of the apply's products (fp32 apply only)
    (1032, 4096, "288 output tiles: no mid split", ""),
    (1024, 2016, "63 K steps: no mid split", ""),
    (1024, 2017, "64 K steps: mid split", ""),
    (128, 4096, "few-tile split", ""),
    (200, 3072, "few-tile split, ragged", ""),
    # operand planes of the apply and the update
    (896, 1024, "aligned: apply on the exact 64-tile kernels", "upd"),
    (1000, 1024, "unaligned: apply on planes", "upd"),
    (599, 300, "apply below the planes", "upd"),
    (600, 300, "apply on planes", "upd"),
    (513, 100, "update below the planes", "upd"),
    (513, 384, "update on planes", "upd"),
]

F = _lib
# boundary pairs: (shape on the side without the flag, shape with it, flag)
PAIRS = [
    ((1023, 2048), (1024, 2048), F.KRON_ROUTE_INV_SOLVES), ((1024, 2047), (1024, 2048), F.KRON_ROUTE_INV_SOLVES),
    ((511, 2560), (512, 2560), F.KRON_ROUTE_INV_SOLVES), ((512, 2559), (512, 2560), F.KRON_ROUTE_INV_SOLVES),
    ((255, 4096), (256, 4096), F.KRON_ROUTE_INV_SOLVES), ((256, 4095), (256, 4096), F.KRON_ROUTE_INV_SOLVES),
    ((256, 8193), (256, 8192), F.KRON_ROUTE_INV_SOLVES), ((1024, 8193), (1024, 8192), F.KRON_ROUTE_INV_SOLVES),
    ((2049, 8192), (2048, 8192), F.KRON_ROUTE_INV_FIRST), ((4096, 4097), (4096, 4096), F.KRON_ROUTE_INV_FIRST),
    ((3072, 6144), (2048, 8192), F.KRON_ROUTE_INV_FIRST), ((6144, 6144), (4096, 4096), F.KRON_ROUTE_INV_FIRST),
    ((2048, 8192), (4096, 4096), F.KRON_ROUTE_BG_FRONT),
    ((1024, 1535), (1024, 1536), F.KRON_ROUTE_GRAD_RECT), ((2817, 4226), (2816, 4224), F.KRON_ROUTE_GRAD_RECT),
    ((896, 1024), (1000, 1024), F.KRON_ROUTE_PLANES_APPLY), ((599, 300), (600, 300), F.KRON_ROUTE_PLANES_APPLY),
    ((513, 100), (513, 384), F.KRON_ROUTE_PLANES_UPDATE),
]
# the chunk tiers of the rectangular gradient split: distinct counts, growing with the ratio of the sides
CHUNK_TIERS = [(1024, 1536), (1024, 3072), (512, 2560), (512, 3584)]
# the apply's split-K rules live inside its launches (product dimensions, not the layer's): no flag; these pairs run both sides
APPLY_SPLIT_PAIRS = [((1032, 4096), (1024, 4096)), ((1024, 2016), (1024, 2017))]


def _entries():
    out = []
    for M, N, why, fam in TABLE:
        out.append((M, N, why, fam))
        if M != N and "one" not in fam:
            out.append((N, M, why + " (transposed)", fam))
    return out


ENTRIES = _entries()


def _cases(want):
    return [pytest.param(M, N, fam, id="%dx%d" % (M, N)) for M, N, why, fam in ENTRIES if want(fam)]


dev = torch.device("cuda:0")


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    d = torch.linalg.vector_norm(b)
    return float(torch.linalg.vector_norm(a - b) / (d if d > 0 else 1.0))


def _flags(M, N):
    return _lib.load().psgd_kron_dd_route_flags(M, N)


def _chunks(f):
    return (f & F.KRON_ROUTE_RECT_CHUNKS_MASK) >> F.KRON_ROUTE_RECT_CHUNKS_SHIFT


def _gen(M, N):
    return torch.Generator(device=dev).manual_seed(7919 * M + N)


def _tri(n, g, off):
    return torch.triu(torch.randn(n, n, device=dev, generator=g) * off, 1) + torch.diag(torch.exp(0.3 * torch.randn(n, device=dev, generator=g)))


def _balanced(M, N):
    """Factors as in tests/fuzz_gpu.py (Ql x 1.7: rho != 1), dG = row and column scalings of dX, and a gradient G."""
    g = _gen(M, N)
    off = 0.5 / max(M, N) ** 0.5
    Ql, Qr = _tri(M, g, off) * 1.7, _tri(N, g, off)
    dX = torch.randn(M, N, device=dev, generator=g)
    dG = torch.exp(torch.empty(M, 1, device=dev).uniform_(-1, 1, generator=g)) * dX \
        * torch.exp(torch.empty(1, N, device=dev).uniform_(-1, 1, generator=g))
    G = torch.randn(M, N, device=dev, generator=g)
    return Ql, Qr, dX, dG, G


def _solve(A, B, upper, cols=512):
    """A^-1 B for a triangular A, in blocks of columns of B (as the oracle does: the library's solve needs a workspace that grows
    with the right-hand side)."""
    return torch.cat([torch.linalg.solve_triangular(A, B[:, j:j + cols], upper=upper) for j in range(0, B.shape[1], cols)], 1)


def _illcond(M, N):
    """cond(Q) ~ 1e4 factors (tests/kron_cases.py) and dG near the fixed point, (Ql'Ql)^-1 dX (Qr'Qr)^-1 with column scalings, in fp64
    on the device."""
    rng = np.random.default_rng(M + 13 * N)
    Ql, Qr = (torch.from_numpy(illcond_factor(rng, n).astype(np.float32)).to(dev) for n in (M, N))
    g = _gen(M, N)
    dX = torch.randn(M, N, device=dev, generator=g)
    L, Rt = Ql.double(), Qr.double()
    X = _solve(L, _solve(L.t(), dX.double(), False), True)                              # (Ql'Ql)^-1 dX
    X = _solve(Rt, _solve(Rt.t(), X.t(), False), True).t()                              # ... (Qr'Qr)^-1
    dG = (X * torch.exp(torch.empty(1, N, device=dev, dtype=torch.float64).uniform_(-0.5, 0.5, generator=g))).float()
    return Ql, Qr, dX, dG


def _update_errors(Ql, Qr, dX, dG, got):
    """[(factor error, increment error)] of the two updated factors against fp64; increments against the balanced factors."""
    ref = ref64.update_precond_dense_dense(Ql.double(), Qr.double(), dX.double(), dG.double(), STEP, TINY)
    rho = torch.sqrt(torch.max(torch.diagonal(Ql.double())) / torch.max(torch.diagonal(Qr.double())))
    bases = (Ql.double() / rho, Qr.double() * rho)
    return [(rel(g_, r_), rel(g_.double() - q0, r_ - q0)) for g_, r_, q0 in zip(got, ref, bases)], ref, bases


def _assert_factors_are_triangular(got):
    for q in got:
        assert torch.equal(q, torch.triu(q)), "entries below the diagonal"
        assert bool((torch.diagonal(q) > 0).all()), "diagonal not positive"


def _tiles(t):
    """(interior, ragged corner) 128 x 128 output tiles of t: the second tile of the diagonal where there is one, and the last tile."""
    rows, cols = t.shape
    i = 128 if rows > 256 and cols > 256 else 0
    return (slice(i, i + 128), slice(i, i + 128)), (slice((rows - 1) // 128 * 128, rows), slice((cols - 1) // 128 * 128, cols))


def _assert_tile_loss_fails(t, *checks):
    """A result with one 128 x 128 tile lost (zeroed) must fail every bar: an interior tile and the ragged corner tile."""
    for tile in _tiles(t):
        bad = t.clone()
        bad[tile] = 0
        assert not torch.equal(bad, t)
        for err, bar in checks:
            assert err(bad) >= bar, (tile, err(bad), bar)


def test_route_table_straddles_its_thresholds(hip_lib):
    """Each boundary pair of the table lies on the two sides of the flag it names (in both orientations), and every shape of a
    pair is in the table.  A threshold that moves fails here, naming the pair."""
    shapes = {(M, N) for M, N, _, _ in ENTRIES}
    for without, with_, bit in PAIRS:
        for a, b in ((without, with_), (without[::-1], with_[::-1])):
            assert a in shapes and b in shapes, (a, b)
            fa, fb = _flags(*a), _flags(*b)
            assert fa >= 0 and fb >= 0
            assert not fa & bit and fb & bit, ("pair no longer straddles its threshold", a, b, hex(bit), hex(fa), hex(fb))
    tiers = [_chunks(_flags(M, N)) for M, N in CHUNK_TIERS]
    assert all(_flags(M, N) & F.KRON_ROUTE_GRAD_RECT for M, N in CHUNK_TIERS)
    assert tiers == sorted(set(tiers)) and len(tiers) == 4, tiers
    for a, b in APPLY_SPLIT_PAIRS:
        assert a in shapes and b in shapes
    # the families the entries claim: the inverse tiers and the stream order are on the inverse route where the pairs say so
    for M, N, _, fam in ENTRIES:
        f = _flags(M, N)
        if "ill" in fam and f & F.KRON_ROUTE_INV_SOLVES:
            assert f & F.KRON_ROUTE_BF16_INV, (M, N)


@pytest.mark.parametrize("M,N,fam", _cases(lambda fam: "upd" in fam))
def test_fp32_update_balanced(psgd_mod, M, N, fam):
    """(a) The fp32 update on balanced data against fp64: factors 1e-5, increments 2e-3, triangular with a positive diagonal."""
    Ql, Qr, dX, dG, _ = _balanced(M, N)
    got = psgd_mod.update_precond_kron(Ql, Qr, dX, dG, STEP)
    errs, ref, bases = _update_errors(Ql, Qr, dX, dG, got)
    for i, (e_fac, e_inc) in enumerate(errs):
        assert e_fac < TOL and e_inc < INCR_TOL, (i, errs, hex(_flags(M, N)))
    _assert_factors_are_triangular(got)
    if "teeth" in fam:
        for g_, r_, q0 in zip(got, ref, bases):
            _assert_tile_loss_fails(g_, (lambda t: rel(t, r_), TOL), (lambda t: rel(t.double() - q0, r_ - q0), INCR_TOL))


@pytest.mark.parametrize("M,N,fam", _cases(lambda fam: "ill" in fam))
def test_fp32_update_ill_conditioned(psgd_mod, M, N, fam):
    """(b) The fp32 update with cond(Q) ~ 1e4 factors near the fixed point (the solves carry the conditioning): the same bars."""
    Ql, Qr, dX, dG = _illcond(M, N)
    got = psgd_mod.update_precond_kron(Ql, Qr, dX, dG, STEP)
    errs, _, _ = _update_errors(Ql, Qr, dX, dG, got)
    for i, (e_fac, e_inc) in enumerate(errs):
        assert e_fac < TOL and e_inc < INCR_TOL, (i, errs, hex(_flags(M, N)))
    _assert_factors_are_triangular(got)


@pytest.mark.parametrize("M,N,fam", _cases(lambda fam: "ill" in fam))
def test_bf16_update(psgd_mod, M, N, fam):
    """(c) The bf16-operand update (fp32 solves, on the inverse route where the flag says so) against fp64 on the bf16-rounded data:
    increments 2e-2, factors BF16_UPD_STATE_TOL."""
    Ql, Qr, dX, dG, _ = _balanced(M, N)
    dXb, dGb = dX.to(torch.bfloat16), dG.to(torch.bfloat16)
    got = psgd_mod.update_precond_kron(Ql, Qr, dXb, dGb, STEP)
    assert all(q.dtype == torch.float32 for q in got)
    errs, _, _ = _update_errors(Ql, Qr, dXb, dGb, got)
    for i, (e_fac, e_inc) in enumerate(errs):
        assert e_fac < BF16_UPD_STATE_TOL and e_inc < BF16_TOL, (i, errs, hex(_flags(M, N)))
    _assert_factors_are_triangular(got)


@pytest.mark.parametrize("M,N,fam", _cases(lambda fam: True))
def test_fp32_apply_routes(psgd_mod, M, N, fam):
    """(d) The fp32 apply on the default reference route, then on the opt-in "auto" route: the Gram-free direct chain on first
    sight (where it is a path of its own), prepare + apply, prepared -- every call within 1e-5 of fp64."""
    from psgd_tf_amd import kron
    Ql, Qr, _, _, G = _balanced(M, N)
    ref = ref64.precond_grad_dense_dense(Ql.double(), Qr.double(), G.double())
    assert kron._apply_route == "reference"
    out = psgd_mod.precond_grad_kron(Ql, Qr, G)
    assert rel(out, ref) < TOL, (rel(out, ref), hex(_flags(M, N)))
    if "teeth" in fam:
        _assert_tile_loss_fails(out, (lambda t: rel(t, ref), TOL))
    key = (G.get_device(), M, N, kron._raw_stream(G.get_device()))
    direct = bool(_flags(M, N) & F.KRON_ROUTE_APPLY_DIRECT)
    Ql, Qr = Ql.clone(), Qr.clone()                        # (new factor tensors: first sight)
    old = kron.set_apply_route("auto")
    try:
        paths = []
        for _ in range(3):
            out = psgd_mod.precond_grad_kron(Ql, Qr, G)
            paths.append(kron._apply_slots[key].path)
            assert rel(out, ref) < TOL, (paths, rel(out, ref))
        assert paths == (["direct", "both", "prepared"] if direct else ["both", "prepared", "prepared"]), paths
    finally:
        kron.set_apply_route(old)


@pytest.mark.parametrize("M,N,fam", _cases(lambda fam: "upd" in fam))
def test_bf16_apply(psgd_mod, M, N, fam):
    """(e) The bf16 apply (bf16 gradient, fp32 factors) within 2e-2 of fp64 on the same bf16 values."""
    Ql, Qr, _, _, G = _balanced(M, N)
    Gb = G.to(torch.bfloat16)
    out = psgd_mod.precond_grad_kron(Ql, Qr, Gb)
    e = rel(out, ref64.precond_grad_dense_dense(Ql.double(), Qr.double(), Gb.double()))
    assert e < BF16_TOL, (e, hex(_flags(M, N)))


@pytest.mark.parametrize("M,N,fam", _cases(lambda fam: "mag" in fam))
def test_fp32_data_magnitudes(psgd_mod, M, N, fam):
    """(f) G and dX x 1e+-12, dG / the same factor (the plane formats carry their own scales): apply and update at the fp32 bars."""
    Ql, Qr, dX, dG, G = _balanced(M, N)
    s = 1e12 if M < N else 1e-12
    G, dX, dG = G * s, dX * s, dG / s
    out = psgd_mod.precond_grad_kron(Ql, Qr, G)
    e = rel(out, ref64.precond_grad_dense_dense(Ql.double(), Qr.double(), G.double()))
    assert e < TOL, (s, e)
    got = psgd_mod.update_precond_kron(Ql, Qr, dX, dG, STEP)
    errs, _, _ = _update_errors(Ql, Qr, dX, dG, got)
    for i, (e_fac, e_inc) in enumerate(errs):
        assert e_fac < TOL and e_inc < INCR_TOL, (s, i, errs)


@pytest.fixture(autouse=True)
def _release_cached_blocks():
    """Hand the blocks torch's caching allocator keeps back to the device after every case: the table sweeps ~90 large shapes, and
    the fp64 solves of the reference allocate their library workspace outside that allocator."""
    yield
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def psgd_mod(hip_lib):
    import preconditioned_stochastic_gradient_descent as m
    return m
