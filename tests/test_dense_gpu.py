"""Dense preconditioner on the GPU (psgd_dense.hip via update_precond_dense / precond_grad_dense) against the fp64 oracle."""
import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from tests.uvd_cases import rel_err

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 31, 64, 65, 66, 68, 127, 128, 129, 192, 255, 256, 257, 400, 1000, 1021, 1023, 1024, 1025, 1028, 4096)


@pytest.fixture
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    m.set_dense_route("native")
    yield m
    m.set_dense_route("native")


def _upper(rng, n):
    """The identity advanced by a few updates: unit-scale diagonal (0.2 .. 5) and a small strictly upper part; condition <= ~1e2."""
    d = np.exp(rng.uniform(np.log(0.2), np.log(5.0), n))
    return np.triu(rng.standard_normal((n, n)) * (0.3 / np.sqrt(n)), 1) + np.diag(d)


def _problem(n, dense, seed):
    rng = np.random.default_rng(seed)
    Q = _upper(rng, n)
    if dense:
        Q = Q + np.tril(rng.standard_normal((n, n)) * (0.3 / np.sqrt(n)), -1)
    dx, dg, g = (rng.standard_normal(n) for _ in range(3))
    return [a.astype(np.float32) for a in (Q, dx, dg, g)]


def _dev(*arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


@pytest.mark.parametrize("dense", [False, True], ids=["upper", "dense"])
@pytest.mark.parametrize("n", SIZES)
def test_update_and_apply_match_fp64(psgd, n, dense):
    Q, dx, dg, g = _problem(n, dense, seed=n + 7 * dense)
    tQ, tdx, tdg, tg = _dev(Q, dx, dg, g)
    Qn = psgd.update_precond_dense(tQ, [tdx], [tdg], step=0.01)
    pg = psgd.precond_grad_dense(tQ, [tg])[0]
    Q64 = Q.astype(np.float64)
    ref = orc.update_precond_dense(Q64, [dx.astype(np.float64)], [dg.astype(np.float64)], step=0.01)
    ref_pg = orc.precond_grad_dense(Q64, [g.astype(np.float64)])[0]
    got = Qn.cpu().numpy()
    assert rel_err(got, ref) < 1e-5
    assert rel_err(got.astype(np.float64) - Q64, ref - Q64) < 2e-3
    assert rel_err(pg.cpu().numpy(), ref_pg) < 1e-5
    if not dense:
        assert not np.tril(got, -1).any()                      # an upper-triangular Q stays upper-triangular, exactly


def _unaligned(t):
    """t as a contiguous view 1 .. 3 floats into a larger buffer: its address is not a multiple of 16 bytes"""
    n = t.numel()
    for off in (1, 2, 3):
        v = torch.zeros(n + 4, device=t.device, dtype=t.dtype)[off:off + n].view(t.shape)
        if v.data_ptr() % 16:
            v.copy_(t)
            return v
    raise AssertionError("no unaligned view")


@pytest.mark.parametrize("dense", [False, True], ids=["upper", "dense"])
@pytest.mark.parametrize("n", [68, 256, 1024])
def test_unaligned_q_view(psgd, n, dense):
    """N % 4 == 0 with Q at an address that is not 16-byte aligned: the scalar instantiations (update_large<1>, apply_large<1>) at
    sizes that otherwise only see the float4 ones.  Same fp64 bars as the aligned call, equal to it within 1e-5, bit-identical on
    repeat."""
    Q, dx, dg, g = _problem(n, dense, seed=n + 13 * dense)
    tQ, tdx, tdg, tg = _dev(Q, dx, dg, g)
    vQ = _unaligned(tQ)
    assert vQ.is_contiguous() and vQ.data_ptr() % 16 != 0 and tQ.data_ptr() % 16 == 0 and torch.equal(vQ, tQ)
    Qa, pa = psgd.update_precond_dense(tQ, [tdx], [tdg], step=0.01), psgd.precond_grad_dense(tQ, [tg])[0]
    Qu, pu = psgd.update_precond_dense(vQ, [tdx], [tdg], step=0.01), psgd.precond_grad_dense(vQ, [tg])[0]
    assert torch.equal(vQ, tQ)                                    # the view is not modified
    assert torch.equal(Qu, psgd.update_precond_dense(vQ, [tdx], [tdg], step=0.01))
    assert torch.equal(pu, psgd.precond_grad_dense(vQ, [tg])[0])
    Q64 = Q.astype(np.float64)
    ref = orc.update_precond_dense(Q64, [dx.astype(np.float64)], [dg.astype(np.float64)], step=0.01)
    ref_pg = orc.precond_grad_dense(Q64, [g.astype(np.float64)])[0]
    for got, pg in ((Qu, pu), (Qa, pa)):
        got = got.cpu().numpy()
        assert rel_err(got, ref) < 1e-5
        assert rel_err(got.astype(np.float64) - Q64, ref - Q64) < 2e-3
        assert rel_err(pg.cpu().numpy(), ref_pg) < 1e-5
        if not dense:
            assert not np.tril(got, -1).any()
    assert rel_err(Qu.cpu().numpy(), Qa.cpu().numpy()) < 1e-5
    assert rel_err(pu.cpu().numpy(), pa.cpu().numpy()) < 1e-5


def _solve_direction(Q64, Qn, step):
    """With dg = 0 the update is Q_new - Q = mu triu(b b') Q with mu = step / (max_i b_i^2 + tiny): T = (Q_new - Q) Q^-1 (fp64) holds
    mu b_i b_j at [i, j], j >= i.  Through the row and column of p = argmax T[i, i]: u_j = mu b_p b_j / sqrt(mu b_p^2) =
    sqrt(step) b_j / max|b| up to the sign of b_p -- the solve's b up to the scale the update normalises away.  Q^-1 amplifies the
    rounding of Q_new; the diagonal of an upper-triangular Q needs no inverse: (Q_new - Q)[i, i] / (step Q[i, i]) = (b_i / max|b|)^2.
    Returns (u / sqrt(step), p, those squares)."""
    D = Qn.astype(np.float64) - Q64
    T = np.linalg.solve(Q64.T, D.T).T
    p = int(np.argmax(np.diag(T)))
    u = np.concatenate([T[:p, p], T[p, p:]]) / np.sqrt(T[p, p])
    return u / np.sqrt(step), p, np.diag(D) / (step * np.diag(Q64))


@pytest.mark.parametrize("n", [129, 1000])
def test_blocked_solve_residual_on_a_less_benign_q(psgd, n):
    """The blocked solve through explicit 64 x 64 block inverses on the least benign Q of the randomised sweep's domain (diagonal
    exp(U(-1.6, 1.6)), strictly upper part 2 / sqrt(N): condition ~1e3 .. 1e5).  b = Q^-T dx is read back out of an update with
    dg = 0 (_solve_direction; the step is free here and any value is a valid call: step = 1, against the 0.01 / 0.1 of the other
    tests, makes the increment largest against the rounding of Q_new, which both routes share) and compared with the fp64 solve,
    both normalised to max|b| = 1, and so are the squares (b_i / max|b|)^2 off the diagonal, which carry less of Q_new's rounding.  Bar
    for each: twice the error of the torch-op route (torch's fp32 triangular solve) read back the same way, plus 1e-5."""
    rng = np.random.default_rng(100 + n)
    Q = (np.triu(rng.standard_normal((n, n)) * (2.0 / np.sqrt(n)), 1) + np.diag(np.exp(rng.uniform(-1.6, 1.6, n)))).astype(np.float32)
    dx = rng.standard_normal(n).astype(np.float32)
    Q64 = Q.astype(np.float64)
    b64 = np.linalg.solve(Q64.T, dx.astype(np.float64))
    tQ, tdx = _dev(Q, dx)
    zero = torch.zeros(n, device="cuda")
    err, err2 = {}, {}
    for route in ("native", "torch"):
        psgd.set_dense_route(route)
        Qn = psgd.update_precond_dense(tQ, [tdx], [zero], step=1.0).cpu().numpy()
        b, p, sq = _solve_direction(Q64, Qn, 1.0)
        want = b64 / np.max(np.abs(b64)) * np.sign(b64[p])
        assert abs(b64[p]) == np.max(np.abs(b64))                # the pivot is the largest entry of the true solution
        err[route] = rel_err(b, want)
        err2[route] = rel_err(sq, want * want)
    psgd.set_dense_route("native")
    print("solve n=%d cond %.1e: b native %.2e torch %.2e, b^2 native %.2e torch %.2e"
          % (n, np.linalg.cond(Q64), err["native"], err["torch"], err2["native"], err2["torch"]))
    assert err["native"] <= 2 * err["torch"] + 1e-5, err
    assert err2["native"] <= 2 * err2["torch"] + 1e-5, err2


def test_kat_r_rosenbrock_first_step(psgd):
    """hello_psgd.py's first step with v = (1, 0): g = (-4, 0), Hv = (802, 400) (tests/test_oracle_kat.py on the GPU)."""
    Q = 0.1 * torch.eye(2, device="cuda")
    f = lambda v: torch.tensor(v, dtype=torch.float32, device="cuda")
    Qn = psgd.update_precond_dense(Q, [f(1.0), f(0.0)], [f(802.0), f(400.0)], step=0.2)
    assert np.allclose(Qn.cpu().numpy(), [[0.08, -0.0101326], [0.0, 0.09494634]], rtol=2e-6, atol=1e-9)
    pg = psgd.precond_grad_dense(Qn, [f(-4.0), f(0.0)])
    assert pg[0].shape == () and pg[1].shape == ()
    assert np.allclose([float(pg[0]), float(pg[1])], [-0.0256, 0.00324243], rtol=2e-6)


@pytest.mark.parametrize("n", [3, 129])
def test_zero_curvature_leaves_q(psgd, n):
    """dx = dg = 0: max|G| = 0, mu = step / tiny (finite in fp32), G = 0, so Q' == Q."""
    Q, _, _, _ = _problem(n, True, seed=3)
    tQ = _dev(Q)[0]
    z = torch.zeros(n, device="cuda")
    Qn = psgd.update_precond_dense(tQ, [z], [z], step=0.01)
    assert torch.equal(Qn, tQ)


@pytest.mark.parametrize("n", [5, 300])
def test_nan_propagates(psgd, n):
    Q, dx, dg, _ = _problem(n, False, seed=4)
    dg[n // 2] = np.nan
    Qn = psgd.update_precond_dense(*_dev(Q), [_dev(dx)[0]], [_dev(dg)[0]]).cpu().numpy()
    with np.errstate(invalid="ignore"):
        ref = orc.update_precond_dense(Q.astype(np.float64), [dx.astype(np.float64)], [dg.astype(np.float64)])
    assert np.array_equal(np.isnan(Qn), np.isnan(ref)) and np.isnan(Qn).all()


@pytest.mark.parametrize("n_parts", [(3, (4, 5), (2, 3, 2)), ((7, 9), (33,), (2, 2, 2, 2), (5,))])
def test_lists_of_tensors_and_strided_inputs(psgd, n_parts):
    rng = np.random.default_rng(5)
    shapes = [s if isinstance(s, tuple) else (s,) for s in n_parts]
    n = sum(int(np.prod(s)) for s in shapes)
    Q = _upper(rng, n).astype(np.float32)
    dxs = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    dgs = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    gs = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    # strided views: Q as the transpose of a transposed copy, every vector a stride-2 slice of a larger tensor
    tQ = torch.from_numpy(np.ascontiguousarray(Q.T)).cuda().t()
    strided = lambda a: torch.from_numpy(np.repeat(a[..., None], 2, axis=-1)).cuda()[..., 0]
    tdx, tdg, tg = [strided(a) for a in dxs], [strided(a) for a in dgs], [strided(a) for a in gs]
    assert not tQ.is_contiguous() and not tdx[0].is_contiguous()
    before = [t.clone() for t in [tQ] + tdx + tdg + tg]
    Qn = psgd.update_precond_dense(tQ, tdx, tdg, step=0.05)
    pgs = psgd.precond_grad_dense(Qn, tg)
    for a, b in zip(before, [tQ] + tdx + tdg + tg):
        assert torch.equal(a, b)                                # inputs are not modified
    f64 = lambda xs: [x.astype(np.float64) for x in xs]
    ref = orc.update_precond_dense(Q.astype(np.float64), f64(dxs), f64(dgs), step=0.05)
    assert rel_err(Qn.cpu().numpy(), ref) < 1e-5
    refs = orc.precond_grad_dense(Qn.cpu().numpy().astype(np.float64), f64(gs))
    assert [tuple(p.shape) for p in pgs] == [tuple(s) for s in shapes]
    for p, r in zip(pgs, refs):
        assert rel_err(p.cpu().numpy(), r) < 1e-5


def test_shape_errors_name_the_function(psgd):
    Q = torch.eye(4, device="cuda")
    with pytest.raises(ValueError, match="update_precond_dense"):
        psgd.update_precond_dense(torch.zeros(4, 5, device="cuda"), [torch.zeros(4, device="cuda")], [torch.zeros(4, device="cuda")])
    with pytest.raises(ValueError, match="update_precond_dense"):
        psgd.update_precond_dense(Q, [torch.zeros(5, device="cuda")], [torch.zeros(5, device="cuda")])
    with pytest.raises(ValueError, match="precond_grad_dense"):
        psgd.precond_grad_dense(Q, [torch.zeros(3, device="cuda")])


@pytest.mark.parametrize("n", [40, 1000])
def test_side_stream(psgd, n):
    Q, dx, dg, g = _problem(n, True, seed=6)
    tQ, tdx, tdg, tg = _dev(Q, dx, dg, g)
    ref_q = psgd.update_precond_dense(tQ, [tdx], [tdg])
    ref_g = psgd.precond_grad_dense(tQ, [tg])[0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        q2 = psgd.update_precond_dense(tQ, [tdx], [tdg])
        g2 = psgd.precond_grad_dense(tQ, [tg])[0]
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(q2, ref_q) and torch.equal(g2, ref_g)


@pytest.mark.parametrize("n", [64, 1021, 4096])
def test_bit_identical_repeats(psgd, n):
    Q, dx, dg, g = _problem(n, True, seed=8)
    tQ, tdx, tdg, tg = _dev(Q, dx, dg, g)
    a = psgd.update_precond_dense(tQ, [tdx], [tdg])
    b = psgd.update_precond_dense(tQ, [tdx], [tdg])
    assert torch.equal(a, b)
    assert torch.equal(psgd.precond_grad_dense(tQ, [tg])[0], psgd.precond_grad_dense(tQ, [tg])[0])


@pytest.mark.parametrize("n", [17, 400, 1021])
def test_first_call_on_poisoned_memory(psgd, monkeypatch, n):
    """Workspaces filled with 0xFF bytes and outputs with NaN when created: the first call equals the second, bit for bit."""
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as core
    orig = torch.empty
    made = []

    def empty(*a, **k):
        t = orig(*a, **k)
        if t.is_cuda and t.numel():
            t.fill_(0xFF if t.dtype == torch.uint8 else float("nan"))
            made.append(t.dtype)
        return t
    monkeypatch.setattr(torch, "empty", empty)
    Q, dx, dg, g = _problem(n, True, seed=9)
    tQ, tdx, tdg, tg = _dev(Q, dx, dg, g)
    core._ws_cache._d.clear()
    first = psgd.update_precond_dense(tQ, [tdx], [tdg]).clone()
    assert torch.uint8 in made and torch.float32 in made
    second = psgd.update_precond_dense(tQ, [tdx], [tdg])
    assert torch.isfinite(first).all() and torch.equal(first, second)
    core._ws_cache._d.clear()
    first = psgd.precond_grad_dense(tQ, [tg])[0].clone()
    second = psgd.precond_grad_dense(tQ, [tg])[0]
    assert torch.isfinite(first).all() and torch.equal(first, second)
    monkeypatch.undo()
    core._ws_cache._d.clear()


def test_large_n_diagonal_64bit_indexing(psgd):
    """N = 46 400: N^2 > 2^31.  Diagonal Q = diag(q): a = q dg, b = dx / q, Q'[i, j] = [i == j] q_i - mu (a_i a_j - b_i b_j) q_j
    for j >= i and 0 below; the apply is q^2 g.  Sampled rows (the last ones included) against this closed form in fp64."""
    n = 46400
    rng = np.random.default_rng(10)
    q = np.exp(rng.uniform(-0.5, 0.5, n)).astype(np.float32)
    dx, dg, g = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    tQ = torch.zeros((n, n), device="cuda")
    tQ.diagonal().copy_(torch.from_numpy(q))
    tdx, tdg, tg = _dev(dx, dg, g)
    Qn = psgd.update_precond_dense(tQ, [tdx], [tdg], step=0.01)
    pg = psgd.precond_grad_dense(tQ, [tg])[0].cpu().numpy()
    q64, dx64, dg64 = (v.astype(np.float64) for v in (q, dx, dg))
    a, b = q64 * dg64, dx64 / q64
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = 0.0
    for i0 in range(0, n, 2048):                                 # max over i <= j of |a_i a_j - b_i b_j|, fp64 on the device
        i1 = min(n, i0 + 2048)
        blk = (ta[i0:i1, None] * ta[None, i0:] - tb[i0:i1, None] * tb[None, i0:]).abs()
        blk = torch.triu(blk)                                    # column offset i0: keeps j >= i
        m = max(m, float(blk.max()))
        del blk
    mu = 0.01 / (m + np.finfo(np.float32).tiny)
    for i in (0, 1, 63, 64, 12345, 32767, 46336, n - 2, n - 1):
        row = Qn[i].cpu().numpy().astype(np.float64)
        exp = np.zeros(n)
        exp[i:] = -mu * (a[i] * a[i:] - b[i] * b[i:]) * q64[i:]
        exp[i] += q64[i]
        assert rel_err(row, exp) < 1e-5, i
        assert not row[:i].any()
    assert rel_err(pg, q64 * q64 * g.astype(np.float64)) < 1e-6
    del Qn, tQ
    torch.cuda.empty_cache()


def test_native_route_taken(psgd, monkeypatch):
    """fp32 on the device never reaches torch's solve or matmul; set_dense_route("torch") does."""
    class Reached(Exception):
        pass

    def boom(*a, **k):
        raise Reached()
    Q, dx, dg, g = _problem(200, False, seed=11)
    tQ, tdx, tdg, tg = _dev(Q, dx, dg, g)
    monkeypatch.setattr(torch.linalg, "solve_triangular", boom)
    monkeypatch.setattr(torch.Tensor, "__matmul__", boom)
    Qn = psgd.update_precond_dense(tQ, [tdx], [tdg])
    psgd.precond_grad_dense(Qn, [tg])
    psgd.set_dense_route("torch")
    with pytest.raises(Reached):
        psgd.update_precond_dense(tQ, [tdx], [tdg])
    with pytest.raises(Reached):
        psgd.precond_grad_dense(tQ, [tg])


def test_tensor_decomposition_example_tracks_fp64(psgd):
    """examples/tensor_decomposition_dense.py (N = 400) for 200 iterations on the GPU against the same loop on the CPU in fp64 through
    the oracle.  Thresholds from the oracle runs of seeds 0-2: the loss falls from ~5e4 to ~810-817 (a rank-5 fit of a uniform tensor
    cannot go much lower), and an fp32 CPU run of the torch route ends within 1e-6 of the oracle's loss.  The native run must end
    within 1 % of the oracle's final loss and stay within 5 % of its curve at iterations 10, 50 and 100."""
    from examples.tensor_decomposition_dense import run

    def upd(Q, dxs, dgs, step):
        return torch.from_numpy(orc.update_precond_dense(Q.numpy(), [x.numpy() for x in dxs], [x.numpy() for x in dgs], step))

    def app(Q, gs):
        return [torch.from_numpy(np.asarray(p)) for p in orc.precond_grad_dense(Q.numpy(), [x.numpy() for x in gs])]
    ref, _ = run(200, 0, "cpu", torch.float64, upd, app)
    got, Q = run(200, 0, "cuda", torch.float32)
    assert Q.is_cuda and Q.shape == (400, 400)
    assert got[-1] < 0.05 * got[0]
    assert abs(got[-1] - ref[-1]) <= 0.01 * ref[-1], (got[-1], ref[-1])
    for i in (10, 50, 100):
        assert abs(got[i] - ref[i]) <= 0.05 * ref[i], (i, got[i], ref[i])
