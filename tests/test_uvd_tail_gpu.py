"""GPU: the step tail of class UVd in HIP (psgd_uvd_tail.hip) -- uvd_pack, the sum of squares of the clip norm, uvd_step_tail and
UVd(step_tail="fused") -- against the torch expressions of the default tail, which are copied here as the reference.
The last two sections: special values (signed zeros, infinities, NaN, the ends of the normal range, subnormals) through every
kernel, where the bar is "the torch tail's bits wherever it is not NaN, and its NaN mask"; and tensor lists long enough for the
second trip of the three grid-stride loops."""
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SIZES_SMALL = [1, 3, 7, 0, 4099, 70_001]


def _sizes_many():
    s = np.random.default_rng(11).integers(0, 2001, 300).tolist()
    s[5], s[6] = 0, 2000
    return s


SIZE_LISTS = {"six": SIZES_SMALL, "many": _sizes_many()}


@pytest.fixture
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _tensors(sizes, dtype, seed, scale=1.0):
    """one tensor per size; every third one is a view that starts one element into its allocation (pointer aligned to the element
    only: 4 bytes for fp32, 2 for the half types), every fifth of the longer ones is two-dimensional"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for k, n in enumerate(sizes):
        if k % 3 == 1:
            t = (torch.randn(n + 1, device="cuda", generator=g) * scale).to(dtype)[1:]
        else:
            t = (torch.randn(n, device="cuda", generator=g) * scale).to(dtype)
        if k % 5 == 0 and n % 2 == 0 and n > 0:
            t = t.view(2, n // 2)
        assert t.is_contiguous() and t.numel() == n
        out.append(t)
    assert any(t.data_ptr() % 16 for t in out if t.numel())
    return out


# ----------------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", list(SIZE_LISTS))
def test_pack_equals_cat(psgd, which, dtype):
    """bit-equal to torch.cat([...]).float() * scale: a power-of-two scale is exact, so equality is the bar"""
    sizes = SIZE_LISTS[which]
    ts = _tensors(sizes, dtype, seed=3)
    total = sum(sizes)
    for scale in (1.0, 2.0 ** -12):
        ref = torch.cat([t.reshape(-1) for t in ts]).float() * scale
        for shift in (0, 1):                                   # the flat vector on a 16-byte boundary, and one element past it
            buf = torch.full((total + 8,), float("nan"), device="cuda")
            got = psgd.uvd_pack(ts, buf[shift:shift + total], scale)
            assert got.shape == (total,) and got.data_ptr() == buf.data_ptr() + 4 * shift
            assert torch.equal(_bits(got), _bits(ref)), (which, dtype, scale, shift)
            assert torch.isnan(buf[:shift]).all() and torch.isnan(buf[shift + total:]).all()    # nothing outside the vector


def test_pack_rejects_what_it_cannot_take(psgd):
    a = torch.randn(4, 6, device="cuda")
    out = torch.empty(100, device="cuda")
    with pytest.raises(ValueError):
        psgd.uvd_pack([a.t()], out)                                   # strided
    with pytest.raises(ValueError):
        psgd.uvd_pack([a, a.bfloat16()], out)                          # two dtypes
    with pytest.raises(ValueError):
        psgd.uvd_pack([a], out[:10])                                   # out too short
    with pytest.raises(TypeError):
        psgd.uvd_pack([a], out.double())


# ------------------------------------------------------------------------------------------------------------- sum of squares
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097, 1_000_003])
def test_sumsq(psgd, N):
    """Reference, exactly: every product x_i * x_i rounded to fp32 (numpy float32 multiply, what the kernel's per-lane product is),
    then the fp32 products summed in fp64 by numpy.  The kernel sums the same fp32 products in fp64 in another (fixed) order; with
    non-negative terms the two differ by at most a few N * 2^-53 relative, far inside 1e-12."""
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import UVdTailPlan, uvd_sumsq
    x = torch.randn(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N)) * 3.0
    plan = UVdTailPlan([N], torch.float32, x.device)
    plan.ws.fill_(0xFF)
    plan.sumsq.fill_(float("nan"))
    first = uvd_sumsq(x, plan=plan).clone()
    second = uvd_sumsq(x, plan=plan).clone()
    xs = x.cpu().numpy()
    ref = np.sum((xs * xs).astype(np.float64))
    assert (xs * xs).dtype == np.float32
    got = float(first.item())
    print("sumsq N=%d: got %.17g ref %.17g rel %.3g" % (N, got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-12 * ref
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))


# --------------------------------------------------------------------------------------------------- update without clipping
def _torch_tail(params, pre_grad, lr, vs):
    """the loop of UVd.step (the torch tail), with its index arithmetic: the reference of the parameter update"""
    sizes = [int(p.numel()) for p in params]
    cums = np.cumsum(sizes).tolist()
    for k, (p, i, j) in enumerate(zip(params, sizes, cums)):
        delta = (lr * torch.reshape(pre_grad[j - i:j], p.shape)).to(p.dtype)
        if vs is not None:
            delta = delta + vs[k]
        p.sub_(delta)


@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", list(SIZE_LISTS))
def test_update_without_clipping_is_bit_identical(psgd, which, dtype, with_vs):
    sizes = SIZE_LISTS[which]
    ref = _tensors(sizes, dtype, seed=5)
    got = [t.clone() for t in ref]
    got = [(torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape) if k % 3 == 1 else t) for k, t in enumerate(got)]
    vs = _tensors(sizes, dtype, seed=6, scale=0.05) if with_vs else None
    pre = torch.randn(sum(sizes), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    for lr in (0.01, 0.37):
        _torch_tail(ref, pre, lr, vs)
        psgd.uvd_step_tail(got, pre, lr, vs=vs)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(_bits(a), _bits(b)), (which, dtype, with_vs, lr, k, sizes[k])
    # max_norm = inf is "no clipping" too (the class passes its hyper-parameter as it is)
    _torch_tail(ref, pre, 0.01, vs)
    psgd.uvd_step_tail(got, pre, 0.01, max_norm=math.inf, vs=vs)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, ref))


@pytest.mark.parametrize("dtype", DTYPES)
def test_perturbation_is_p_add_v(psgd, dtype):
    """pre_grad=None: the p.add_(v) loop of the finite-difference branch, bit for bit"""
    sizes = SIZE_LISTS["many"]
    ref = _tensors(sizes, dtype, seed=8)
    got = [t.clone() for t in ref]
    vs = _tensors(sizes, dtype, seed=9, scale=2.0 ** -6)
    for p, v in zip(ref, vs):
        p.add_(v)
    psgd.uvd_step_tail(got, None, 0.0, vs=vs)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, ref))
    with pytest.raises(ValueError):
        psgd.uvd_step_tail(got, None, 0.0)


# ------------------------------------------------------------------------------------------------------ update with clipping
def _spacing(x64, dtype):
    """distance between neighbouring `dtype` numbers around |x| (normal range)"""
    bits = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}[dtype]
    tiny = float(torch.finfo(dtype).tiny)
    e = np.floor(np.log2(np.maximum(np.abs(x64), tiny)))
    return 2.0 ** (e - bits)


def _inside_clip_bound(p_new, ref64, delta64, dtype):
    """The bound of the clipped update.  lr_eff is ONE fp32 rounding of the exact product, so fl32(lr_eff g) is within 2 * 2^-24 |delta|
    of the fp64 delta and the difference p - delta adds half an ulp of p: fp32 parameters must sit within 2 ulp of p plus
    4 * 2^-24 |delta| of the fp64 reference; half-precision parameters must be the correctly rounded reference or its neighbour,
    and the neighbour in at most 1 % of the elements."""
    got = p_new.double().cpu().numpy()
    if dtype == torch.float32:
        bound = 2 * _spacing(ref64, dtype) + 4 * 2.0 ** -24 * np.abs(delta64)
        return bool((np.abs(got - ref64) <= bound).all()), 0.0
    ref_t = torch.from_numpy(ref64).to(dtype).double().numpy()
    diff = np.abs(got - ref_t)
    ok = bool((diff <= _spacing(ref_t, dtype) * 1.0000001).all())
    return ok, float((diff > 0).mean())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("below", [True, False])
def test_update_with_clipping(psgd, dtype, below):
    sizes = SIZES_SMALL + [257, 12_345]
    rng = np.random.default_rng(21)                          # host-side draws: the same numbers wherever the test runs
    host = [torch.from_numpy(rng.standard_normal(n + 1).astype(np.float32)).to(dtype) for n in sizes]
    params = [h.cuda()[1:] if k % 3 == 1 else h[1:].cuda() for k, h in enumerate(host)]
    pre_host = torch.from_numpy((rng.standard_normal(sum(sizes)) * 0.7).astype(np.float32))
    pre = pre_host.cuda()
    lr, tiny = 0.05, float(torch.finfo(dtype).tiny)
    g64 = pre_host.double().numpy()
    norm = math.sqrt(float(np.sum(g64 * g64)))
    max_norm = 0.25 * norm if below else 3.0 * norm
    lr_eff = float(np.float32(lr)) * min(max_norm / (norm + tiny), 1.0)                 # the formula in fp64
    assert (lr_eff < 0.3 * lr) if below else (lr_eff == float(np.float32(lr)))
    p64 = torch.cat([h[1:] for h in host]).double().numpy()
    delta64 = lr_eff * g64
    if dtype != torch.float32:
        delta64 = torch.from_numpy(delta64).to(dtype).double().numpy()                   # delta is rounded to the parameters' type first
    ref64 = p64 - delta64

    # the bound holds for the torch tail itself (CPU tensors, the expressions of UVd.step): it is not tighter than the path it replaces
    cpu_params = [h[1:].clone() for h in host]
    cpu_pre = pre_host
    grad_norm = torch.sqrt(torch.sum(cpu_pre * cpu_pre)) + tiny
    _torch_tail(cpu_params, cpu_pre, lr * torch.clamp(max_norm / grad_norm, max=1.0), None)
    ok, frac = _inside_clip_bound(torch.cat([p.reshape(-1) for p in cpu_params]), ref64, delta64, dtype)
    print("torch tail on the CPU: inside %s, neighbour fraction %.4g" % (ok, frac))
    assert ok and frac <= 0.01

    psgd.uvd_step_tail(params, pre, lr, max_norm=max_norm, tiny=tiny)
    ok, frac = _inside_clip_bound(torch.cat([p.reshape(-1) for p in params]), ref64, delta64, dtype)
    print("fused tail: inside %s, neighbour fraction %.4g" % (ok, frac))
    assert ok and frac <= 0.01


# --------------------------------------------------------------------------------------------------------------------- class
ROWS = [1, 7, 64, 100, 28]


def _run_class(psgd, step_tail, pdtype, exact, route, clip, group=None, steps=6, nan_step=None):
    """6 steps of class UVd on a 200-row quadratic split into 5 tensors; everything random comes from seeds fixed here.
    nan_step: on that step (counted from 0) the closure adds NaN * w[17] to the loss: one NaN gradient element"""
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.uniform(0.5, 3.0, 200).astype(np.float32)).cuda()
    c = torch.from_numpy((rng.standard_normal(200) * 0.03).astype(np.float32)).cuda()
    w0 = rng.standard_normal(200).astype(np.float32)
    cuts = np.cumsum([0] + ROWS)
    params = [torch.from_numpy(w0[cuts[k]:cuts[k + 1]]).cuda().to(pdtype).requires_grad_(True) for k in range(5)]
    params[2] = params[2].detach().view(8, 8).requires_grad_(True)

    now = {"step": -1}

    def closure():
        w = torch.cat([p.reshape(-1) for p in params]).float()
        loss = 0.5 * torch.sum(a * w * w) + 0.5 * torch.sum(c * w) ** 2
        return loss + float("nan") * w[17] if now["step"] == nan_step else loss

    torch.manual_seed(100)
    psgd.manual_seed(101)
    kw = dict(state_dtype=torch.bfloat16, state_route="native") if route == "native" else dict(state_dtype="param")
    opt = psgd.UVd(params, rank_of_modification=5, lr_params=0.2, lr_preconditioner=0.05, grad_clip_max_norm=2.0 if clip else None,
                   exact_hessian_vector_product=exact, generator=torch.Generator().manual_seed(102), placement=None, group=group,
                   step_tail=step_tail, **kw)
    assert (opt._tail is not None) == (step_tail == "fused")
    losses = []
    for now["step"] in range(steps):
        losses.append(float(opt.step(closure)))
    now["step"] = -1
    losses.append(float(closure()))
    return [p.detach() for p in params], (opt._U, opt._V, opt._d), losses


@pytest.mark.parametrize("route", ["widen", "native"])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("pdtype", [torch.float32, torch.bfloat16])
def test_class_fused_tail_equals_torch_tail(psgd, pdtype, exact, route):
    pt, st, lt = _run_class(psgd, "torch", pdtype, exact, route, clip=False)
    pf, sf, lf = _run_class(psgd, "fused", pdtype, exact, route, clip=False)
    for k, (x, y) in enumerate(zip(pf, pt)):
        assert torch.equal(_bits(x), _bits(y)), ("parameter", k)
    for name, x, y in zip("UVd", sf, st):
        assert torch.equal(_bits(x), _bits(y)), name
    assert lf == lt and all(math.isfinite(v) for v in lf)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("pdtype", [torch.float32, torch.bfloat16])
def test_class_fused_tail_with_clipping(psgd, pdtype, exact):
    pt, _, lt = _run_class(psgd, "torch", pdtype, exact, "widen", clip=True)
    pf, _, lf = _run_class(psgd, "fused", pdtype, exact, "widen", clip=True)
    x = torch.cat([p.reshape(-1) for p in pf]).double()
    y = torch.cat([p.reshape(-1) for p in pt]).double()
    rel = float((x - y).norm() / y.norm())
    print("clipped run, %s exact=%s: relative difference %.3g, losses %s" % (pdtype, exact, rel, lf))
    assert rel <= (1e-6 if pdtype == torch.float32 else 1e-2)
    assert all(b < a for a, b in zip(lf, lf[1:])), lf


# ------------------------------------------------------------------------------------------------------------------- sharded
@pytest.fixture(scope="module")
def pg():
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29551", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_group_tail_equals_ungrouped_tail(psgd, pg, dtype):
    """a 1-rank RCCL group: the all-reduce of the sum of squares is the identity, so every bit must agree"""
    sizes = SIZE_LISTS["many"]
    a = _tensors(sizes, dtype, seed=31)
    b = [t.clone() for t in a]
    pre = torch.randn(sum(sizes), device="cuda", generator=torch.Generator(device="cuda").manual_seed(32))
    max_norm = 0.1 * float(pre.norm())
    psgd.uvd_step_tail(a, pre, 0.05, max_norm=max_norm)
    psgd.uvd_step_tail(b, pre, 0.05, max_norm=max_norm, group=pg)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    assert not torch.equal(_bits(a[-1]), _bits(_tensors(sizes, dtype, seed=31)[-1]))       # and something moved


def test_class_with_group_fused_equals_torch(psgd, pg):
    pt, st, _ = _run_class(psgd, "torch", torch.float32, True, "widen", clip=False, group=pg)
    pf, sf, _ = _run_class(psgd, "fused", torch.float32, True, "widen", clip=False, group=pg)
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(pf, pt))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(sf, st))
    _, _, lc = _run_class(psgd, "fused", torch.float32, True, "widen", clip=True, group=pg)      # the norm through the all-reduce
    assert all(b < a for a, b in zip(lc, lc[1:])), lc


# ------------------------------------------------------------------------------------------------------------------ fallback
def test_fallback_and_bad_value(psgd):
    base = torch.randn(6, 4, device="cuda")
    strided = base.t().detach().requires_grad_(True)
    assert not strided.is_contiguous()
    other = torch.randn(5, device="cuda", requires_grad=True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        opt = psgd.UVd([strided, other], rank_of_modification=2, placement=None, step_tail="fused")
    assert len([w for w in seen if "step_tail" in str(w.message)]) == 1
    assert opt._tail is None
    torch.manual_seed(0)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for _ in range(3):
            loss = opt.step(lambda: 0.5 * (strided * strided).sum() + 0.5 * (other * other).sum())
    assert not [w for w in seen if "step_tail" in str(w.message)] and math.isfinite(float(loss))                                          # one warning for the life of the object
    with pytest.raises(ValueError):
        psgd.UVd([other], rank_of_modification=2, step_tail="foreach")


# ---------------------------------------------------------------------------------------------------------------- first call
def test_first_call_on_poisoned_buffers(psgd):
    """the clipped update twice from the same inputs, each time with a fresh plan whose workspace, norm word and tables start as
    0xFF bytes / NaN: finite and identical (nothing reads what the call itself did not write)"""
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as core
    sizes = SIZES_SMALL
    start = _tensors(sizes, torch.bfloat16, seed=41)
    vs = _tensors(sizes, torch.bfloat16, seed=42, scale=0.01)
    pre = torch.randn(sum(sizes), device="cuda", generator=torch.Generator(device="cuda").manual_seed(43))
    results = []
    for _ in range(2):
        plan = core.UVdTailPlan(sizes, torch.bfloat16, pre.device)
        plan.ws.fill_(0xFF)
        plan.sumsq.fill_(float("nan"))
        params = [t.clone() for t in start]
        flat = torch.full((sum(sizes),), float("nan"), device="cuda")
        psgd.uvd_pack(params, flat, plan=plan)
        psgd.uvd_step_tail(params, pre, 0.05, max_norm=1.0, vs=vs, plan=plan)
        results.append((params, flat.clone()))
    torch.cuda.synchronize()
    for x, y in zip(results[0][0], results[1][0]):
        assert torch.isfinite(x.float()).all() and torch.equal(_bits(x), _bits(y))
    assert torch.isfinite(results[0][1]).all() and torch.equal(results[0][1], results[1][1])


# ------------------------------------------------------------------------------------------------------------- special values
def _specials(dtype):
    """+-0, +-Inf, NaN, the largest finite value, the smallest normal and two subnormals (half the smallest normal, the smallest
    subnormal) of `dtype`"""
    fi = torch.finfo(dtype)
    vals = [0.0, -0.0, math.inf, -math.inf, math.nan, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny * 0.5, fi.tiny * fi.eps]
    out = torch.tensor(vals, dtype=torch.float64).to(dtype).cuda()
    assert float(out[-1].double()) == fi.tiny * fi.eps and float(out[-2].double()) == fi.tiny * 0.5      # they survive the cast
    return out


def _plant(tensors, vals, shift=0):
    """write `vals` into every tensor of at least 257 elements at its start (the scalar head of a chunk and the first vector
    accesses), in its middle (the vector body) and at its end (the last vector access and the scalar tail); `shift` moves them"""
    k, hit = vals.numel(), 0
    for t in tensors:
        n = t.numel()
        if n < 257:
            continue
        f = t.view(-1)
        for lo in (shift, n // 2 + shift, n - k - shift):
            f[lo:lo + k] = vals.to(t.dtype)
        hit += 1
    assert hit >= 2
    return tensors


def _assert_same_or_both_nan(got, ref, what):
    """bit-equal wherever the reference is not NaN, and the same NaN mask"""
    got, ref = got.reshape(-1), ref.reshape(-1)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn), (what, "NaN masks differ at", torch.nonzero(gn != rn).reshape(-1)[:8].tolist(),
                                 "NaN in got / ref:", int(gn.sum()), int(rn.sum()))
    bad = (_bits(got) != _bits(ref)) & ~rn
    assert not bool(bad.any()), (what, "bits differ at", torch.nonzero(bad).reshape(-1)[:8].tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", list(SIZE_LISTS))
def test_pack_special_values(psgd, which, dtype):
    """the widening and the product of pack on special values of the SOURCE dtype; 1/3 is a scale whose products round"""
    sizes = SIZE_LISTS[which]
    ts = _plant(_tensors(sizes, dtype, seed=51), _specials(dtype))
    total = sum(sizes)
    for scale in (1.0, 2.0 ** -12, 1.0 / 3.0):
        ref = torch.cat([t.reshape(-1) for t in ts]).float() * scale
        assert int(torch.isnan(ref).sum()) >= 6 and int(torch.isinf(ref).sum()) >= 12
        for shift in (0, 1):
            buf = torch.full((total + 8,), 7.0, device="cuda")
            got = psgd.uvd_pack(ts, buf[shift:shift + total], scale)
            _assert_same_or_both_nan(got, ref, (which, dtype, scale, shift))
            assert bool((buf[:shift] == 7.0).all()) and bool((buf[shift + total:] == 7.0).all())


def _sumsq_ref(x):
    xs = x.cpu().numpy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sq = xs * xs                                      # numpy float32 products, as in test_sumsq
        assert sq.dtype == np.float32
        return float(np.sum(sq.astype(np.float64)))


@pytest.mark.parametrize("where", [5, 2049, 4098])       # the first trip of the vector loop, a later trip, the scalar tail
def test_sumsq_special_values(psgd, where):
    """NaN -> NaN; Inf -> +Inf; 3e19 -> +Inf (its fp32 square overflows: "each product rounded to fp32" is the contract);
    all 1e-30 -> exactly 0 (every fp32 square underflows to 0).  Reference: the numpy expression of test_sumsq."""
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import UVdTailPlan, uvd_sumsq
    N = 4099
    assert where < N and 4 * (N // 4) <= 4098
    base = torch.randn(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(61))
    plan = UVdTailPlan([N], torch.float32, base.device)
    for bad, want in ((math.nan, math.nan), (math.inf, math.inf), (-math.inf, math.inf), (3e19, math.inf), (-3e19, math.inf)):
        x = base.clone()
        x[where] = bad
        plan.sumsq.fill_(123.0)
        got = float(uvd_sumsq(x, plan=plan).item())
        ref = _sumsq_ref(x)
        assert (math.isnan(ref) and math.isnan(want)) or ref == want
        assert (math.isnan(got) and math.isnan(want)) or got == want, (bad, got, want)
    x = torch.full((N,), 1e-30, device="cuda")
    plan.sumsq.fill_(123.0)
    got = float(uvd_sumsq(x, plan=plan).item())
    assert _sumsq_ref(x) == 0.0 and got == 0.0 and math.copysign(1.0, got) == 1.0


def test_sumsq_of_nothing_is_zero(psgd, hip_lib):
    """N = 0 through the C ABI (the Python wrapper never passes it): no partial launch, the fold of zero partials writes +0"""
    from psgd_tf_amd import _lib
    x = torch.ones(4, device="cuda")
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.full((_lib.UVD_SUMSQ_WS_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = hip_lib.psgd_uvd_sumsq_f32(x.data_ptr(), 0, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert int(out.view(torch.int64).item()) == 0


def _special_update_inputs(which, dtype, with_vs):
    sizes = SIZE_LISTS[which]
    sp = _specials(dtype)
    ref = _plant(_tensors(sizes, dtype, seed=71), sp)
    vs = _plant(_tensors(sizes, dtype, seed=72, scale=0.05), sp.flip(0), shift=3) if with_vs else None
    pre = torch.randn(sum(sizes), device="cuda", generator=torch.Generator(device="cuda").manual_seed(73))
    sp32 = _specials(torch.float32)
    off = 0
    for n in sizes:                                          # pre_grad: fp32 specials against special and ordinary parameters
        if n >= 257:
            for lo in (5, n // 2 - 4, n - sp32.numel() - 7):
                pre[off + lo:off + lo + sp32.numel()] = sp32
        off += n
    if dtype == torch.float16:                               # +-65504 -+ delta: 65520 is the tie that rounds to Inf, 65519 stays finite
        kb = int(np.argmax(sizes))
        big, k0 = ref[kb].view(-1), sum(sizes[:kb])
        for j, (p0, dl) in enumerate([(65504.0, -16.0), (65504.0, -15.0), (65504.0, -1000.0), (-65504.0, 16.0), (-65504.0, 15.0),
                                      (-65504.0, 1000.0), (65504.0, 1000.0)]):
            big[100 + j] = p0
            pre[k0 + 100 + j] = dl                           # the first lr is 1: delta = dl exactly
            if vs is not None:
                vs[kb].view(-1)[100 + j] = 0.0
    got = [t.clone() for t in ref]
    got = [(torch.cat([t.reshape(-1)[:1], t.reshape(-1)])[1:].view(t.shape) if k % 3 == 1 else t) for k, t in enumerate(got)]
    return sizes, ref, got, vs, pre


@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", list(SIZE_LISTS))
def test_update_without_clipping_special_values(psgd, which, dtype, with_vs):
    """the unclipped update on special parameters, pre_grad and vs; float16 adds parameters at +-65504 whose update overflows"""
    sizes, ref, got, vs, pre = _special_update_inputs(which, dtype, with_vs)
    for lr in (1.0, 0.37):
        _torch_tail(ref, pre, lr, vs)
        psgd.uvd_step_tail(got, pre, lr, vs=vs)
        for k, (a, b) in enumerate(zip(got, ref)):
            _assert_same_or_both_nan(a, b, (which, dtype, with_vs, lr, k, sizes[k]))
        if dtype == torch.float16 and lr == 1.0:
            assert int(torch.isinf(torch.cat([t.reshape(-1) for t in ref])).sum()) >= 4      # the overflowing updates are in


@pytest.mark.parametrize("dtype", DTYPES)
def test_perturbation_special_values(psgd, dtype):
    """pre_grad=None, the p.add_(v) branch, on special parameters and vs"""
    sizes = SIZE_LISTS["six"]
    sp = _specials(dtype)
    ref = _plant(_tensors(sizes, dtype, seed=81), sp)
    vs = _plant(_tensors(sizes, dtype, seed=82, scale=2.0 ** -6), sp.flip(0), shift=3)
    got = [t.clone() for t in ref]
    for p, v in zip(ref, vs):
        p.add_(v)
    psgd.uvd_step_tail(got, None, 0.0, vs=vs)
    for k, (a, b) in enumerate(zip(got, ref)):
        _assert_same_or_both_nan(a, b, (dtype, k, sizes[k]))


def _clipped_torch_tail(params, pre, lr, max_norm, tiny):
    """psgd.py:753-762 as the torch tail of UVd.step computes it, on the device"""
    grad_norm = torch.sqrt(torch.sum(pre * pre)) + tiny
    _torch_tail(params, pre, lr * torch.clamp(max_norm / grad_norm, max=1.0), None)


def _clip_case(dtype, seed):
    sizes = SIZES_SMALL + [257, 12_345]
    start = _tensors(sizes, dtype, seed=seed)
    z = torch.tensor([0.0, -0.0, -0.0, 0.0], dtype=dtype, device="cuda")
    _plant(start, z)                                          # signed zeros among the parameters: -0 - (-0) = +0, -0 - (+0) = -0
    pre = torch.randn(sum(sizes), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 1)) * 0.7
    return sizes, start, pre


@pytest.mark.parametrize("dtype", DTYPES)
def test_clipped_update_nan_norm_poisons_every_parameter(psgd, dtype):
    """One NaN in pre_grad: the norm is NaN, tf.minimum (psgd.py:754) and torch.clamp return NaN, lr is NaN and EVERY parameter
    becomes NaN.  A comparison-based minimum (ratio < 1 ? ratio : 1) is false for a NaN and takes the full unclipped step."""
    sizes, start, pre = _clip_case(dtype, 91)
    pre[4242] = float("nan")
    tiny = float(torch.finfo(dtype).tiny)
    ref, got = [t.clone() for t in start], [t.clone() for t in start]
    _clipped_torch_tail(ref, pre, 0.05, 1.0, tiny)
    psgd.uvd_step_tail(got, pre, 0.05, max_norm=1.0, tiny=tiny)
    r, g = torch.cat([t.reshape(-1) for t in ref]), torch.cat([t.reshape(-1) for t in got])
    assert bool(torch.isnan(r).all())
    finite = int(torch.isfinite(g).sum())
    print("clipped update, NaN norm, %s: torch tail %d of %d NaN; fused tail %d NaN, %d finite"
          % (dtype, int(torch.isnan(r).sum()), r.numel(), int(torch.isnan(g).sum()), finite))
    assert finite == 0 and bool(torch.isnan(g).all()), "%d of %d parameters finite where the torch tail has NaN" % (finite, g.numel())


@pytest.mark.parametrize("dtype", DTYPES)
def test_clipped_update_inf_zero_gradient_and_zero_max_norm(psgd, dtype):
    """+Inf in pre_grad: the norm is +Inf, lr_eff = 0, every delta is +-0 and exactly the Inf element (0 * Inf) is NaN;
    an all-zero pre_grad (norm = tiny, ratio clamps to 1, delta = +-0); max_norm = 0 (lr_eff = 0).  Bits of the torch tail."""
    tiny = float(torch.finfo(dtype).tiny)
    for case in ("inf", "zero_grad", "zero_max_norm"):
        sizes, start, pre = _clip_case(dtype, 95)
        max_norm = 1.0
        if case == "inf":
            pre[4242] = float("inf")
        elif case == "zero_grad":
            pre.zero_()
            pre[::2] = -0.0
        else:
            max_norm = 0.0
        ref, got = [t.clone() for t in start], [t.clone() for t in start]
        _clipped_torch_tail(ref, pre, 0.05, max_norm, tiny)
        psgd.uvd_step_tail(got, pre, 0.05, max_norm=max_norm, tiny=tiny)
        for k, (a, b) in enumerate(zip(got, ref)):
            _assert_same_or_both_nan(a, b, (case, dtype, k, sizes[k]))
        g = torch.cat([t.reshape(-1) for t in got])
        s = torch.cat([t.reshape(-1) for t in start])
        nan_at = torch.nonzero(torch.isnan(g)).reshape(-1).tolist()
        assert nan_at == ([4242] if case == "inf" else []), (case, nan_at[:8])
        keep = torch.ones_like(g, dtype=torch.bool)
        keep[nan_at] = False
        assert torch.equal(g[keep].float(), s[keep].float())                  # nothing moved (signs of zeros: the bits above)
        if case == "zero_grad":
            flipped = _bits(g) != _bits(s)                                    # only -0 - (-0) = +0 may differ from the input
            assert bool(((s == 0) & (g == 0))[flipped].all())


def test_class_fused_tail_nan_gradient_equals_torch_tail(psgd):
    """class level: a NaN gradient element on the third step, clipping on; parameters and state carry the same NaN masks after
    it whichever tail runs"""
    pt, st, lt = _run_class(psgd, "torch", torch.float32, True, "widen", clip=True, steps=3, nan_step=2)
    pf, sf, lf = _run_class(psgd, "fused", torch.float32, True, "widen", clip=True, steps=3, nan_step=2)
    assert math.isnan(lt[2]) and math.isnan(lf[2]) and math.isfinite(lt[1]) and math.isfinite(lf[1])
    for k, (x, y) in enumerate(zip(pf, pt)):
        assert torch.equal(torch.isnan(x), torch.isnan(y)), ("parameter", k, int(torch.isnan(x).sum()), int(torch.isnan(y).sum()))
    assert any(bool(torch.isnan(y).any()) for y in pt)
    for name, x, y in zip("UVd", sf, st):
        assert torch.equal(torch.isnan(x), torch.isnan(y)), name


# ----------------------------------------------------------------------------------------------------------------- grid-stride
def _grid_stride_sizes():
    """[3, G C + C + 5] (G = the grid limit, C = the chunk): G + 3 chunks, the first three workgroups take a second one and the
    3-element tensor puts the big one off the 16-byte grid of the flat vector; [3, 2 G C + 5]: EVERY workgroup takes a second"""
    from psgd_tf_amd import _lib
    C, G = _lib.UVD_TAIL_CHUNK, _lib.UVD_TAIL_MAX_GRID
    return {"one_more": [3, G * C + C + 5], "all_twice": [3, 2 * G * C + 5]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", ["one_more", "all_twice"])
def test_pack_and_update_grid_stride(psgd, which, dtype):
    """more chunks than workgroups: the second trip of the grid-stride loops of pack and of the unclipped update, bit for bit"""
    from psgd_tf_amd import _lib
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import uvd_tail_chunks
    sizes = _grid_stride_sizes()[which]
    nchunks = int(uvd_tail_chunks(sizes).shape[0])
    assert nchunks > _lib.UVD_TAIL_MAX_GRID
    assert which != "all_twice" or nchunks > 2 * _lib.UVD_TAIL_MAX_GRID
    ts = _tensors(sizes, dtype, seed=111)
    total = sum(sizes)
    scale = 2.0 ** -12
    ref = torch.cat([t.reshape(-1) for t in ts]).float() * scale
    buf = torch.full((total + 8,), float("nan"), device="cuda")
    got = psgd.uvd_pack(ts, buf[1:1 + total], scale)
    assert torch.equal(_bits(got), _bits(ref))
    assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + total:]).all()
    del buf, got
    pre = ref * 4096.0                                          # (any fp32 vector of the right length)
    params = [t.clone() for t in ts]
    params[1] = torch.cat([ts[1].reshape(-1)[:1], ts[1].reshape(-1)])[1:].view(ts[1].shape)
    _torch_tail(ts, pre, 0.37, None)
    psgd.uvd_step_tail(params, pre, 0.37)
    for a, b in zip(params, ts):
        assert torch.equal(_bits(a), _bits(b))


def test_sumsq_grid_stride(psgd):
    """more tiles than partials: the second trip of the loop of the sum of squares; the bar and the reference of test_sumsq"""
    from psgd_tf_amd import _lib
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import UVdTailPlan, uvd_sumsq
    C = _lib.UVD_TAIL_CHUNK
    N = _lib.UVD_SUMSQ_PARTIALS * C + 4099
    assert -(-N // C) > _lib.UVD_SUMSQ_PARTIALS
    x = torch.randn(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(121)) * 3.0
    plan = UVdTailPlan([N], torch.float32, x.device)
    plan.ws.fill_(0xFF)
    plan.sumsq.fill_(float("nan"))
    first = uvd_sumsq(x, plan=plan).clone()
    second = uvd_sumsq(x, plan=plan).clone()
    ref = _sumsq_ref(x)
    got = float(first.item())
    print("sumsq N=%d: got %.17g ref %.17g rel %.3g" % (N, got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-12 * ref
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))
