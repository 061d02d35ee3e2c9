"""GPU: the step tail of class UVd in HIP (psgd_uvd_tail.hip) -- uvd_pack, the sum of squares of the clip norm, uvd_step_tail and
UVd(step_tail="fused") -- against the torch expressions of the default tail, which are copied here as the reference."""
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


def _run_class(psgd, step_tail, pdtype, exact, route, clip, group=None, steps=6):
    """6 steps of class UVd on a 200-row quadratic split into 5 tensors; everything random comes from seeds fixed here"""
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.uniform(0.5, 3.0, 200).astype(np.float32)).cuda()
    c = torch.from_numpy((rng.standard_normal(200) * 0.03).astype(np.float32)).cuda()
    w0 = rng.standard_normal(200).astype(np.float32)
    cuts = np.cumsum([0] + ROWS)
    params = [torch.from_numpy(w0[cuts[k]:cuts[k + 1]]).cuda().to(pdtype).requires_grad_(True) for k in range(5)]
    params[2] = params[2].detach().view(8, 8).requires_grad_(True)

    def closure():
        w = torch.cat([p.reshape(-1) for p in params]).float()
        return 0.5 * torch.sum(a * w * w) + 0.5 * torch.sum(c * w) ** 2

    torch.manual_seed(100)
    psgd.manual_seed(101)
    kw = dict(state_dtype=torch.bfloat16, state_route="native") if route == "native" else dict(state_dtype="param")
    opt = psgd.UVd(params, rank_of_modification=5, lr_params=0.2, lr_preconditioner=0.05, grad_clip_max_norm=2.0 if clip else None,
                   exact_hessian_vector_product=exact, generator=torch.Generator().manual_seed(102), placement=None, group=group,
                   step_tail=step_tail, **kw)
    assert (opt._tail is not None) == (step_tail == "fused")
    losses = [float(opt.step(closure)) for _ in range(steps)]
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
