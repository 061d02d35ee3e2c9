"""GPU: momentum and decoupled weight decay in the step tail of class UVd.

Kernels (psgd_uvd_pack_blend_f32, psgd_uvd_param_update_multi_wd, through the C ABI): bit for bit against NumPy float32
restatements of the formulas of include/psgd_hip.h -- every product, sum and narrowing rounded on its own -- wherever the
restatement is not NaN, and its NaN mask.  Class: the "fused" and "torch" tails, a hand-written loop over the functional API,
placed and unplaced states, checkpoint / resume and a 1-rank group, all bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SIZES = [0, 1, 4095, 4096, 4097, 3]


def _size_lists():
    from psgd_tf_amd import _lib
    C, G = _lib.UVD_TAIL_CHUNK, _lib.UVD_TAIL_MAX_GRID
    return {"six": SIZES, "grid_stride": [3, G * C + C + 5]}       # G + 3 chunks: three workgroups take a second one


@pytest.fixture
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


@pytest.fixture
def core():
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as m
    return m


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _specials(dtype):
    """+-0, +-Inf, NaN, the ends of the normal range and two subnormals of `dtype`"""
    fi = torch.finfo(dtype)
    vals = [0.0, -0.0, math.inf, -math.inf, math.nan, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny * 0.5, fi.tiny * fi.eps]
    return torch.tensor(vals, dtype=torch.float64).to(dtype).cuda()


def _tensors(sizes, dtype, seed, scale=1.0, specials=True, shift=0):
    """one tensor per size; every third one starts one element into its allocation (aligned to the element only); tensors of at
    least 257 elements carry the special values at their start, middle and end (scalar head, vector body, scalar tail)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    sp, out = _specials(dtype), []
    for k, n in enumerate(sizes):
        t = (torch.randn(n + 1, device="cuda", generator=g) * scale).to(dtype)
        t = t[1:] if k % 3 == 1 else t[:n].clone()
        if specials and n >= 257:
            for lo in (shift, n // 2 + shift, n - sp.numel() - shift):
                t[lo:lo + sp.numel()] = sp
        assert t.is_contiguous() and t.numel() == n
        out.append(t)
    return out


def _widen_np(t):
    """a device tensor of any of the three dtypes -> float32 numpy, exactly"""
    if t.dtype == torch.float32:
        return t.detach().cpu().numpy().reshape(-1).copy()
    if t.dtype == torch.float16:
        return t.detach().cpu().numpy().reshape(-1).astype(np.float32)
    u = t.detach().cpu().view(torch.int16).numpy().reshape(-1).view(np.uint16).astype(np.uint32) << 16
    return u.view(np.float32)


def _narrow_np(x, dtype):
    """T(x) as float32 numpy: round to nearest even into `dtype` and widen again"""
    x = np.asarray(x, dtype=np.float32)
    if dtype == torch.float32:
        return x
    with np.errstate(over="ignore", invalid="ignore"):
        if dtype == torch.float16:
            return x.astype(np.float16).astype(np.float32)
        u = x.view(np.uint32).astype(np.uint64)
        r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint32) << 16
        out = r.astype(np.uint32).view(np.float32).copy()
        out[np.isnan(x)] = np.nan
        return out


def _same_or_both_nan(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(ref, dtype=np.float32).reshape(-1)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (what, "NaN masks differ at", np.nonzero(gn != rn)[0][:8].tolist(), int(gn.sum()), int(rn.sum()))
    bad = (got.view(np.int32) != ref.view(np.int32)) & ~rn
    assert not bad.any(), (what, "bits differ at", np.nonzero(bad)[0][:8].tolist(), got[bad][:4], ref[bad][:4])


# --------------------------------------------------------------------------------------------------------------- pack + blend
def _blend_ref(ts, old, scale, beta, omb):
    """out = fl32(fl32(beta * out) + fl32(omb * x)), x = fl32(float(t) * scale); beta == 0: out = fl32(omb * x)"""
    f = np.float32
    with np.errstate(all="ignore"):
        x = np.concatenate([_widen_np(t) for t in ts]) * f(scale)
        assert x.dtype == np.float32
        nx = f(omb) * x
        if beta == 0.0:
            return nx
        return (f(beta) * old) + nx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["six", "grid_stride"])
def test_pack_blend_kernel_equals_the_float32_restatement(core, hip_lib, which, dtype):
    sizes = _size_lists()[which]
    total = sum(sizes)
    ts = _tensors(sizes, dtype, seed=3)
    plan = core.UVdTailPlan(sizes, dtype, ts[0].device)
    segs = plan.table("pack", ts, "test")
    g = torch.Generator(device="cuda").manual_seed(5)
    old0 = torch.randn(total + 8, device="cuda", generator=g)
    sp = _specials(torch.float32)
    for lo in (4, total // 2 + 5, total - sp.numel() - 2):          # special values in the buffer too, against special and ordinary x
        old0[lo:lo + sp.numel()] = sp
    inv_sqrt_eps = float(np.float32(1.0) / np.float32(torch.finfo(dtype).eps ** 0.5))
    for shift in ((0, 1) if which == "six" else (1,)):              # the buffer on a 16-byte boundary, and one element past it
        for beta in (0.0, 0.5, 0.9):
            beta = float(np.float32(beta))
            omb = float(np.float32(1.0) - np.float32(beta))
            for scale in (1.0, inv_sqrt_eps):
                buf = old0.clone()
                out = buf[shift:shift + total]
                ref = _blend_ref(ts, out.cpu().numpy(), scale, beta, omb)
                rc = hip_lib.psgd_uvd_pack_blend_f32(segs, len(ts), plan.chunks.data_ptr(), plan.nchunks, plan.code, scale, beta, omb,
                                                     out.data_ptr(), _stream())
                assert rc == 0
                _same_or_both_nan(out.cpu().numpy(), ref, (which, dtype, shift, beta, scale))
                assert int(np.isnan(ref).sum()) >= 3 and int(np.isinf(ref).sum()) >= 4          # the special values are in
                keep = torch.ones(total + 8, dtype=torch.bool, device="cuda")
                keep[shift:shift + total] = False                                               # nothing outside the vector moved
                assert torch.equal(_bits(buf[keep]), _bits(old0[keep]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pack_blend_beta_zero_does_not_read_the_buffer(psgd, hip_lib, core, dtype):
    """beta = 0, omb = 1 on a buffer of 0xFF bytes (NaN): the bits of psgd_uvd_pack_f32, through the C ABI and through
    uvd_pack_blend"""
    sizes = SIZES
    total = sum(sizes)
    ts = _tensors(sizes, dtype, seed=7)
    scale = float(np.float32(1.0) / np.float32(torch.finfo(dtype).eps ** 0.5))
    want = psgd.uvd_pack(ts, torch.empty(total, device="cuda"), scale).cpu().numpy()
    plan = core.UVdTailPlan(sizes, dtype, ts[0].device)
    segs = plan.table("pack", ts, "test")
    buf = torch.full((4 * total,), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32)
    assert bool(torch.isnan(buf).all())
    rc = hip_lib.psgd_uvd_pack_blend_f32(segs, len(ts), plan.chunks.data_ptr(), plan.nchunks, plan.code, scale, 0.0, 1.0, buf.data_ptr(),
                                         _stream())
    assert rc == 0
    _same_or_both_nan(buf.cpu().numpy(), want, (dtype, "C ABI"))
    buf = torch.full((4 * total,), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32)
    got = psgd.uvd_pack_blend(ts, buf, 0.0, scale)
    assert got.data_ptr() == buf.data_ptr() and got.shape == (total,)
    _same_or_both_nan(got.cpu().numpy(), want, (dtype, "uvd_pack_blend"))
    assert int(np.isnan(want).sum()) == 9                            # only the NaN of the inputs: none leaked from the buffer
    with pytest.raises(ValueError):
        psgd.uvd_pack_blend(ts, buf, 1.0)
    with pytest.raises(ValueError):
        psgd.uvd_pack_blend(ts, buf[:10], 0.5)


def test_pack_blend_wrapper_equals_the_torch_operations(psgd):
    """uvd_pack_blend(tensors, m, beta) == m.mul_(beta); m.add_(x.mul(1 - beta)): what the torch tail of class UVd runs"""
    ts = _tensors(SIZES, torch.bfloat16, seed=9, specials=False)
    m = torch.randn(sum(SIZES), device="cuda", generator=torch.Generator(device="cuda").manual_seed(10))
    ref = m.clone()
    for k in range(1, 4):
        beta, omb = psgd.uvd_momentum_coefficients(k, 0.9)
        x = torch.cat([t.reshape(-1) for t in ts]).float()
        ref.mul_(beta)
        ref.add_(x.mul(omb))
        psgd.uvd_pack_blend(ts, m, beta)
        assert torch.equal(_bits(m), _bits(ref)), k


# --------------------------------------------------------------------------------------------------- update with weight decay
def _update_ref(params, pre, vs, lr_eff, wd, dtype):
    """delta = T(fl32(lr_eff g)); [delta = T(delta + v)]; wd != 0: delta = T(delta + T(fl32(c p))), c = fl32(lr_eff wd);
    p = T(p - delta) -- float32 numpy, one operation per rounding"""
    f = np.float32
    with np.errstate(all="ignore"):
        p = np.concatenate([_widen_np(t) for t in params])
        delta = _narrow_np(f(lr_eff) * pre, dtype)
        if vs is not None:
            delta = _narrow_np(delta + np.concatenate([_widen_np(t) for t in vs]), dtype)
        if wd != 0.0:
            c = f(lr_eff) * f(wd)
            assert isinstance(c, np.float32)
            delta = _narrow_np(delta + _narrow_np(c * p, dtype), dtype)
        return _narrow_np(p - delta, dtype)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_wd_kernel_equals_the_float32_restatement(psgd, core, dtype, with_vs, clip):
    sizes = SIZES + [257]
    total = sum(sizes)
    params = _tensors(sizes, dtype, seed=21)
    vs = _tensors(sizes, dtype, seed=22, scale=0.05, shift=3) if with_vs else None
    pre = torch.randn(total, device="cuda", generator=torch.Generator(device="cuda").manual_seed(23)) * 0.7
    if not clip:                                                    # (with clipping one NaN would make every parameter NaN)
        sp = _specials(torch.float32)
        for lo in (sizes[2] + 7, total // 2, total - sp.numel() - 5):
            pre[lo:lo + sp.numel()] = sp
    plan = core.UVdTailPlan(sizes, dtype, pre.device)
    tiny = float(torch.finfo(dtype).tiny)
    pre_np = pre.cpu().numpy()
    for lr, wd in ((0.37, 0.01), (1.0, 0.5), (0.05, 3.0)):
        lr_eff = float(np.float32(lr))
        max_norm = None
        if clip:
            sumsq = float(core.uvd_sumsq(pre, plan=plan).item())      # the device double the kernel reads (fixed order: the same bits)
            max_norm = 0.25 * math.sqrt(sumsq)
            ratio = float(np.float32(max_norm)) / (math.sqrt(sumsq) + float(np.float32(tiny)))
            assert ratio < 0.3
            lr_eff = float(np.float32(float(np.float32(lr)) * min(ratio, 1.0)))
        ref = _update_ref(params, pre_np, vs, lr_eff, wd, dtype)
        psgd.uvd_step_tail(params, pre, lr, max_norm, tiny, vs, plan=plan, weight_decay=wd)
        got = np.concatenate([_widen_np(t) for t in params])
        _same_or_both_nan(got, ref, (dtype, with_vs, clip, lr, wd))
        assert 3 <= int(np.isnan(ref).sum()) < total // 2 and float(np.nanmax(np.abs(ref))) > 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_update_wd_grid_stride(psgd, dtype):
    """more chunks than workgroups: the second trip of the loop of the decayed update"""
    sizes = _size_lists()["grid_stride"]
    params = _tensors(sizes, dtype, seed=31)
    pre = torch.randn(sum(sizes), device="cuda", generator=torch.Generator(device="cuda").manual_seed(32))
    ref = _update_ref(params, pre.cpu().numpy(), None, float(np.float32(0.37)), 0.01, dtype)
    psgd.uvd_step_tail(params, pre, 0.37, weight_decay=0.01)
    _same_or_both_nan(np.concatenate([_widen_np(t) for t in params]), ref, dtype)


@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_wd_zero_is_the_old_entry_point(core, hip_lib, dtype, with_vs):
    sizes = SIZES + [257]
    start = _tensors(sizes, dtype, seed=41)
    vs = _tensors(sizes, dtype, seed=42, scale=0.05, shift=3) if with_vs else None
    pre = torch.randn(sum(sizes), device="cuda", generator=torch.Generator(device="cuda").manual_seed(43))
    plan = core.UVdTailPlan(sizes, dtype, pre.device)
    vsegs = plan.table("vs", vs, "test") if with_vs else None
    tiny = float(torch.finfo(dtype).tiny)
    for clip in (False, True):
        sq = core.uvd_sumsq(pre, plan=plan).data_ptr() if clip else None
        a, b = [t.clone() for t in start], [t.clone() for t in start]
        common = (len(sizes), plan.chunks.data_ptr(), plan.nchunks, plan.code, pre.data_ptr(), 0.37, sq, 3.0, tiny)
        assert hip_lib.psgd_uvd_param_update_multi(plan.table("params", a, "test"), vsegs, *common, _stream()) == 0
        assert hip_lib.psgd_uvd_param_update_multi_wd(plan.table("params", b, "test"), vsegs, *common, 0.0, _stream()) == 0
        for x, y, s in zip(a, b, start):
            _same_or_both_nan(_widen_np(x), _widen_np(y), (dtype, with_vs, clip))
        assert not torch.equal(_bits(a[2]), _bits(start[2]))
    with pytest.raises(ValueError):
        core.uvd_step_tail(start, None, 0.0, vs=start, weight_decay=0.1)


# --------------------------------------------------------------------------------------------------------------------- class
ROWS = [300, 0, 391, 1, 329]            # N = 1021 over five tensors, one of them empty, one two-dimensional
N, RANK, STEPS = sum(ROWS), 10, 8
MOM, WD = 0.9, 0.02


def _problem(pdtype):
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.uniform(0.5, 3.0, N).astype(np.float32)).cuda()
    c = torch.from_numpy((rng.standard_normal(N) * 0.03).astype(np.float32)).cuda()
    w0 = rng.standard_normal(N).astype(np.float32)
    cuts = np.cumsum([0] + ROWS)
    params = [torch.from_numpy(w0[cuts[k]:cuts[k + 1]]).cuda().to(pdtype) for k in range(5)]
    params[2] = params[2].view(17, 23)
    params = [p.requires_grad_(True) for p in params]
    a_k = [a[cuts[k]:cuts[k + 1]].view(params[k].shape) for k in range(5)]
    c_k = [c[cuts[k]:cuts[k + 1]].view(params[k].shape) for k in range(5)]
    return params, a_k, c_k


def _closure_for(params, a_k, c_k):
    def closure():                       # tensor by tensor: the empty one gets a differentiable (empty) gradient too
        quad = sum(0.5 * torch.sum(a * p.float() * p.float()) for p, a in zip(params, a_k))
        lin = sum(torch.sum(c * p.float()) for p, c in zip(params, c_k))
        return quad + 0.5 * lin ** 2
    return closure


def _make(psgd, params, step_tail, exact, clip, placement=None, group=None, momentum=MOM, weight_decay=WD, seed=103, **kw):
    if momentum is not None:
        kw.update(momentum=momentum, weight_decay=weight_decay)
    return psgd.UVd(params, rank_of_modification=RANK, lr_params=0.1, lr_preconditioner=0.05, grad_clip_max_norm=0.5 if clip else None,
                    preconditioner_update_probability=0.75, exact_hessian_vector_product=exact,
                    generator=torch.Generator().manual_seed(seed), placement=placement, group=group, step_tail=step_tail, **kw)


def _snapshot(params, opt):
    m = opt._momentum_buffer().clone() if float(opt.momentum) > 0 else None
    return {"params": [p.detach().clone() for p in params], "m": m, "U": opt._U.clone(), "V": opt._V.clone(), "d": opt._d.clone(),
            "k": opt._m_step}


def _run(psgd, step_tail, pdtype, exact, clip, steps=STEPS, **kw):
    params, a_k, c_k = _problem(pdtype)
    torch.manual_seed(100)
    opt = _make(psgd, params, step_tail, exact, clip, **kw)
    assert (opt._tail is not None) == (step_tail == "fused")
    seen, orig = [], opt._precondition
    opt._precondition = lambda v, h, g: (seen.append(v is None), orig(v, h, g))[1]
    closure = _closure_for(params, a_k, c_k)
    losses = [float(opt.step(closure)) for _ in range(steps)]
    if steps == STEPS:
        assert True in seen and False in seen                 # steps with and without a preconditioner update
    snap = _snapshot(params, opt)
    snap["losses"], snap["opt"] = losses, opt
    return snap


def _assert_same_run(x, y, what):
    for k, (a, b) in enumerate(zip(x["params"], y["params"])):
        assert torch.equal(_bits(a), _bits(b)), (what, "parameter", k)
    for name in ("m", "U", "V", "d"):
        if x[name] is None or y[name] is None:
            assert x[name] is None and y[name] is None, (what, name)
        else:
            assert torch.equal(_bits(x[name].reshape(-1)), _bits(y[name].reshape(-1))), (what, name)
    assert x["k"] == y["k"], what


_torch_runs = {}


def _torch_run(psgd, pdtype, exact, clip):
    """the reference run of a configuration, computed once and shared (never modified)"""
    key = (pdtype, exact, clip)
    if key not in _torch_runs:
        _torch_runs[key] = _run(psgd, "torch", pdtype, exact, clip)
    return _torch_runs[key]


CONFIGS = [(pd, ex, cl) for pd in (torch.float32, torch.bfloat16) for ex in (True, False) for cl in (False, True)]


@pytest.mark.parametrize("pdtype,exact,clip", CONFIGS)
def test_class_fused_tail_equals_torch_tail(psgd, pdtype, exact, clip):
    t = _torch_run(psgd, pdtype, exact, clip)
    f = _run(psgd, "fused", pdtype, exact, clip)
    _assert_same_run(f, t, (pdtype, exact, clip))
    assert t["k"] == STEPS and all(math.isfinite(v) for v in t["losses"]) and t["losses"][-1] < t["losses"][0]
    assert f["opt"]._m is not None and "g" not in f["opt"]._flat_bufs          # no flat g temporary beside the momentum buffer
    assert float(t["m"].abs().max()) > 0


def _manual_run(psgd, core, pdtype, exact, clip):
    """the same eight steps written out over the functional API, with a momentum buffer of its own"""
    params, a_k, c_k = _problem(pdtype)
    torch.manual_seed(100)
    seed_opt = _make(psgd, params, "torch", exact, clip)             # draws the initial U, V, d exactly as the class run does
    U, V, d = seed_opt._U, seed_opt._V, seed_opt._d
    gen = torch.Generator().manual_seed(103)
    closure = _closure_for(params, a_k, c_k)
    tiny, scale = torch.finfo(pdtype).tiny, torch.finfo(pdtype).eps ** 0.5
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).to(torch.float32)
    m = torch.zeros(N, device="cuda")
    for k in range(STEPS):
        update_Q = bool(torch.rand((), generator=gen).item() < 0.75)
        vs = None
        if update_Q and exact:
            grads = torch.autograd.grad(closure(), params, create_graph=True)
            vs = [torch.randn_like(p) for p in params]
            Hvs = torch.autograd.grad(grads, params, vs)
            grads = [g.detach() for g in grads]
        elif update_Q:
            grads = torch.autograd.grad(closure(), params)
            vs = [torch.randn_like(p) * scale for p in params]
            with torch.no_grad():
                for p, v in zip(params, vs):
                    p.add_(v)
            Hvs = [pg - g for pg, g in zip(torch.autograd.grad(closure(), params), grads)]
        else:
            grads = torch.autograd.grad(closure(), params)
        beta, omb = psgd.uvd_momentum_coefficients(k, MOM)
        g = flat(grads)
        if beta == 0.0:
            m.copy_(g.mul(omb))
        else:
            m.mul_(beta)
            m.add_(g.mul(omb))
        if update_Q:
            v, h = flat(vs), flat(Hvs)
            if not exact:
                v, h = v / scale, h / scale
            pre = psgd.update_precond_UVd_math_and_precond_grad(U, V, d, v[:, None].contiguous(), h[:, None].contiguous(),
                                                                m[:, None].contiguous(), step=0.05, tiny=tiny, generator=gen)
        else:
            pre = psgd.precond_grad_UVd_math(U, V, d, m[:, None].contiguous())
        lr = torch.tensor(0.1, dtype=torch.float32, device="cuda")
        if clip:                                                    # lr_eff as the step-tail kernel forms it: fp64, one rounding
            sq = torch.sum((pre * pre).double())
            ratio = float(np.float32(0.5)) / (torch.sqrt(sq) + float(np.float32(tiny)))
            lr = (lr.double() * torch.clamp(ratio, max=1.0)).float()
        c = lr * torch.tensor(WD, dtype=torch.float32, device="cuda")
        with torch.no_grad():
            lo = 0
            for j, p in enumerate(params):
                n = p.numel()
                delta = (lr * pre.reshape(-1)[lo:lo + n].reshape(p.shape)).to(p.dtype)
                if update_Q and not exact:
                    delta = delta + vs[j]
                delta = delta + (c * p.float()).to(p.dtype)
                p.sub_(delta)
                lo += n
    return {"params": [p.detach().clone() for p in params], "m": m, "U": U, "V": V, "d": d, "k": STEPS}


@pytest.mark.parametrize("pdtype,exact,clip", [(torch.float32, True, False), (torch.bfloat16, False, True), (torch.float32, False, False),
                                               (torch.bfloat16, True, True)])
def test_class_torch_tail_equals_a_hand_written_loop(psgd, core, pdtype, exact, clip):
    _assert_same_run(_torch_run(psgd, pdtype, exact, clip), _manual_run(psgd, core, pdtype, exact, clip), (pdtype, exact, clip))


@pytest.mark.parametrize("step_tail", ["fused", "torch"])
def test_class_placed_equals_unplaced(psgd, step_tail):
    placed = _run(psgd, step_tail, torch.float32, True, True, placement="packed")
    assert placed["opt"]._arena is not None and placed["opt"]._m is None          # m IS the arena's g region: no buffer of its own
    assert placed["opt"]._momentum_buffer().data_ptr() == placed["opt"]._arena.g.data_ptr()
    _assert_same_run(placed, _torch_run(psgd, torch.float32, True, True), step_tail)


@pytest.mark.parametrize("step_tail", ["fused", "torch"])
def test_class_defaults_take_the_paths_of_before(psgd, hip_lib, step_tail):
    """momentum=0, weight_decay=0 equals a run without the arguments; no buffer, no call of the new entry points"""
    from psgd_tf_amd import _lib
    calls = []

    class Spy:
        def __getattr__(self, name):
            if name in ("psgd_uvd_pack_blend_f32", "psgd_uvd_param_update_multi_wd"):
                calls.append(name)
            return getattr(hip_lib, name)
    real = _lib._lib
    _lib._lib = Spy()
    try:
        zero = _run(psgd, step_tail, torch.bfloat16, False, True, momentum=0.0, weight_decay=0.0)
        none = _run(psgd, step_tail, torch.bfloat16, False, True, momentum=None)
        assert not calls
        on = _run(psgd, step_tail, torch.bfloat16, False, True, steps=2)
        assert (sorted(set(calls)) == ["psgd_uvd_pack_blend_f32", "psgd_uvd_param_update_multi_wd"]) == (step_tail == "fused")
    finally:
        _lib._lib = real
    _assert_same_run(zero, none, step_tail)
    assert zero["m"] is None and zero["opt"]._m is None and zero["k"] == 0
    assert not torch.equal(_bits(on["params"][0]), _bits(zero["params"][0]))


def test_hyper_parameters_can_change_mid_run(psgd):
    """.assign between steps: momentum switched on warms up from k = 0 (the first blended step does not read the buffer), switched
    off it sets k back; an invalid value is refused at the next step"""
    params, a_k, c_k = _problem(torch.float32)
    torch.manual_seed(100)
    opt = _make(psgd, params, "fused", True, False, momentum=0.0, weight_decay=0.0)
    closure = _closure_for(params, a_k, c_k)
    opt.step(closure)
    assert opt._m is None and opt._m_step == 0
    opt.momentum.assign(0.9)
    opt.weight_decay.assign(0.01)
    opt._momentum_buffer().fill_(float("nan"))
    opt.step(closure)
    opt.step(closure)
    assert opt._m_step == 2 and bool(torch.isfinite(opt._m).all()) and all(bool(torch.isfinite(p).all()) for p in params)
    opt.momentum.assign(0.0)
    opt.step(closure)
    assert opt._m_step == 0
    opt.momentum.assign(1.0)
    with pytest.raises(ValueError, match="momentum"):
        opt.step(closure)


# ---------------------------------------------------------------------------------------------------------------- checkpoint
@pytest.mark.parametrize("step_tail,placement", [("fused", "packed"), ("torch", None), ("fused", None)])
def test_checkpoint_resume_is_bit_identical(psgd, step_tail, placement):
    whole = _run(psgd, step_tail, torch.float32, False, True, placement=placement)
    half = _run(psgd, step_tail, torch.float32, False, True, placement=placement, steps=4)
    sd = half["opt"].state_dict()
    cuda_rng = torch.cuda.get_rng_state()
    assert sd["momentum_step"] == 4 and sd["momentum_buffer"].device.type == "cpu" and sd["momentum_buffer"].dtype == torch.float32
    assert sd["momentum_buffer"].shape == (N,) and sd["hyper"]["momentum"] == MOM and sd["hyper"]["weight_decay"] == WD
    params, a_k, c_k = _problem(torch.float32)
    with torch.no_grad():
        for p, q in zip(params, half["params"]):
            p.copy_(q)
    torch.manual_seed(999)                                           # a NEW optimizer: other seeds, other hyper-parameters
    opt = _make(psgd, params, step_tail, True, False, placement=placement, momentum=0.5, weight_decay=0.0, seed=7)
    opt.load_state_dict(sd)
    assert float(opt.momentum) == MOM and float(opt.weight_decay) == WD and opt._m_step == 4
    torch.cuda.set_rng_state(cuda_rng)
    closure = _closure_for(params, a_k, c_k)
    for _ in range(4):
        opt.step(closure)
    _assert_same_run(_snapshot(params, opt), whole, (step_tail, placement))


def test_old_style_checkpoint_loads_with_a_zeroed_buffer(psgd):
    run = _run(psgd, "fused", torch.float32, True, False, steps=3)
    opt = run["opt"]
    sd = opt.state_dict()
    old = {k: v for k, v in sd.items() if k not in ("momentum_buffer", "momentum_step")}
    old["hyper"] = {k: v for k, v in sd["hyper"].items() if k not in ("momentum", "weight_decay")}
    assert float(opt._m.abs().max()) > 0 and opt._m_step == 3
    opt.momentum.assign(0.8)
    opt.load_state_dict(old)
    assert opt._m_step == 0 and float(opt._m.abs().max()) == 0.0
    assert float(opt.momentum) == 0.8 and float(opt.weight_decay) == WD            # the dict has none: the object keeps its own
    for name in ("U", "V", "d"):
        assert torch.equal(getattr(opt, "_" + name).cpu(), sd[name])
    bad = dict(sd)
    bad["momentum_buffer"] = sd["momentum_buffer"][:-1]
    with pytest.raises(ValueError, match="momentum_buffer"):
        opt.load_state_dict(bad)
    plain = _make(psgd, _problem(torch.float32)[0], "fused", True, False, momentum=0.0, weight_decay=0.0)
    plain.load_state_dict(old)                                                     # and into an optimizer without momentum
    assert plain._m is None and plain._m_step == 0


# ------------------------------------------------------------------------------------------------------------------- sharded
@pytest.fixture(scope="module")
def pg():
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29563", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield dist.group.WORLD
    dist.destroy_process_group()


@pytest.mark.parametrize("step_tail", ["fused", "torch"])
def test_one_rank_group_equals_the_unsharded_run(psgd, pg, step_tail):
    """a 1-rank RCCL group: every exchange and the all-reduce of the clip norm are the identity, m is this rank's rows = all rows"""
    grouped = _run(psgd, step_tail, torch.float32, True, True, group=pg)
    _assert_same_run(grouped, _torch_run(psgd, torch.float32, True, True), step_tail)
