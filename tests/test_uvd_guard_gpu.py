"""GPU: the guarded step of class UVd (nonfinite="skip", loss_scale) and its two kernels.

Kernels (psgd_uvd_pack_check_f32 through uvd_pack(flag=, stamp=), psgd_uvd_check_multi through uvd_check): one bad value planted
in every element path of a chunk raises the flag to the stamp, the packed vector keeps the bits of the plain pack, the check
writes nothing; clean lists do not raise it.  Class: a skipped step leaves every bit where it was, loss scaling by a power of two
changes no bit, the dynamic scale backs off and grows, and a checkpoint taken after a skip resumes bit for bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8193]
BAD = [math.inf, -math.inf, math.nan]
BIG = SIZES.index(8193)


@pytest.fixture
def psgd():
    import preconditioned_stochastic_gradient_descent as m
    return m


@pytest.fixture
def core():
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as m
    return m


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------------------------------- kernels
GUARD = 9           # NaN words between the sources: a kernel that read one of them would raise the flag on a clean list


def _sources(sizes, dtype, seed):
    """the tensors as views of ONE buffer, separated by GUARD NaN words, tensor k starting k elements past a 16-byte boundary
    (source heads 0, 1, 2, 3 for fp32 and 0 .. 7 for the 16-bit types); returns (buffer, views, mask of the guard words)"""
    per16 = 128 // torch.finfo(dtype).bits
    offs, pos = [], 0
    for k, n in enumerate(sizes):
        pos += GUARD
        pos += (k % per16 - pos) % per16
        offs.append(pos)
        pos += n
    buf = torch.full((pos + GUARD,), math.nan, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    g = torch.Generator(device="cuda").manual_seed(seed)
    guard = torch.ones(pos + GUARD, dtype=torch.bool, device="cuda")
    views = []
    for o, n in zip(offs, sizes):
        buf[o:o + n] = torch.randn(n, device="cuda", generator=g).to(dtype)
        guard[o:o + n] = False
        views.append(buf[o:o + n])
    return buf, views, guard


class _Judge:
    """runs the checked pack and the check on one list with a fresh stamp each and reports (raised by pack, raised by check);
    the packed vector must have the bits of the plain pack"""

    def __init__(self, core, views, sizes, dtype):
        self.core, self.views, self.total = core, views, sum(sizes)
        self.plan = core.UVdTailPlan(sizes, dtype, views[0].device)
        self.stamp = 0
        self.out = torch.empty(self.total + 4, device="cuda")
        self.ref = torch.empty(self.total + 4, device="cuda")

    def __call__(self, shift, scale, what):
        core, plan = self.core, self.plan
        self.out.fill_(-7.0)
        self.ref.fill_(-7.0)
        self.stamp += 2
        got = core.uvd_pack(self.views, self.out[shift:shift + self.total], scale, plan=plan, flag=plan.flags[0:1], stamp=self.stamp)
        core.uvd_check(self.views, scale, plan=plan, role="pack", flag=plan.flags[2:3], stamp=self.stamp + 1)
        want = core.uvd_pack(self.views, self.ref[shift:shift + self.total], scale, plan=plan)
        assert torch.equal(_bits(self.out), _bits(self.ref)), (what, "the checked pack writes other bits than the plain pack")
        assert got.data_ptr() == self.out[shift:].data_ptr() and want.numel() == self.total
        flags = plan.flags.tolist()
        assert flags[1] == 0 and flags[3] == 0, (what, flags)                       # nobody else's word was touched
        return flags[0] == self.stamp, flags[2] == self.stamp + 1


def _plants(shift, dtype):
    """(tensor, element, path) of the bad values for the output starting `shift` elements past a 16-byte boundary: the paths of
    k_uvd_pack in the first chunk of the 8193-element tensor, the chunk border, and the short tensors"""
    E = 4 if dtype == torch.float32 else 8
    start = sum(SIZES[:BIG])
    head = (-(shift + start)) % 4                       # head_of(dst) of the first chunk: elements up to the 16-byte boundary
    nvec = (4096 - head) // E
    out = [(BIG, head, "body-first"), (BIG, head + E - 1, "body-first"), (BIG, head + (nvec - 1) * E, "body-last"),
           (BIG, head + nvec * E - 1, "body-last"), (BIG, 4095, "chunk-last"), (BIG, 4096, "chunk-next-first"), (BIG, 8192, "last")]
    if head:
        out += [(BIG, 0, "head"), (BIG, head - 1, "head")]
    if head + nvec * E < 4096:
        out += [(BIG, head + nvec * E, "tail"), (BIG, 4095, "tail")]
    out += [(SIZES.index(4097), 4095, "chunk-last"), (SIZES.index(4097), 4096, "chunk-next-first")]
    for n in (1, 3, 5, 63, 65):
        k = SIZES.index(n)
        h = (-(shift + sum(SIZES[:k]))) % 4
        out += [(k, 0, "short-in-head" if n <= h else ("head" if h else "body-first")), (k, n - 1, "short")]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_bad_value_anywhere_raises_the_flag(core, dtype):
    buf, views, guard = _sources(SIZES, dtype, seed=11)
    before = buf.clone()
    judge = _Judge(core, views, SIZES, dtype)
    assert judge(0, 1.0, "clean") == (False, False)
    inv_sqrt_eps = float(np.float32(1.0) / np.float32(torch.finfo(dtype).eps ** 0.5))
    paths, heads = set(), set()
    for shift in (0, 1, 2, 3):
        assert judge(shift, inv_sqrt_eps, ("clean", shift)) == (False, False)
        for k, i, path in _plants(shift, dtype):
            paths.add(path)
            heads.add((-(shift + sum(SIZES[:k]))) % 4)
            keep = views[k][i].clone()
            for bad in BAD:
                views[k][i] = bad
                assert judge(shift, 1.0, (dtype, shift, k, i, path, bad)) == (True, True), (dtype, shift, k, i, path, bad)
            views[k][i] = keep
        assert judge(shift, 1.0, ("clean again", shift)) == (False, False)          # the stamps of the bad runs do not linger
    assert paths >= {"head", "body-first", "body-last", "tail", "chunk-last", "chunk-next-first", "short-in-head", "short", "last"}
    assert heads == {0, 1, 2, 3}
    assert torch.equal(_bits(buf), _bits(before))                                   # sources and guard words: not a bit moved
    assert bool(torch.isnan(buf[guard].float()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_trip_of_the_grid_stride_loop(core, dtype):
    from psgd_tf_amd import _lib
    sizes = [3, _lib.UVD_TAIL_MAX_GRID * _lib.UVD_TAIL_CHUNK + _lib.UVD_TAIL_CHUNK + 5]       # 2048 + 3 chunks
    buf, views, guard = _sources(sizes, dtype, seed=12)
    judge = _Judge(core, views, sizes, dtype)
    assert judge.plan.nchunks > _lib.UVD_TAIL_MAX_GRID
    assert judge(1, 1.0, "clean") == (False, False)
    for bad in BAD:
        views[1][-1] = bad
        assert judge(1, 1.0, (dtype, bad)) == (True, True), (dtype, bad)
    views[1][-1] = 1.0
    assert judge(1, 1.0, "clean again") == (False, False)
    assert bool(torch.isnan(buf[guard].float()).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_lists_and_overflow_under_the_scale(core, dtype):
    """+-0, subnormals and +-the largest finite value of the dtype are finite under scale = 1; the largest finite fp32 (and
    bf16) times 2 is not: the predicate is on the WRITTEN value"""
    fi = torch.finfo(dtype)
    vals = torch.tensor([0.0, -0.0, fi.tiny * 0.5, -fi.tiny * 0.5, fi.tiny * fi.eps, -fi.tiny * fi.eps, fi.max, -fi.max, fi.tiny],
                        dtype=torch.float64).to(dtype)
    assert bool(torch.isfinite(vals).all()) and float(vals[6]) == fi.max
    buf, views, guard = _sources(SIZES, dtype, seed=13)
    for v in views:                                   # the special values over and over: every path of every tensor sees them
        v.copy_(vals.cuda().repeat(v.numel() // vals.numel() + 1)[:v.numel()])
    judge = _Judge(core, views, SIZES, dtype)
    for shift in (0, 1, 2, 3):
        assert judge(shift, 1.0, (dtype, shift)) == (False, False)
    overflows = dtype != torch.float16                # bfloat16 has float32's range; twice the float16 maximum is a finite float32
    assert judge(1, 2.0, (dtype, "scale 2")) == (overflows, overflows)
    assert judge(2, -2.0, (dtype, "scale -2")) == (overflows, overflows)
    assert judge(1, 1.0, (dtype, "scale 1 again")) == (False, False)
    if dtype == torch.float32:                        # one such element is enough, whatever path it is in
        buf2, views2, _ = _sources(SIZES, dtype, seed=14)
        judge2 = _Judge(core, views2, SIZES, dtype)
        for k, i in ((BIG, 0), (BIG, 4000), (BIG, 8192), (1, 0)):
            keep = views2[k][i].clone()
            views2[k][i] = -fi.max
            assert judge2(3, 1.0, (k, i)) == (False, False)
            assert judge2(3, 2.0, (k, i)) == (True, True)
            views2[k][i] = keep


def test_stamps_and_argument_errors(core, hip_lib):
    from psgd_tf_amd import _lib
    sizes = [5, 4097]
    _, views, _ = _sources(sizes, torch.float32, seed=15)
    plan = core.UVdTailPlan(sizes, torch.float32, views[0].device)
    assert plan.flags.dtype == torch.int32 and plan.flags.tolist() == [0, 0, 0, 0]
    out = torch.empty(sum(sizes), device="cuda")
    views[1][4096] = math.nan
    core.uvd_pack(views, out, plan=plan, flag=plan.flags[1:2], stamp=7)
    core.uvd_check(views, plan=plan, flag=plan.flags[3:4], stamp=2 ** 31 - 1)
    assert plan.flags.tolist() == [0, 7, 0, 2 ** 31 - 1]
    views[1][4096] = 0.5
    core.uvd_pack(views, out, plan=plan, flag=plan.flags[1:2], stamp=8)            # a clean list under the next stamp ...
    core.uvd_check(views, plan=plan, flag=plan.flags[3:4], stamp=1)
    assert plan.flags.tolist() == [0, 7, 0, 2 ** 31 - 1]                           # ... leaves the old stamps: neither reads as bad
    with pytest.raises(ValueError, match="flag and stamp"):
        core.uvd_pack(views, out, plan=plan, stamp=3)
    with pytest.raises(ValueError, match="flag and stamp"):
        core.uvd_pack(views, out, plan=plan, flag=plan.flags[0:1])
    with pytest.raises(ValueError, match="int32"):
        core.uvd_pack(views, out, plan=plan, flag=out, stamp=3)
    for stamp in (0, -1):
        with pytest.raises(_lib.PsgdHipError, match="psgd_uvd_pack_check_f32"):
            core.uvd_pack(views, out, plan=plan, flag=plan.flags[0:1], stamp=stamp)
        with pytest.raises(_lib.PsgdHipError, match="psgd_uvd_check_multi"):
            core.uvd_check(views, plan=plan, flag=plan.flags[0:1], stamp=stamp)
    segs, st = plan.table("pack", views, "test"), torch.cuda.current_stream().cuda_stream
    args = (segs, 2, plan.chunks.data_ptr(), plan.nchunks, plan.code, 1.0)
    assert hip_lib.psgd_uvd_pack_check_f32(*args, out.data_ptr(), None, 1, st) == _lib.PSGD_ERR_BAD_ARG
    assert hip_lib.psgd_uvd_pack_check_f32(*args, out.data_ptr(), plan.flags.data_ptr(), 0, st) == _lib.PSGD_ERR_BAD_ARG
    assert hip_lib.psgd_uvd_check_multi(*args, None, 1, st) == _lib.PSGD_ERR_BAD_ARG
    assert hip_lib.psgd_uvd_check_multi(*args, plan.flags.data_ptr(), 0, st) == _lib.PSGD_ERR_BAD_ARG
    assert plan.flags.tolist() == [0, 7, 0, 2 ** 31 - 1]


# --------------------------------------------------------------------------------------------------------------------- class
ROWS = [300, 0, 391, 1, 329]            # N = 1021 over five tensors, one of them empty, one two-dimensional
N, RANK = sum(ROWS), 10


def _problem(pdtype, scale=1.0):
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.uniform(0.5, 3.0, N).astype(np.float32)).cuda()
    c = torch.from_numpy((rng.standard_normal(N) * 0.03).astype(np.float32)).cuda()
    w0 = rng.standard_normal(N).astype(np.float32) * scale
    cuts = np.cumsum([0] + ROWS)
    params = [torch.from_numpy(w0[cuts[k]:cuts[k + 1]]).cuda().to(pdtype) for k in range(5)]
    params[2] = params[2].view(17, 23)
    params = [p.requires_grad_(True) for p in params]
    a_k = [a[cuts[k]:cuts[k + 1]].view(params[k].shape) for k in range(5)]
    c_k = [c[cuts[k]:cuts[k + 1]].view(params[k].shape) for k in range(5)]
    return params, a_k, c_k


def _closure_for(params, a_k, c_k, factor):
    def closure():                       # factor["x"] = inf on the step that overflows
        quad = sum(0.5 * torch.sum(a * p.float() * p.float()) for p, a in zip(params, a_k))
        lin = sum(torch.sum(c * p.float()) for p, c in zip(params, c_k))
        return (quad + 0.5 * lin ** 2) * factor["x"]
    return closure


def _snapshot(params, opt):
    return {"params": [p.detach().clone() for p in params], "U": opt._U.clone(), "V": opt._V.clone(), "d": opt._d.clone(),
            "m": opt._momentum_buffer().clone() if float(opt.momentum) > 0 else None,
            "m_step": opt._m_step, "round_step": getattr(opt, "_round_step", None)}


def _ulp(x, dtype):
    """the spacing of `dtype` at magnitude x (float64 numpy; frexp / ldexp on the host are exact, a device pow(2, e) need not be)"""
    fi = torch.finfo(dtype)
    _, e = np.frexp(np.maximum(np.abs(x), fi.tiny))                   # x = m 2^e, 0.5 <= m < 1
    return np.ldexp(fi.eps, e - 1)


CONFIGS = {"fp32": (torch.float32, dict(placement=None)),
           "fp32-packed": (torch.float32, dict(placement="packed")),
           "fp16-fp32state": (torch.float16, dict(placement=None)),
           "bf16-native": (torch.bfloat16, dict(placement=None, state_dtype=torch.bfloat16, state_route="native"))}


def _guard_run(psgd, core, monkeypatch, config, tail, exact, mom, nonfinite, prob=1.0):
    pdtype, kw = CONFIGS[config]
    params, a_k, c_k = _problem(pdtype)
    torch.manual_seed(100)
    opt = psgd.UVd(params, rank_of_modification=RANK, lr_params=0.05, lr_preconditioner=0.05, grad_clip_max_norm=0.5,
                   preconditioner_update_probability=prob, exact_hessian_vector_product=exact, momentum=mom,
                   generator=torch.Generator().manual_seed(103), step_tail=tail, nonfinite=nonfinite, **kw)
    assert (opt._tail is not None) == (tail == "fused") and (opt._arena is not None) == (config == "fp32-packed")
    draws = []
    real = core._randn_like
    monkeypatch.setattr(core, "_randn_like", lambda p: (draws.append(real(p)), draws[-1])[1])
    calls = []
    orig = opt._precondition
    opt._precondition = lambda v, h, g: (calls.append(1), orig(v, h, g))[1]
    factor = {"x": 1.0}
    closure = _closure_for(params, a_k, c_k, factor)
    for _ in range(2):
        assert math.isfinite(float(opt.step(closure)))
    before, n_calls = _snapshot(params, opt), len(calls)
    del draws[:]
    factor["x"] = math.inf
    ret = opt.step(closure)
    factor["x"] = 1.0
    return opt, params, closure, before, ret, draws, len(calls) - n_calls


@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("tail", ["fused", "torch"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_skipped_step_leaves_every_bit(psgd, core, monkeypatch, config, tail, exact, mom):
    """Two good steps, one whose loss is multiplied by inf, one more good step.  After the bad one U, V, d, the momentum buffer,
    _m_step and _round_step equal their snapshots bit for bit, and so do the parameters on the exact route.  On the
    finite-difference route a parameter is p' = T(T(p + v) - v): each of the two roundings errs by at most half a spacing of T at
    a magnitude of at most |p| + |v|, so |p' - p| <= ulp_T(|p| + |v|), one spacing of T where the perturbed parameter lives (v is
    absolute, sqrt(eps) randn: relative to a small |p| alone the difference can be many of ITS spacings, in the reference too)."""
    opt, params, closure, before, ret, draws, precond_calls = _guard_run(psgd, core, monkeypatch, config, tail, exact, mom, "skip")
    assert not math.isfinite(float(ret))                                           # the closure's value, passed through
    assert opt.last_step_skipped is True and opt.skipped_steps == 1 and precond_calls == 0
    after = _snapshot(params, opt)
    for name in ("U", "V", "d", "m"):
        if before[name] is None:
            assert after[name] is None
        else:
            assert torch.equal(_bits(after[name].reshape(-1)), _bits(before[name].reshape(-1))), name
    assert after["m_step"] == before["m_step"] == (2 if mom else 0) and after["round_step"] == before["round_step"]
    pdtype = CONFIGS[config][0]
    for k, (p0, p1) in enumerate(zip(before["params"], after["params"])):
        if exact:
            assert torch.equal(_bits(p1), _bits(p0)), ("parameter", k)
        elif p0.numel():
            v = (draws[k] * opt._delta_param_scale).double().cpu().numpy()         # as step() forms it, in the parameters' type
            p0 = p0.double().cpu().numpy()
            err = np.abs(p1.double().cpu().numpy() - p0)
            bound = _ulp((np.abs(p0) + np.abs(v)) * (1 + 2 * torch.finfo(pdtype).eps), pdtype)
            print("%s %s mom=%g tensor %d: max |p' - p| / bound = %.3f" % (config, tail, mom, k, float((err / bound).max())))
            assert (err <= bound).all(), ("parameter", k, float((err / bound).max()))
    assert math.isfinite(float(opt.step(closure)))                                 # the next good step
    assert opt.last_step_skipped is False and opt.skipped_steps == 1
    assert opt._m_step == (3 if mom else 0)
    for t in [opt._U, opt._V, opt._d] + list(params) + ([opt._momentum_buffer()] if mom else []):
        assert bool(torch.isfinite(t.float()).all())
    assert any(not torch.equal(_bits(p1), _bits(p2.detach())) for p1, p2 in zip(after["params"], params))


@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("tail", ["fused", "torch"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_propagate_is_the_contract_of_before(psgd, core, monkeypatch, config, tail, exact, mom):
    """the same run with nonfinite="propagate" (the default) ends with a NaN state"""
    opt, params, closure, before, ret, draws, precond_calls = _guard_run(psgd, core, monkeypatch, config, tail, exact, mom, "propagate")
    assert precond_calls == 1 and opt.skipped_steps == 0 and opt.last_step_skipped is False
    assert not all(bool(torch.isfinite(t.float()).all()) for t in (opt._U, opt._V, opt._d))
    assert all(not bool(torch.isfinite(p.float()).all()) for p in params if p.numel())
    if mom:
        assert not bool(torch.isfinite(opt._momentum_buffer()).all())


@pytest.mark.parametrize("tail", ["fused", "torch"])
@pytest.mark.parametrize("mom", [0.0, 0.9])
def test_a_step_without_an_update_checks_g_alone(psgd, core, monkeypatch, tail, mom):
    opt, params, closure, before, ret, draws, precond_calls = _guard_run(psgd, core, monkeypatch, "fp16-fp32state", tail, True, mom,
                                                                         "skip", prob=0.0)
    assert opt.last_step_skipped and opt.skipped_steps == 1 and precond_calls == 0 and not draws
    after = _snapshot(params, opt)
    for name in ("U", "V", "d", "m"):
        if before[name] is not None:
            assert torch.equal(_bits(after[name].reshape(-1)), _bits(before[name].reshape(-1))), name
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(after["params"], before["params"])) and after["m_step"] == before["m_step"]
    if tail == "fused":
        flags = opt._tail.flags.tolist()
        assert flags[2] == opt._stamp and flags[0] == flags[1] == flags[3] == 0     # only g's word was ever written
    assert math.isfinite(float(opt.step(closure))) and not opt.last_step_skipped


# ---------------------------------------------------------------------------------------------------------------- loss scale
def _mlp_run(psgd, tail, exact, mom, **kw):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 8, generator=g).cuda()
    y = torch.randn(64, 1, generator=g).cuda()
    params = [(torch.randn(8, 16, generator=g) * 0.4).cuda().requires_grad_(True), torch.zeros(16, device="cuda", requires_grad=True),
              (torch.randn(16, 1, generator=g) * 0.3).cuda().requires_grad_(True), torch.zeros(1, device="cuda", requires_grad=True)]

    def closure():
        W1, b1, W2, b2 = params
        return torch.mean((torch.tanh(x @ W1 + b1) @ W2 + b2 - y) ** 2)
    torch.manual_seed(200)
    opt = psgd.UVd(params, rank_of_modification=5, lr_params=0.05, lr_preconditioner=0.1, grad_clip_max_norm=1.0,
                   preconditioner_update_probability=0.8, exact_hessian_vector_product=exact, momentum=mom, placement=None,
                   generator=torch.Generator().manual_seed(9), step_tail=tail, **kw)
    losses = [float(opt.step(closure)) for _ in range(5)]
    return opt, params, losses


@pytest.mark.parametrize("mom", [0.0, 0.9])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("tail", ["fused", "torch"])
def test_loss_scale_changes_no_bit(psgd, tail, exact, mom):
    """fp32 parameters, a small tanh MLP: five steps with loss_scale = 2^10 equal five steps of an optimizer without the arguments,
    bit for bit (the factor and its inverse are exact), and the closure's value is the unscaled loss"""
    plain, p0, l0 = _mlp_run(psgd, tail, exact, mom)
    scaled, p1, l1 = _mlp_run(psgd, tail, exact, mom, nonfinite="skip", loss_scale=2.0 ** 10)
    assert scaled.skipped_steps == 0 and l0 == l1 and all(math.isfinite(v) for v in l0)
    for a, b in zip(p0 + [plain._U, plain._V, plain._d], p1 + [scaled._U, scaled._V, scaled._d]):
        assert torch.equal(_bits(a.detach()), _bits(b.detach()))
    if mom:
        assert torch.equal(_bits(plain._momentum_buffer()), _bits(scaled._momentum_buffer()))


@pytest.mark.parametrize("tail", ["fused", "torch"])
def test_dynamic_scale_backs_off_and_grows(psgd, tail):
    """fp16 parameters with max |p| = 1.5 and loss = sum p^2 / 2 in float32: the gradient in the parameters' type is fl16(S p),
    which overflows at S = 2^16 (98304 > 65504) and not at 2^15 (49152); lr = 1e-3 moves |p| by parts in a thousand, far from
    either border.  Steps that leave the preconditioner alone, so that g decides alone."""
    w = torch.linspace(-1.5, 1.5, 1021).to(torch.float16).cuda()
    assert float(w.abs().max()) == 1.5
    params = [w[:500].clone().requires_grad_(True), w[500:].clone().requires_grad_(True)]
    closure = lambda: 0.5 * sum(torch.sum(p.float() ** 2) for p in params)
    opt = psgd.UVd(params, rank_of_modification=RANK, lr_params=1e-3, preconditioner_update_probability=0.0, placement=None,
                   generator=torch.Generator().manual_seed(1), step_tail=tail, nonfinite="skip", loss_scale="dynamic",
                   loss_scale_growth_interval=2)
    seen = []
    for _ in range(6):
        before = [p.detach().clone() for p in params]
        loss = float(opt.step(closure))
        assert math.isfinite(loss) and loss < 1000.0                               # the unscaled loss
        seen.append((float(opt.loss_scale), opt.last_step_skipped, opt.skipped_steps))
        same = all(torch.equal(_bits(a), _bits(b.detach())) for a, b in zip(before, params))
        assert same == opt.last_step_skipped
    #                2^16 overflows     two good steps at 2^15 double it   2^16 overflows again ...
    assert seen == [(2.0 ** 15, True, 1), (2.0 ** 15, False, 1), (2.0 ** 16, False, 1), (2.0 ** 15, True, 2), (2.0 ** 15, False, 2),
                    (2.0 ** 16, False, 2)], seen
    assert all(bool(torch.isfinite(p).all()) for p in params)


def test_dynamic_scale_clamps(psgd):
    params, a_k, c_k = _problem(torch.float32, scale=1e-3)
    factor = {"x": 1.0}
    closure = _closure_for(params, a_k, c_k, factor)
    opt = psgd.UVd(params, rank_of_modification=RANK, lr_params=1e-3, placement=None, generator=torch.Generator().manual_seed(1),
                   step_tail="fused", nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=1)
    opt.loss_scale.assign(2.0 ** 23)
    opt.step(closure)
    assert (float(opt.loss_scale), opt.last_step_skipped) == (2.0 ** 24, False)
    opt.step(closure)
    assert (float(opt.loss_scale), opt.last_step_skipped) == (2.0 ** 24, False)    # the clamp above
    opt.loss_scale.assign(2.0)
    factor["x"] = math.inf
    opt.step(closure)
    assert (float(opt.loss_scale), opt.last_step_skipped) == (1.0, True)
    opt.step(closure)
    assert (float(opt.loss_scale), opt.last_step_skipped, opt.skipped_steps) == (1.0, True, 2)      # the clamp below
    opt.loss_scale.assign(3.0)
    with pytest.raises(ValueError, match="power of two"):
        opt.step(closure)


# ---------------------------------------------------------------------------------------------------------------- checkpoint
def _ckpt_optimizer(psgd, params, **kw):
    return psgd.UVd(params, rank_of_modification=RANK, lr_params=0.05, lr_preconditioner=0.05, grad_clip_max_norm=0.5,
                    preconditioner_update_probability=0.75, momentum=0.9, placement=None, step_tail="fused", **kw)


@pytest.mark.parametrize("exact", [True, False])
def test_checkpoint_after_a_skip_resumes_bit_for_bit(psgd, exact):
    guard = dict(nonfinite="skip", loss_scale="dynamic", loss_scale_growth_interval=2, exact_hessian_vector_product=exact)
    params, a_k, c_k = _problem(torch.float16)
    factor = {"x": 1.0}
    closure = _closure_for(params, a_k, c_k, factor)
    torch.manual_seed(300)
    opt = _ckpt_optimizer(psgd, params, generator=torch.Generator().manual_seed(7), **guard)
    opt.loss_scale.assign(2.0 ** 8)
    for x in (1.0, 1.0, math.inf):
        factor["x"] = x
        opt.step(closure)
    factor["x"] = 1.0
    assert opt.last_step_skipped and opt.skipped_steps == 1 and float(opt.loss_scale) == 2.0 ** 8      # grown once, halved once
    sd, cuda_rng = opt.state_dict(), torch.cuda.get_rng_state()
    saved = [p.detach().clone() for p in params]
    for _ in range(3):
        opt.step(closure)
    # ---- a fresh optimizer on the saved parameters
    params2 = [p.clone().requires_grad_(True) for p in saved]
    closure2 = _closure_for(params2, a_k, c_k, {"x": 1.0})
    torch.manual_seed(999)
    opt2 = _ckpt_optimizer(psgd, params2, generator=torch.Generator().manual_seed(8), **guard)
    opt2.load_state_dict(sd)
    assert (opt2.skipped_steps, float(opt2.loss_scale), opt2._good_steps, opt2._m_step) == (1, 2.0 ** 8, 0, 2)
    torch.cuda.set_rng_state(cuda_rng)
    for _ in range(3):
        opt2.step(closure2)
    assert (opt2.skipped_steps, float(opt2.loss_scale)) == (opt.skipped_steps, float(opt.loss_scale)) == (1, 2.0 ** 9)
    for a, b in zip(params + [opt._U, opt._V, opt._d, opt._momentum_buffer()], params2 + [opt2._U, opt2._V, opt2._d, opt2._momentum_buffer()]):
        assert torch.equal(_bits(a.detach()), _bits(b.detach()))
    # ---- the dict of an unguarded optimizer loads into a guarded one: the guard starts fresh
    plain = _ckpt_optimizer(psgd, [p.clone().requires_grad_(True) for p in saved], generator=torch.Generator().manual_seed(7),
                            exact_hessian_vector_product=exact)
    plain.step(_closure_for(plain._params_with_grad, a_k, c_k, {"x": 1.0}))
    psd = plain.state_dict()
    assert not {"nonfinite", "skipped_steps", "loss_scale", "loss_scale_good_steps"} & set(psd)
    opt2.load_state_dict(psd)
    assert (opt2.skipped_steps, opt2._good_steps, float(opt2.loss_scale), opt2._m_step) == (0, 0, 2.0 ** 9, 1)
    assert torch.equal(_bits(opt2._U), _bits(plain._U))
    assert math.isfinite(float(opt2.step(closure2))) and not opt2.last_step_skipped
