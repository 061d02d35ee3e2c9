"""The three stochastic step-tail kernels (psgd_uvd_param_update_multi_sr, psgd_multi_param_update_sr,
psgd_multi_param_update_mixed_sr) through their wrappers, bit for bit against the torch restatement
(param_update_stochastic_ / stochastic_narrow_bf16), and the statistics that are the point of them: unbiasedness, and a weight
that moves where round to nearest stalls."""
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK, MAX_GRID = 4096, 2048
BF = torch.bfloat16
TINY = float(torch.finfo(BF).tiny)
SPECIALS = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max),
            float(np.finfo(np.float32).tiny), -float(np.finfo(np.float32).tiny), 1e-45, -1e-45, 5e-39]     # tests/test_multi_tail_gpu.py
ENTRIES = ["uvd", "multi", "mixed"]


@pytest.fixture(scope="module")
def m():
    from psgd_tf_amd import _lib
    from psgd_tf_amd import preconditioned_stochastic_gradient_descent as psgd
    assert _lib.UVD_TAIL_CHUNK == CHUNK and _lib.UVD_TAIL_MAX_GRID == MAX_GRID
    return psgd


def _dev():
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _carve(sizes, dtype, shift):
    """tensors of these element counts inside ONE buffer, tensor i starting an ODD number of elements past a 16-byte boundary where
    the dtype is 2 bytes wide (aligned to 2 bytes only), 1 .. 3 floats past one where it is float32; `shift` varies the pattern"""
    per = 16 // torch.empty(0, dtype=dtype).element_size()
    starts, pos = [], 0
    for i, n in enumerate(sizes):
        off = (2 * ((i + shift) % (per // 2)) + 1) % per
        pos = (pos + per - 1) // per * per + off
        starts.append(pos)
        pos += n
    buf = torch.zeros(pos + per, dtype=dtype, device=_dev())
    assert buf.data_ptr() % 16 == 0
    out = [buf[s:s + n] for s, n in zip(starts, sizes)]
    assert all(t.data_ptr() % 4 != 0 for t in out if dtype == BF and t.numel())
    return out


def _fill(ts, gen, scale=1.0, plant=None):
    for t in ts:
        t.copy_((torch.randn(t.numel(), device=_dev(), generator=gen) * scale).to(t.dtype))
        if plant is not None:
            k = min(int(t.numel()), len(plant))
            t[:k] = torch.tensor(plant[:k], device=_dev()).to(t.dtype)
    return ts


def _problem(sizes, seed, mixed, plant=False):
    """parameters and vs bf16 at 2-byte alignment, gradients fp32 (every other one bf16 when mixed), each role in its own buffer"""
    gen = _gen(seed)
    p = _fill(_carve(sizes, BF, 0), gen, plant=SPECIALS if plant else None)
    v = _fill(_carve(sizes, BF, 1), gen, 2.0 ** -6, plant=SPECIALS[3:] + SPECIALS[:3] if plant else None)
    if mixed:
        g = []
        gf, gb = _carve(sizes, torch.float32, 1), _carve(sizes, BF, 2)
        for i in range(len(sizes)):
            g.append(gb[i] if i % 2 else gf[i])
        _fill(g, gen, plant=SPECIALS[5:] + SPECIALS[:5] if plant else None)
    else:
        g = _fill(_carve(sizes, torch.float32, 1), gen, plant=SPECIALS[5:] + SPECIALS[:5] if plant else None)
    return p, g, v


def _f64(x):
    return torch.tensor(float(np.float32(x)), dtype=torch.float64, device=_dev())


def _lr_eff(lr, S, max_norm):
    """what the kernels form from the device double: fl32(lr * min(max_norm / (sqrt(S) + tiny), 1)) in fp64, NaN propagating"""
    if S is None:
        return float(np.float32(lr))
    St = torch.tensor(S, dtype=torch.float64, device=_dev())
    return (_f64(lr) * torch.minimum(_f64(max_norm) / (torch.sqrt(St) + _f64(TINY)), _f64(1.0))).float()


def _reference(m, p, g, v, lr_eff, wd, seed, index0):
    """the torch restatement on clones: the parameters it leaves"""
    out, start = [], 0
    c = None
    if wd != 0.0:
        c = lr_eff * torch.tensor(wd, dtype=torch.float32, device=_dev()) if isinstance(lr_eff, torch.Tensor) \
            else float(np.float32(lr_eff) * np.float32(wd))
    for k, t in enumerate(p):
        q = t.clone()
        m.param_update_stochastic_(q, g[k].float(), None if v is None else v[k], lr_eff, c, seed, index0 + start)
        out.append(q)
        start += int(t.numel())
    return out


def _run(m, p, g, v, lr, S, max_norm, wd, seed, index0):
    """psgd_multi_param_update_sr, or psgd_multi_param_update_mixed_sr when a gradient is bf16, with a host-written sum"""
    sumsq = None if S is None else torch.tensor([S], dtype=torch.float64, device=_dev())
    m.multi_param_update(p, g, v, lr, sumsq, None if S is None else max_norm, None, weight_decay=wd, rounding="stochastic",
                         rounding_seed=seed, index0=index0)


_PLANS = {}


def _run_uvd(m, p, g, v, lr, S, max_norm, wd, seed, index0):
    """psgd_uvd_param_update_multi_sr through the C ABI with OUR device double (uvd_step_tail computes the norm itself; here the
    update alone is under test, as in tests/test_multi_tail_gpu.py)"""
    from psgd_tf_amd import _lib
    sizes = tuple(int(t.numel()) for t in p)
    plan = _PLANS.get(sizes)
    if plan is None:
        plan = _PLANS[sizes] = m.UVdTailPlan(sizes, BF, _dev())
    flat = torch.cat([x.float().reshape(-1) for x in g])
    sumsq = None if S is None else torch.tensor([S], dtype=torch.float64, device=_dev())
    rc = _lib.load().psgd_uvd_param_update_multi_sr(
        plan.table("params", p, "test"), None if v is None else plan.table("vs", v, "test"), len(p), plan.chunks.data_ptr(),
        plan.nchunks, plan.code, flat.data_ptr(), float(lr), None if sumsq is None else sumsq.data_ptr(),
        float(max_norm) if S is not None else 0.0, TINY, float(wd), seed, index0, m._stream_ptr(_dev()))
    _lib.check(rc, "psgd_uvd_param_update_multi_sr")
    torch.cuda.synchronize()


def _go(m, entry, p, g, v, lr, S, max_norm, wd, seed, index0):
    if entry == "uvd":
        _run_uvd(m, p, g, v, lr, S, max_norm, wd, seed, index0)
    else:
        assert any(t.dtype == BF for t in g) == (entry == "mixed")
        _run(m, p, g, v, lr, S, max_norm, wd, seed, index0)


def _raw(t):
    return t.reshape(-1).view(torch.int16 if t.dtype == BF else torch.int32)


def _assert_codes(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        same = a.reshape(-1).view(torch.int16) == b.reshape(-1).view(torch.int16)
        assert bool(same.all()), "%s: tensor %d differs at %s" % (what, i, torch.nonzero(~same)[:4].flatten().tolist())


# ----------------------------------------------------------------------------------------------- bit for bit, every combination
SIZES = [1, 7, 8, 9, 4099]
CLIPS = [None, 4.0e4, float("nan")]       # sumsq absent; a norm of 200 against max_norm 1.5 (clipping); a NaN sumsq


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_combination_matches_the_torch_restatement(m, entry):
    lr, max_norm, seed = 0.0371, 1.5, 0x1234567890ABCDEF
    for with_vs, wd, S in itertools.product([False, True], [0.0, 0.01], CLIPS):
        p, g, v = _problem(SIZES, 1, entry == "mixed")
        v = v if with_vs else None
        untouched = [t.clone() for t in g + (v or [])]
        want = _reference(m, p, g, v, _lr_eff(lr, S, max_norm), wd, seed, 0)
        _go(m, entry, p, g, v, lr, S, max_norm, wd, seed, 0)
        what = "%s vs=%s wd=%s S=%s" % (entry, with_vs, wd, S)
        _assert_codes(p, want, what)
        assert all(torch.equal(_raw(a), _raw(b)) for a, b in zip(g + (v or []), untouched)), what + ": an operand was written"
        if S is not None and math.isnan(S):                  # a NaN sumsq makes every parameter NaN, as in the nearest kernels
            assert all(bool((t.view(torch.int16) == 0x7FC0).all()) for t in p), what
        if S == 4.0e4:
            assert float(_lr_eff(lr, S, max_norm)) < float(np.float32(lr)) * 0.01


@pytest.mark.parametrize("entry", ENTRIES)
def test_grid_stride_second_trip(m, entry):
    sizes = [6] * 2100 + [5000]                              # tests/test_multi_tail_gpu.py: 2102 chunks > 2048 workgroups
    assert sum(-(-n // CHUNK) for n in sizes) > MAX_GRID
    p, g, v = _problem(sizes, 2, entry == "mixed")
    want = _reference(m, p, g, v, float(np.float32(0.05)), 0.01, 99, 0)
    _go(m, entry, p, g, v, 0.05, None, 0.0, 0.01, 99, 0)
    _assert_codes(p, want, entry + " grid stride")


@pytest.mark.parametrize("index0", [12345, 2 ** 32 - 4100, 2 ** 32, 5 * 2 ** 32 + 3])
@pytest.mark.parametrize("entry", ENTRIES)
def test_index0(m, entry, index0):
    """index0 non-zero, across 2^32 inside a tensor, and beyond it"""
    p, g, v = _problem(SIZES + [CHUNK + 3], 3, entry == "mixed")
    want = _reference(m, p, g, v, float(np.float32(0.02)), 0.0, 7, index0)
    other = _reference(m, p, g, v, float(np.float32(0.02)), 0.0, 7, index0 % 2 ** 32)
    _go(m, entry, p, g, v, 0.02, None, 0.0, 0.0, 7, index0)
    _assert_codes(p, want, "%s index0=%d" % (entry, index0))
    if index0 >= 2 ** 32:                                    # the high half of the index enters the hash
        assert not all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(want, other))


@pytest.mark.parametrize("entry", ENTRIES)
def test_special_values(m, entry):
    """+-0, +-Inf, NaN, the largest finite value, subnormals, planted where the tensors start, another special meeting another in
    every role; a NaN result is the quiet NaN 0x7FC0"""
    sizes = [len(SPECIALS), 2 * len(SPECIALS) + 5, 40]
    for with_vs, wd in itertools.product([False, True], [0.0, 0.01]):
        p, g, v = _problem(sizes, 4, entry == "mixed", plant=True)
        v = v if with_vs else None
        want = _reference(m, p, g, v, float(np.float32(0.0371)), wd, 5, 0)
        _go(m, entry, p, g, v, 0.0371, None, 0.0, wd, 5, 0)
        _assert_codes(p, want, "%s specials vs=%s wd=%s" % (entry, with_vs, wd))
        for t in p:
            nan = torch.isnan(t.float())
            assert bool((t.view(torch.int16)[nan] == 0x7FC0).all())


# ------------------------------------------------------------------------------------------------------------------ properties
def _x_of(p, g, v, lr32, c):
    """fl32(w - d) of the chain, per tensor"""
    out = []
    for k, t in enumerate(p):
        w = t.float()
        d = g[k].float() * lr32
        if v is not None:
            d = d + v[k].float()
        if c is not None:
            d = d + w * c
        out.append(w - d)
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_neighbour_property(m, entry):
    """every result is one of the two bf16 neighbours of the fp32 x, and x itself where x is a bf16 value"""
    sizes = SIZES + [2 * CHUNK + 5]
    p, g, v = _problem(sizes, 5, entry == "mixed")
    g[-1].zero_()                                            # the last tensor: x = w, a bf16 value, which must come back as it is
    v[-1].zero_()
    lr32 = float(np.float32(0.0371))
    xs = _x_of(p, g, v, lr32, None)
    _go(m, entry, p, g, v, 0.0371, None, 0.0, 0.0, 17, 0)
    exact = 0
    for t, x in zip(p, xs):
        xb = x.view(torch.int32)
        lo = xb & -65536                                     # towards zero: the bits with the low half cleared
        hi = lo + 65536                                      # away from zero (sign-magnitude: the same for both signs)
        got = t.float().view(torch.int32)
        assert bool(((got == lo) | (got == hi)).all())
        rep = (xb & 0xFFFF) == 0
        assert bool((got[rep] == xb[rep]).all())
        exact += int(rep.sum())
    assert exact >= 2 * CHUNK + 5                            # the second clause was exercised


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_bits_do_not_depend_on_how_the_elements_are_split_into_tensors(m, entry):
    """the same elements with the same global indices: one list of 3 tensors, one of 7 with other boundaries and alignments"""
    n = 2 * CHUNK + 333
    gen = _gen(6)
    P = torch.randn(n, device=_dev(), generator=gen).to(BF)
    G = torch.randn(n, device=_dev(), generator=gen)
    if entry == "mixed":
        G = G.to(BF).float()                                 # exact in both gradient types
    V = (torch.randn(n, device=_dev(), generator=gen) * 2.0 ** -6).to(BF)
    results = []
    for sizes in ([CHUNK + 3, 37, n - CHUNK - 40], [1, 7, 8, 9, 4099, 100, n - 4224]):
        assert sum(sizes) == n
        p, v = _carve(sizes, BF, 0), _carve(sizes, BF, 1)
        if entry == "mixed":
            gf, gb = _carve(sizes, torch.float32, 1), _carve(sizes, BF, 2)
            g = [gb[i] if i % 2 else gf[i] for i in range(len(sizes))]
        else:
            g = _carve(sizes, torch.float32, 1)
        pos = 0
        for k, s in enumerate(sizes):
            p[k].copy_(P[pos:pos + s]); v[k].copy_(V[pos:pos + s]); g[k].copy_(G[pos:pos + s].to(g[k].dtype))
            pos += s
        _go(m, entry, p, g, v, 0.0371, None, 0.0, 0.01, 21, 2 ** 32 - 1000)
        results.append(torch.cat([t.reshape(-1) for t in p]))
    assert torch.equal(results[0].view(torch.int16), results[1].view(torch.int16))
    want = _reference(m, [P.clone()], [G], [V], float(np.float32(0.0371)), 0.01, 21, 2 ** 32 - 1000)[0]
    assert torch.equal(results[0].view(torch.int16), want.view(torch.int16))


def test_wrappers_refuse_other_dtypes(m):
    from psgd_tf_amd import kron_optimizer as ko
    for dt in (torch.float32, torch.float16):
        t = torch.zeros(8, dtype=dt, device=_dev())
        with pytest.raises(ValueError, match="needs bfloat16 parameters"):
            ko.multi_param_update([t], [t.float()], lr=0.1, rounding="stochastic", rounding_seed=1)
        with pytest.raises(ValueError, match="needs bfloat16 parameters"):
            m.uvd_step_tail([t], t.float(), 0.1, rounding="stochastic", rounding_seed=1)


def test_nearest_is_untouched_by_the_new_keywords(m):
    """rounding="nearest" passed explicitly: the entry points and the bits of before"""
    from psgd_tf_amd import kron_optimizer as ko
    p, g, v = _problem(SIZES, 8, False)
    q = [t.clone() for t in p]
    ko.multi_param_update(p, g, v, 0.0371, weight_decay=0.01)
    ko.multi_param_update(q, g, v, 0.0371, weight_decay=0.01, rounding="nearest")
    _assert_codes(p, q, "multi nearest")
    flat = torch.cat([x.reshape(-1) for x in g])
    m.uvd_step_tail(p, flat, 0.0371, vs=v, weight_decay=0.01)
    m.uvd_step_tail(q, flat, 0.0371, vs=v, weight_decay=0.01, rounding="nearest")
    _assert_codes(p, q, "uvd nearest")


# ---------------------------------------------------------------------------------------------------------------- unbiasedness
QS = [1.0 / 32, 1.0 / 2, 31.0 / 32]
N_EL, N_SEEDS = 4096, 256


@pytest.mark.parametrize("entry", ENTRIES)
def test_unbiased_where_nearest_is_not(m, entry):
    """x = 1 + q ulp, ulp = 2^-7 (the bf16 spacing in [1, 2)), formed as w - lr g with w = 1, lr = 1 and g = -q ulp: every step
    exact in fp32, and g (an odd number below 32 times a power of two) exact in bf16 too, for the mixed entry.  n = 4096 elements
    x 256 seeds = 2^20 draws per q.  The low 16 bits of x are q 2^16, so a draw stores 1 + ulp with probability q exactly and
    1 otherwise: the mean of n independent draws has standard deviation ulp sqrt(q (1 - q) / n), and the bound is six of them.
    Round to nearest misses by |q - round(q)| ulp whatever n: 1/32 ulp for q = 1/32 and 31/32, 1/2 ulp for q = 1/2 (the tie goes
    to the even code, 1.0)."""
    ulp = 2.0 ** -7
    n = N_EL * N_SEEDS
    from psgd_tf_amd import kron_optimizer as ko
    for q in QS:
        w0, g0 = 1.0, -q * ulp                               # x = 1 - (1 * (-q ulp)) = 1 + q ulp, every step exact
        assert float(torch.tensor(g0).to(BF)) == g0
        x = w0 - g0
        p = _carve([N_EL], BF, 0)
        g = _carve([N_EL], BF if entry == "mixed" else torch.float32, 1)
        g[0].fill_(g0)
        if entry == "mixed":
            g = g + [torch.zeros(1, device=_dev())]          # a mixed list has both kinds
            p = p + [torch.ones(1, dtype=BF, device=_dev())]
        total = torch.zeros((), dtype=torch.float64, device=_dev())
        for seed in range(N_SEEDS):
            p[0].fill_(w0)
            _go(m, entry, p, g, None, 1.0, None, 0.0, 0.0, 1000 + seed, 0)
            total += p[0].double().sum()
        mean = float(total) / n
        bound = 6.0 * ulp * math.sqrt(q * (1.0 - q) / n)
        print("%s q = %.5f: mean - x = %+.3e ulp, bound %.3e ulp" % (entry, q, (mean - x) / ulp, bound / ulp))
        assert abs(mean - x) <= bound
        p[0].fill_(w0)                                       # the same inputs rounded to nearest
        if entry == "uvd":
            m.uvd_step_tail(p, g[0].float(), 1.0)
        else:
            ko.multi_param_update(p, g, None, 1.0)
        near = float(p[0].double().mean())
        assert abs(near - x) == abs(q - round(q)) * ulp
        assert abs(near - x) > bound                         # the contrast: nearest is outside the bound whatever n


# ----------------------------------------------------------------------------------------------------------------------- stall
@pytest.mark.parametrize("entry", ["multi", "uvd"])
def test_nearest_stalls_and_stochastic_moves(m, entry):
    """4096 bf16 weights at 1.0, lr g = 2^-12 for 256 steps: the sum of the updates is 256 2^-12 = 2^-4.
    Nearest: 1 - 2^-12 lies in [0.5, 1) where the spacing is 2^-8, 2^-12 is 1/16 of it, below half: every step returns 1.0.
    Stochastic: step t of element e moves it from a bf16 value y to one of the neighbours of y - 2^-12, the lower with probability
    qd, E[new] = y - 2^-12 exactly (unbiased), Var[new | y] = ulp(y)^2 qd (1 - qd) <= ulp^2 / 4 with ulp <= 2^-7 throughout (the
    weights stay in (0.5, 2)).  The steps' errors are martingale differences, so after 256 steps Var[w_e] <= 256 2^-14 / 4 = 2^-8,
    and the mean over 4096 independent elements has variance <= 2^-8 / 4096 = 2^-20: sigma <= 2^-10, and the bound is 6 sigma."""
    from psgd_tf_amd import kron_optimizer as ko
    n, steps, upd = 4096, 256, 2.0 ** -12
    g = torch.full((n,), upd, device=_dev())
    for rounding in ("nearest", "stochastic"):
        p = [torch.ones(n, dtype=BF, device=_dev())]
        for t in range(steps):
            kw = dict(rounding="stochastic", rounding_seed=m.uvd_step_rounding_seed(42, t)) if rounding == "stochastic" else {}
            if entry == "multi":
                ko.multi_param_update(p, [g], None, 1.0, **kw)
            else:
                m.uvd_step_tail(p, g, 1.0, **kw)
        if rounding == "nearest":
            assert bool((p[0].view(torch.int16) == 0x3F80).all())                 # every bit unchanged
        else:
            moved = 1.0 - float(p[0].double().mean())
            print("%s: the mean moved by %.6f, expected %.6f, 6 sigma = %.6f" % (entry, moved, steps * upd, 6 * 2.0 ** -10))
            assert abs(moved - steps * upd) <= 6 * 2.0 ** -10
            assert float(p[0].float().min()) > 0.5 and float(p[0].float().max()) <= 1.0
