"""The two typed list kernels of psgd_multi_tail.hip (psgd_multi_widen_check, psgd_multi_param_update_t) through their wrappers
(kron_optimizer.multi_widen_check, multi_param_update on bfloat16 / float16 parameters): bit for bit against the torch expressions

    widen    dst = src.float() * scale
    update   delta = (g * lr_eff).to(T);  delta = delta + v;  delta = delta + (p.float() * c).to(T);  p = p - delta
             (c = float32(lr_eff * wd); torch rounds every one of these operations to its result type on its own)

on sizes around the chunk of 4096 elements and the 16-byte body, every start alignment of the T and of the fp32 operand, a list
that needs a second trip of the grid-stride loop (cap: 2048 workgroups), and with guard bands around every tensor.  The non-finite
values here are data that the kernels must report, not faults."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK, MAX_GRID = 4096, 2048
SIZES = [0, 1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
BAND = 32                                        # guard elements in front of and behind every tensor


@pytest.fixture(scope="module")
def ko():
    from psgd_tf_amd import _lib, kron_optimizer
    assert _lib.UVD_TAIL_CHUNK == CHUNK and _lib.UVD_TAIL_MAX_GRID == MAX_GRID
    return kron_optimizer


def _dev():
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return bool(((_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


class _Carved:
    """a contiguous tensor of n elements that starts `off` elements past a 16-byte boundary, inside a larger buffer whose other
    elements are a guard band (allocations of the caching allocator start on 512-byte boundaries)"""

    def __init__(self, n, off, dtype, values):
        per16 = 16 // torch.empty((), dtype=dtype).element_size()
        self.start = BAND - BAND % per16 + off
        self.buf = torch.full((self.start + n + BAND,), 7.0, dtype=dtype, device=_dev())
        assert self.buf.data_ptr() % 16 == 0
        self.t = self.buf[self.start:self.start + n]
        self.t.copy_(values)
        assert self.t.is_contiguous()
        assert n == 0 or (self.t.data_ptr() % 16) // self.t.element_size() == off % per16      # (an empty view has no pointer)
        self.before = self.buf.clone()

    def band_untouched(self):
        n = self.t.numel()
        return (torch.equal(_bits(self.buf[:self.start]), _bits(self.before[:self.start]))
                and torch.equal(_bits(self.buf[self.start + n:]), _bits(self.before[self.start + n:])))

    def unchanged(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


def _values(n, dtype, gen, scale=1.0):
    return (torch.randn(n, device=_dev(), generator=gen) * scale).to(dtype)


def _specials(dtype, finite_only=False):
    """+-0, the largest and smallest normals, the subnormals' ends and a few values between; +-Inf and NaN unless finite_only"""
    fi = torch.finfo(dtype)
    sub = fi.smallest_normal * fi.eps                                                  # the smallest subnormal
    vals = [0.0, -0.0, fi.max, -fi.max, fi.smallest_normal, -fi.smallest_normal, sub, -sub, fi.smallest_normal - sub, 3 * sub,
            1.0, -1.5, 1.0 + fi.eps, 0.333]
    if not finite_only:
        vals += [float("inf"), -float("inf"), float("nan")]
    return torch.tensor(vals, dtype=torch.float64).to(dtype).to(_dev())


def _flag(value=0):
    return torch.tensor([value], dtype=torch.int32, device=_dev())


# ------------------------------------------------------------------------------------------------------------------- widen
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_widen_special_values_and_scales(ko, dtype):
    """1, 2^-8 and 2^8: a finite bfloat16 value overflows float32 under 2^8 (max bf16 ~ 3.4e38), no finite float16 value does
    (65504 * 256 is a float32); Inf and NaN inputs are covered directly.  The flag follows the written values."""
    for finite_only in (True, False):
        src = _specials(dtype, finite_only)
        for k, scale in enumerate((1.0, 2.0 ** -8, 2.0 ** 8)):
            want = src.float() * scale
            dst = torch.full((src.numel(),), float("nan"), device=_dev())
            flag = _flag(40)
            ko.multi_widen_check([[src]], [[dst]], [scale], flag=flag, stamp=41 + k)
            assert _same(dst, want), (dtype, scale, dst, want)
            assert bool(torch.equal(_bits(dst[:2]), _bits(want[:2])))                   # the signs of the zeros
            bad = not bool(torch.isfinite(want).all())
            assert (int(flag.item()) == 41 + k) == bad, (dtype, scale, finite_only)
            if finite_only:
                assert bad == (dtype == torch.bfloat16 and scale == 2.0 ** 8)
                if scale == 1.0:
                    assert bool((dst.double() == src.double()).all())                   # widening alone is exact


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_widen_sizes_and_alignments(ko, dtype, n):
    """the T source starts 0 .. 7 elements past a 16-byte boundary, the fp32 destination 0 .. 3 floats past one, independently;
    destinations poisoned with NaN, guard bands around both: nothing outside is written, everything inside is"""
    gen = _gen(100 + n)
    vals = _values(n, dtype, gen, 3.0)
    poison = torch.full((n,), float("nan"), device=_dev())
    want = vals.float() * 0.25
    for soff in range(8):
        for doff in range(4):
            src, dst = _Carved(n, soff, dtype, vals), _Carved(n, doff, torch.float32, poison)
            flag = _flag(5)
            ko.multi_widen_check([[src.t]], [[dst.t]], [0.25], flag=flag, stamp=6)
            assert _same(dst.t, want), (n, soff, doff)
            assert not bool(torch.isnan(dst.t).any())
            assert src.unchanged() and dst.band_untouched(), (n, soff, doff)
            assert int(flag.item()) == 5


def _small_lists(dtype, nlists, seed):
    """2100 tensors of 1 .. 3 elements: more chunks than workgroups, the last ones are reached on the second trip of the loop"""
    sizes = [1 + i % 3 for i in range(2100)]
    assert len(sizes) > MAX_GRID
    gen = _gen(seed)
    total = sum(sizes)
    out = []
    for j in range(nlists):
        flat_t, flat_f = _values(total + 8, dtype, gen), torch.full((total + 4,), float("nan"), device=_dev())
        ts, fs, at = [], [], 0
        for n in sizes:
            ts.append(flat_t[at + j:at + j + n])
            fs.append(flat_f[at + j:at + j + n])
            at += n
        out.append((ts, fs))
    return sizes, out


@pytest.mark.parametrize("nlists", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_widen_absent_lists_and_the_grid_stride_loop(ko, dtype, nlists):
    sizes, lists = _small_lists(dtype, nlists, 7)
    scales = [2.0 ** -8, 0.5, 1.0][:nlists]
    flag = _flag(1)
    ko.multi_widen_check([ts for ts, _ in lists], [fs for _, fs in lists], scales, flag=flag, stamp=2)
    assert int(flag.item()) == 1
    for (ts, fs), s in zip(lists, scales):
        for i in (0, 1, 2, 1000, 2047, 2048, 2049, 2098, 2099):
            assert _same(fs[i], ts[i].float() * s), i
        assert _same(torch.cat(fs), torch.cat(ts).float() * s)
    # a single bad element in a tensor that only the second trip reaches, in each list position
    for j in range(nlists):
        ts = lists[j][0]
        old = ts[2099][-1].clone()
        ts[2099][-1] = float("nan")
        flag = _flag(1)
        ko.multi_widen_check([t for t, _ in lists], [f for _, f in lists], scales, flag=flag, stamp=3 + j)
        assert int(flag.item()) == 3 + j, j
        ts[2099][-1] = old
    flag = _flag(1)
    ko.multi_widen_check([t for t, _ in lists], [f for _, f in lists], scales, flag=flag, stamp=9)
    assert int(flag.item()) == 1                                                          # clean again: the old word stays


@pytest.mark.parametrize("value", [float("inf"), float("nan")])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_widen_flag_placements(ko, dtype, value):
    """three lists of three tensors (head, tail, several chunks): unset on finite data, set by one bad element in each list, in the
    first element, in a scalar head, and in the last element of the last chunk; without a flag a list with scale 1 still widens"""
    sizes = [CHUNK + 3, 37, 2 * CHUNK + 5]
    gen = _gen(31)
    srcs = [[_Carved(n, (3 * j + i) % 8, dtype, _values(n, dtype, gen)) for i, n in enumerate(sizes)] for j in range(3)]
    dsts = [[_Carved(n, (j + i + 1) % 4, torch.float32, torch.full((n,), float("nan"), device=_dev())) for i, n in enumerate(sizes)]
            for j in range(3)]
    S, D = [[c.t for c in l] for l in srcs], [[c.t for c in l] for l in dsts]
    scales = [2.0 ** -4, 2.0 ** -4, 1.0]
    want = [[x.float() * s for x in l] for l, s in zip(S, scales)]
    flag = _flag(10)
    ko.multi_widen_check(S, D, scales, flag=flag, stamp=11)
    assert int(flag.item()) == 10
    assert all(_same(d, w) for ld, lw in zip(D, want) for d, w in zip(ld, lw))
    assert all(c.band_untouched() for l in dsts for c in l) and all(c.unchanged() for l in srcs for c in l)
    stamp = 11
    for j in range(3):
        for i, e in ((0, 0), (1, 0), (1, sizes[1] - 1), (2, CHUNK), (2, sizes[2] - 1)):
            old = S[j][i][e].clone()
            S[j][i][e] = value
            stamp += 1
            ko.multi_widen_check(S, D, scales, flag=flag, stamp=stamp)
            assert int(flag.item()) == stamp, (j, i, e)
            assert not bool(torch.isfinite(D[j][i][e]))
            S[j][i][e] = old
    ko.multi_widen_check(S, D, scales, flag=flag, stamp=stamp + 1)
    assert int(flag.item()) == stamp
    for d in D[2]:
        d.fill_(float("nan"))
    ko.multi_widen_check([S[2]], [D[2]], [1.0])                                          # scale 1, no flag
    assert all(_same(d, x.float()) for d, x in zip(D[2], S[2]))


# ------------------------------------------------------------------------------------------------------------------ update
LR, WD, MAX_NORM = 0.05, 0.01, 2.0


def _lr_eff(sumsq, tiny):
    f64 = lambda x: torch.tensor(float(np.float32(x)), dtype=torch.float64, device=_dev())
    return (f64(LR) * torch.minimum(f64(MAX_NORM) / (torch.sqrt(sumsq[0]) + f64(tiny)), f64(1.0))).float()


def _want_update(p, g, v, lr_eff, wd):
    """the chain, one torch op per rounding; lr_eff: a float32 value as a Python float, or a 0-d float32 device tensor"""
    T = p.dtype
    delta = (g * lr_eff).to(T)
    if v is not None:
        delta = delta + v
    if wd:
        c = lr_eff * torch.tensor(wd, dtype=torch.float32, device=_dev()) if isinstance(lr_eff, torch.Tensor) \
            else float(np.float32(lr_eff) * np.float32(wd))
        delta = delta + (p.float() * c).to(T)
    return p - delta


def _operands(sizes, dtype, seed, poff=lambda i: i % 8, goff=lambda i: i % 4, voff=lambda i: (i + 3) % 8):
    gen = _gen(seed)
    P, G, V = [], [], []
    for i, n in enumerate(sizes):
        pv, gv, vv = _values(n, dtype, gen, 0.5), torch.randn(n, device=_dev(), generator=gen) * 4.0, _values(n, dtype, gen, 0.03)
        for e in {0, n // 2, n - 1} if n else ():                                        # zeros of both signs where they meet
            pv[e], gv[e], vv[e] = -0.0, -0.0, -0.0
        if n > 2:
            pv[1], gv[1] = 0.0, -0.0
        P.append(_Carved(n, poff(i), dtype, pv))
        G.append(_Carved(n, goff(i), torch.float32, gv))
        V.append(_Carved(n, voff(i), dtype, vv))
    return P, G, V


@pytest.mark.parametrize("wd", [0.0, WD])
@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_update_all_forms(ko, dtype, clip, with_vs, wd):
    """the eight combinations of {clip, vs, wd} on one list of all the sizes; wd == 0 is the chain without the decay term"""
    P, G, V = _operands(SIZES, dtype, 50)
    tiny = torch.finfo(dtype).tiny
    sumsq = torch.tensor([37.5 ** 2], dtype=torch.float64, device=_dev()) if clip else None
    lr_eff = _lr_eff(sumsq, tiny) if clip else float(np.float32(LR))
    if clip:
        assert float(lr_eff) < float(np.float32(LR))
    want = [_want_update(p.t, g.t, v.t if with_vs else None, lr_eff, wd) for p, g, v in zip(P, G, V)]
    ko.multi_param_update([p.t for p in P], [g.t for g in G], [v.t for v in V] if with_vs else None, LR, sumsq,
                          MAX_NORM if clip else None, None, weight_decay=wd)
    for i, (p, w) in enumerate(zip(P, want)):
        assert _same(p.t, w), (SIZES[i], (_bits(p.t) != _bits(w)).nonzero().flatten()[:5])
        assert p.band_untouched(), SIZES[i]
    assert all(g.unchanged() for g in G) and all(v.unchanged() for v in V)
    moved = sum(int((_bits(p.t) != _bits(p.before[p.start:p.start + p.t.numel()])).sum()) for p in P)
    assert moved > 0.9 * sum(SIZES)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_perturbation_and_a_nan_norm(ko, dtype):
    P, G, V = _operands(SIZES, dtype, 51)
    want = [p.t + v.t for p, v in zip(P, V)]
    ko.multi_param_update([p.t for p in P], None, [v.t for v in V])
    assert all(_same(p.t, w) for p, w in zip(P, want)) and all(p.band_untouched() for p in P)
    assert all(v.unchanged() for v in V)
    nan = torch.tensor([float("nan")], dtype=torch.float64, device=_dev())
    ko.multi_param_update([p.t for p in P], [g.t for g in G], None, LR, nan, MAX_NORM, None, weight_decay=WD)
    assert all(bool(torch.isnan(p.t).all()) for p in P)                                 # a NaN norm makes every parameter NaN
    assert all(p.band_untouched() for p in P)


@pytest.mark.parametrize("n", SIZES[1:])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_update_sizes_and_alignments(ko, dtype, n):
    """the parameter starts 0 .. 7 elements past a 16-byte boundary, the fp32 gradient 0 .. 3 floats past one, independently (vs
    takes yet another start); the full chain with vs and weight decay"""
    for poff in range(8):
        for goff in range(4):
            P, G, V = _operands([n], dtype, 60 + n, lambda i: poff, lambda i: goff, lambda i: (poff + 2 * goff + 1) % 8)
            want = _want_update(P[0].t, G[0].t, V[0].t, float(np.float32(LR)), WD)
            ko.multi_param_update([P[0].t], [G[0].t], [V[0].t], LR, weight_decay=WD)
            assert _same(P[0].t, want), (n, poff, goff)
            assert P[0].band_untouched() and G[0].unchanged() and V[0].unchanged(), (n, poff, goff)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_update_on_the_grid_stride_loop(ko, dtype):
    sizes, ((P, G),) = _small_lists(dtype, 1, 9)
    gen = _gen(10)
    for g in G:
        g.copy_(torch.randn(g.numel(), device=_dev(), generator=gen))
    want = [_want_update(p, g, None, float(np.float32(LR)), WD) for p, g in zip(P, G)]
    ko.multi_param_update(P, G, None, LR, weight_decay=WD)
    assert _same(torch.cat(P), torch.cat(want))
    assert _same(P[2099], want[2099]) and not _same(P[2099], P[2099] * 0)
