"""The list kernels of psgd_multi_tail.hip through their wrappers (kron_optimizer.multi_sumsq / multi_param_update /
multi_diff_scale): bit for bit against the torch expressions they replace, on shape lists chosen for the chunk of 4096 elements and the
grid cap of 2048 workgroups."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK, MAX_GRID = 4096, 2048
TINY = float(np.finfo(np.float32).tiny)
SPECIALS = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max),
            TINY, -TINY, 1e-45, -1e-45, 5e-39]                     # ... subnormals last


@pytest.fixture(scope="module")
def ko():
    from psgd_tf_amd import _lib, kron_optimizer
    assert _lib.UVD_TAIL_CHUNK == CHUNK and _lib.UVD_TAIL_MAX_GRID == MAX_GRID
    return kron_optimizer


def _dev():
    return torch.device("cuda:0")


def _carve(sizes, offsets, gen, fill):
    """tensors of these element counts inside ONE buffer, tensor i starting `offsets[i] mod 4` floats past a 16-byte boundary"""
    starts, pos = [], 0
    for n, o in zip(sizes, offsets):
        pos = (pos + 3) // 4 * 4 + o
        starts.append(pos)
        pos += n
    buf = fill(pos + 4, gen)
    assert buf.data_ptr() % 16 == 0
    return [buf[s:s + n] for s, n in zip(starts, sizes)]


def _lists_of(which):
    """(sizes, offsets of the tensors from a 16-byte boundary, shapes or None)"""
    if which == "edges":
        sizes = [1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]
        return sizes, [0] * len(sizes)
    if which == "empty_middle":
        return [7, 0, 9], [0, 0, 0]
    if which == "grid_stride":                     # 2100 + 2 chunks > 2048 workgroups: the second trip of the grid-stride loop
        sizes = [6] * 2100 + [5000]
        assert sum(-(-n // CHUNK) for n in sizes) > MAX_GRID
        return sizes, [(2 * i) % 4 for i in range(len(sizes))]
    if which == "unaligned":                       # vector heads of 3, 2 and 1 elements, bodies that cross chunks
        return [CHUNK + 3, 37, 2 * CHUNK + 8], [1, 2, 3]
    raise KeyError(which)


WHICH = ["edges", "empty_middle", "grid_stride", "unaligned"]


def _randn(n, gen):
    return torch.randn(n, device=_dev(), generator=gen)


def _make(which, seed, roles, plant=True):
    """role -> list of tensors; every role in its own buffer, with its own offsets in the unaligned case (so that the operands of
    one chunk are aligned differently); special values planted where the tensors start and end"""
    sizes, offsets = _lists_of(which)
    gen = torch.Generator(device=_dev()).manual_seed(seed)
    out = {}
    for r, role in enumerate(roles):
        offs = [(o + (r if which == "unaligned" else 0)) % 4 for o in offsets]
        ts = _carve(sizes, offs, gen, _randn)
        if plant:
            vals = torch.tensor(SPECIALS[r:] + SPECIALS[:r], device=_dev())       # another special meets another in every role
            for t in ts:
                m = min(int(t.numel()), len(SPECIALS))
                t[:m] = vals[:m]
                if t.numel() > 2 * len(SPECIALS):
                    t[-m:] = vals[:m].flip(0)
        out[role] = ts
    if which != "grid_stride":                     # rank 2 where that costs nothing: the class hands over matrices
        out = {k: [t.view(1, t.numel()) for t in v] for k, v in out.items()}
    return out


def _assert_bits(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.reshape(-1), b.reshape(-1)
        same = (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))
        assert bool(same.all()), "%s: tensor %d differs at %s" % (what, i, torch.nonzero(~same)[:4].flatten().tolist())


def _f64(x):
    return torch.tensor(float(np.float32(x)), dtype=torch.float64, device=_dev())


# ------------------------------------------------------------------------------------------------------------------- update
@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("which", WHICH)
def test_update_without_clipping(ko, which, with_vs):
    d = _make(which, 1, ("p", "g", "v"))
    lr = 0.0371
    lr32 = float(np.float32(lr))
    if with_vs:
        want = [p - (g * lr32 + v) for p, g, v in zip(d["p"], d["g"], d["v"])]
    else:
        want = [p - g * lr32 for p, g in zip(d["p"], d["g"])]
    untouched = [t.clone() for t in d["g"] + d["v"]]
    ko.multi_param_update(d["p"], d["g"], d["v"] if with_vs else None, lr)
    _assert_bits(d["p"], want, "update")
    _assert_bits(d["g"] + d["v"], untouched, "operands")


@pytest.mark.parametrize("which", WHICH)
def test_perturbation_is_p_plus_v(ko, which):
    d = _make(which, 2, ("p", "v"))
    want = [p + v for p, v in zip(d["p"], d["v"])]
    ko.multi_param_update(d["p"], None, d["v"])
    _assert_bits(d["p"], want, "perturbation")


@pytest.mark.parametrize("with_vs", [False, True])
@pytest.mark.parametrize("S", [0.0, 1e-6, 4.0, 1e12, float("inf"), float("nan")])
@pytest.mark.parametrize("which", ["edges", "unaligned"])
def test_update_with_clipping_from_a_host_written_sum(ko, which, S, with_vs):
    """S is written by the host: the update alone is under test.  lr_eff = fl32(lr * min(max_norm / (sqrt(S) + tiny), 1)) in fp64."""
    d = _make(which, 3, ("p", "g", "v"), plant=not math.isnan(S))
    lr, max_norm = 0.05, 1.5
    St = torch.tensor([S], dtype=torch.float64, device=_dev())
    lr_t = (_f64(lr) * torch.minimum(_f64(max_norm) / (torch.sqrt(St[0]) + _f64(TINY)), _f64(1.0))).float()
    if with_vs:
        want = [p - (g * lr_t + v) for p, g, v in zip(d["p"], d["g"], d["v"])]
    else:
        want = [p - g * lr_t for p, g in zip(d["p"], d["g"])]
    ko.multi_param_update(d["p"], d["g"], d["v"] if with_vs else None, lr, St, max_norm, TINY)
    _assert_bits(d["p"], want, "clipped update")
    if math.isnan(S):                              # torch.minimum propagates the NaN: every parameter is NaN
        assert all(bool(torch.isnan(p).all()) for p in d["p"])
    if S == 0.0:                                   # ... and + tiny keeps a zero norm from dividing by zero: the full step
        assert float(lr_t) == float(np.float32(lr))


def test_update_argument_errors(ko):
    d = _make("empty_middle", 4, ("p", "g"), plant=False)
    with pytest.raises(ValueError, match="needs vs"):
        ko.multi_param_update(d["p"], None, None)
    with pytest.raises(ValueError, match="go together"):
        ko.multi_param_update(d["p"], d["g"], None, 0.1, torch.zeros(1, dtype=torch.float64, device=_dev()))
    with pytest.raises(ValueError, match=r"grads\[2\] has 8 elements"):
        ko.multi_param_update(d["p"], d["g"][:2] + [torch.zeros(8, device=_dev())])
    with pytest.raises(ValueError, match="grads has 2 tensors"):
        ko.multi_param_update(d["p"], d["g"][:2])
    with pytest.raises(ValueError, match="not contiguous"):
        ko.multi_param_update([torch.zeros(4, 6, device=_dev()).t()], [torch.zeros(6, 4, device=_dev())])
    with pytest.raises(TypeError, match="float32"):
        ko.multi_param_update(d["p"], [g.double() for g in d["g"]])


# --------------------------------------------------------------------------------------------------------------------- diff
@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("which", WHICH)
def test_diff_scale(ko, which, with_x):
    d = _make(which, 5, ("a", "b", "h", "v", "x"))
    s = float(ko._FD_INV)
    want_h = [(a - b) * s for a, b in zip(d["a"], d["b"])]
    want_x = [v * s for v in d["v"]] if with_x else [x.clone() for x in d["x"]]
    for t in d["h"] + (d["x"] if with_x else []):
        t.view(torch.int32).fill_(-1)              # 0xFF bytes: the outputs are written, never read
    untouched = [t.clone() for t in d["a"] + d["b"] + d["v"]]
    ko.multi_diff_scale(d["a"], d["b"], d["h"], d["v"] if with_x else None, d["x"] if with_x else None, s)
    _assert_bits(d["h"], want_h, "h")
    _assert_bits(d["x"], want_x, "x")
    _assert_bits(d["a"] + d["b"] + d["v"], untouched, "operands")


# -------------------------------------------------------------------------------------------------------------------- sumsq
def _dyadic(n, gen):
    return torch.randint(-64, 65, (n,), device=_dev(), generator=gen).float() / 16.0


def _fsum_of_squares(tensors):
    """math.fsum of the float32-rounded squares: the exact sum of what the kernel adds"""
    vals = []
    for t in tensors:
        vals.extend((t * t).double().reshape(-1).cpu().tolist())
    return math.fsum(vals), len(vals)


@pytest.mark.parametrize("which", WHICH)
def test_sumsq_dyadic_is_exact(ko, which):
    """values j / 16, |j| <= 64: every square is a multiple of 2^-8 below 2^5 and every partial sum is exact in fp64, whatever the
    order: the result is THE sum"""
    sizes, offsets = _lists_of(which)
    ts = _carve(sizes, offsets, torch.Generator(device=_dev()).manual_seed(6), _dyadic)
    want, _ = _fsum_of_squares(ts)
    out = ko.multi_sumsq(ts)
    assert float(out[0]) == want


@pytest.mark.parametrize("which", WHICH)
def test_sumsq_random_bound_repeatable_and_workspace_guard(ko, which):
    from psgd_tf_amd import _lib
    sizes, offsets = _lists_of(which)
    ts = _carve(sizes, offsets, torch.Generator(device=_dev()).manual_seed(7), _randn)
    want, n = _fsum_of_squares(ts)
    W, guard = _lib.MULTI_SUMSQ_WS_BYTES, 4096
    ws = torch.full((W + guard,), 0xA5, dtype=torch.uint8, device=_dev())
    out = torch.full((3,), float("nan"), dtype=torch.float64, device=_dev())
    ko.multi_sumsq(ts, out=out[1:2], ws=ws)
    first = float(out[1])
    print("sumsq %s: n = %d, relative error %.3e, bound %.3e" % (which, n, abs(first - want) / want, n * 2.0 ** -53))
    assert abs(first - want) <= n * 2.0 ** -53 * want           # fp64 recursive summation of n non-negative terms, worst case
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2]))               # one double is written
    assert bool((ws[W:] == 0xA5).all()), "bytes past PSGD_MULTI_SUMSQ_WS_BYTES were written"
    again = ko.multi_sumsq(ts)                                                   # another workspace (the plan's), the same bits
    assert float(again[0]) == first
    assert float(ko.multi_sumsq(ts)[0]) == first


def test_sumsq_of_empty_tensors_is_zero(ko):
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=_dev())
    ko.multi_sumsq([torch.zeros(0, 3, device=_dev()), torch.zeros(0, device=_dev())], out=out)
    assert float(out[0]) == 0.0
