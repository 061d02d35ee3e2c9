"""UVd checkpoints on the GPU: the fp32 -> bf16 narrowing kernel (psgd_uvd_bf16_narrow_f32) and UVd.state_dict / load_state_dict.

  1. narrowing, nearest: bit-equal to torch's fp32 -> bfloat16 on every non-NaN element for every head / body / tail split, NaN
     stays NaN, the guard elements around dst untouched;
  2. narrowing, stochastic: floor or ceil, exact on the grid, independent of the chunking (also past 2^33), seeds and tensor ids
     move the stream, the stream is the family's own (the d update of update_precond_UVd_math_ on a case whose fp32 values the host
     reproduces), and unbiased within the binomial bound 0.25 +- 5 sqrt(0.25 * 0.75 / 65536);
  3. - 5. a run interrupted after 3 of 6 steps, saved, loaded into a NEW optimizer (other generator seed, other hyper-parameters)
     and continued is bit-identical to the uninterrupted run: fp32, widen-route bf16 and native bf16 states, the fused tail, a
     placed state (which stays in its arena);
  6. an fp32 checkpoint into a native bf16 state: the codes, the independence of the staging size, and the memory bound;
  7. the same round trip on the row-sharded native optimizer under a 1-rank process group;
  8. a resharded checkpoint's rows on the device;
  9. the documented errors.
"""
import io
import math

import numpy as np
import pytest
import torch

from tests.uvd_cases import TINY32

pytestmark = pytest.mark.gpu

GUARD = 16                                     # guard elements on each side of dst
BEEF = 0xBEEF - 0x10000                        # 0xBEEF as int16


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import psgd_tf_amd.preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


def _codes(t):
    """the 16-bit codes of a bfloat16 tensor as non-negative int64 on the host"""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF


def _bits32(x):
    return x.detach().cpu().contiguous().numpy().view(np.uint32).astype(np.int64)


def _bitwise(t):
    t = t.detach()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bitwise(a).cpu(), _bitwise(b).cpu())


def _narrow(lib, src, dst, index0=0, tensor=0, rounding=0, seed=0):
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.numel() == dst.numel()
    rc = lib.psgd_uvd_bf16_narrow_f32(src.data_ptr(), dst.data_ptr(), src.numel(), index0, tensor, rounding, seed,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dst


def _floor_or_ceil(x, codes):
    """every code is one of the two bf16 neighbours of its fp32 value; a value on the grid is stored exactly"""
    b = _bits32(x).reshape(-1)
    lo = b >> 16
    codes = codes.reshape(-1)
    assert np.all((codes == lo) | (codes == lo + 1))
    on_grid = (b & 0xFFFF) == 0
    assert np.all(codes[on_grid] == lo[on_grid])
    return on_grid


# ------------------------------------------------------------------------------------------------ 1. the kernel, nearest
SPECIALS = (float("nan"), 0.0, -0.0, float("inf"), -float("inf"), 3.4028234663852886e38, -3.4028234663852886e38,
            1e-45, -1e-45, 1e-40, -3e-39)
_values = {}


def _test_values(n):
    """randn scaled over 1e-30 .. 1e30 with the special values in front: made once, never changed"""
    if n not in _values:
        g = torch.Generator().manual_seed(1234)
        x = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 60.0 - 30.0)
        k = min(n, len(SPECIALS))
        x[:k] = torch.tensor(SPECIALS[:k])
        _values[n] = x
    return _values[n]


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("count", [0, 1, 7, 8, 9, 63, 64, 65, 4099])
def test_narrow_nearest(hip_lib, count, offset):
    host = _test_values(count)
    src_buf = torch.zeros(count + offset + 8, device=_dev())
    src = src_buf[offset:offset + count]
    src.copy_(host)
    dst_buf = torch.full((count + offset + 2 * GUARD,), BEEF, dtype=torch.int16, device=_dev())
    dst = dst_buf.view(torch.bfloat16)[GUARD + offset:GUARD + offset + count]
    assert src_buf.data_ptr() % 16 == 0 and dst_buf.data_ptr() % 16 == 0
    if count == 0:          # a no-op that returns OK (the pointers of an empty view are never read)
        assert hip_lib.psgd_uvd_bf16_narrow_f32(src_buf.data_ptr(), dst_buf.data_ptr(), 0, 0, 0, 0, 0,
                                                torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
    else:
        assert src.data_ptr() % 16 == (4 * offset) % 16 and dst.data_ptr() % 16 == (2 * offset) % 16
        _narrow(hip_lib, src, dst, rounding=0)
    got = _codes(dst)
    want = _codes(host.to(torch.bfloat16))
    nan = torch.isnan(host).numpy()
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all(((got[nan] & 0x7F80) == 0x7F80) & ((got[nan] & 0x7F) != 0))          # a NaN stays a NaN
    whole = dst_buf.cpu().numpy()
    assert np.all(whole[:GUARD + offset] == BEEF) and np.all(whole[GUARD + offset + count:] == BEEF)


# ------------------------------------------------------------------------------------------------ 2. the kernel, stochastic
def _stochastic_input(n=4099):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 20.0 - 10.0)
    x[::5] = x[::5].to(torch.bfloat16).float()                     # every fifth value sits on the bf16 grid
    return x


def test_narrow_stochastic_floor_or_ceil(hip_lib):
    host = _stochastic_input()
    src = host.to(_dev())
    dst = torch.empty(host.numel(), dtype=torch.bfloat16, device=_dev())
    got = _codes(_narrow(hip_lib, src, dst, rounding=1, seed=5))
    on_grid = _floor_or_ceil(host, got)
    assert on_grid.sum() >= host.numel() // 5
    lo = _bits32(host) >> 16
    share_up = float(np.mean(got[~on_grid] == lo[~on_grid] + 1))
    assert 0.3 < share_up < 0.7, share_up                          # both neighbours are in use (the mean fractional part is 1/2)


@pytest.mark.parametrize("index0", [0, 2 ** 33 + 5])
def test_narrow_stochastic_does_not_depend_on_the_chunks(hip_lib, index0):
    host = _stochastic_input()
    src = host.to(_dev())
    one = torch.empty(4099, dtype=torch.bfloat16, device=_dev())
    _narrow(hip_lib, src, one, index0=index0, tensor=1, rounding=1, seed=9)
    parts = torch.empty(4099, dtype=torch.bfloat16, device=_dev())
    lo = 0
    for n in (1000, 2048, 1051):
        _narrow(hip_lib, src[lo:lo + n], parts[lo:lo + n], index0=index0 + lo, tensor=1, rounding=1, seed=9)
        lo += n
    assert lo == 4099 and np.array_equal(_codes(one), _codes(parts))
    if index0:          # the high word of the index is part of the counter: 2^33 + 5 is not 5
        low = torch.empty(4099, dtype=torch.bfloat16, device=_dev())
        _narrow(hip_lib, src, low, index0=index0 % 2 ** 32, tensor=1, rounding=1, seed=9)
        assert not np.array_equal(_codes(one), _codes(low))


def test_narrow_stochastic_seeds_and_tensor_ids(hip_lib):
    host = _stochastic_input()
    src = host.to(_dev())
    runs = {}
    for tensor, seed in ((0, 1), (0, 2), (1, 1), (2, 1), (0, 1 + 2 ** 63)):
        dst = torch.empty(4099, dtype=torch.bfloat16, device=_dev())
        runs[(tensor, seed)] = _codes(_narrow(hip_lib, src, dst, tensor=tensor, rounding=1, seed=seed))
    keys = list(runs)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(runs[a], runs[b]), (a, b)
    again = torch.empty(4099, dtype=torch.bfloat16, device=_dev())
    assert np.array_equal(_codes(_narrow(hip_lib, src, again, tensor=0, rounding=1, seed=1)), runs[(0, 1)])


def test_narrow_stochastic_is_the_familys_stream(psgd, hip_lib):
    """The d update of the family (k_d_update: d <- narrow(d - mu d nablaD), stream (seed, tensor 2, row)) on a case whose fp32
    values the host reproduces exactly: U = V = 0, so nablaD = (d h)^2 - (v / d)^2 (psgd.py:569-581); d, h, v are powers of two
    and every row has h = 0 or v = 0, so nablaD is +- a power of two, mu d nablaD is exact and d - mu d nablaD is rounded
    once whether or not the compiler fuses it; mu = step / (max|nablaD| + tiny) is two fp32 operations."""
    n, r, step, seed = 4096, 4, 0.01, 12345
    g = torch.Generator().manual_seed(3)
    dd = torch.pow(2.0, torch.randint(-1, 2, (n, 1), generator=g).float())
    mag = torch.pow(2.0, torch.randint(-2, 3, (n, 1), generator=g).float())
    pick = torch.rand(n, 1, generator=g) < 0.5
    h = torch.where(pick, mag, torch.zeros(n, 1))
    v = torch.where(pick, torch.zeros(n, 1), mag)
    nab = ((dd * h) ** 2 - (v / dd) ** 2).numpy().astype(np.float32)                 # exact: +- powers of two
    mu = np.float32(step) / (np.float32(np.abs(nab).max()) + np.float32(TINY32))
    d64 = dd.numpy().astype(np.float64) * (1.0 - np.float64(mu) * nab.astype(np.float64))    # exact in fp64 ...
    x = torch.from_numpy(d64.astype(np.float32))                                    # ... rounded to fp32 once
    assert float((x != dd).float().mean()) > 0.99
    dev = _dev()
    U = torch.zeros(n, r, dtype=torch.bfloat16, device=dev)
    V = torch.zeros(n, r, dtype=torch.bfloat16, device=dev)
    d = dd.to(dev).to(torch.bfloat16)
    psgd.update_precond_UVd_math_(U, V, d, v.to(dev), h.to(dev), step, TINY32, balance=False, update_U=True,
                                  rounding="stochastic", rounding_seed=seed)
    mine = torch.empty(n, dtype=torch.bfloat16, device=dev)
    _narrow(hip_lib, x.reshape(-1).to(dev), mine, index0=0, tensor=2, rounding=1, seed=seed)
    family = _codes(d).reshape(-1)
    _floor_or_ceil(x, family)                                                       # the host values are the kernel's values
    assert np.array_equal(_codes(mine), family)
    other = torch.empty(n, dtype=torch.bfloat16, device=dev)
    _narrow(hip_lib, x.reshape(-1).to(dev), other, index0=0, tensor=2, rounding=1, seed=seed + 1)
    assert not np.array_equal(_codes(other), family)                                # and the case can tell streams apart


def test_narrow_stochastic_is_unbiased(hip_lib):
    """65536 copies of 1 + 2^-9, a quarter of the way between two codes: the share stored upward is binomial(65536, 1/4)"""
    n = 65536
    src = torch.full((n,), 1.0 + 2.0 ** -9, device=_dev())
    dst = torch.empty(n, dtype=torch.bfloat16, device=_dev())
    got = _codes(_narrow(hip_lib, src, dst, tensor=2, rounding=1, seed=2024))
    assert np.all((got == 0x3F80) | (got == 0x3F81))
    share = float(np.mean(got == 0x3F81))
    print("share stored upward: %.5f" % share)
    assert abs(share - 0.25) <= 5.0 * math.sqrt(0.25 * 0.75 / n)


# ------------------------------------------------------------------------------------------------ 3. - 5. the round trip
KINDS = {
    "fp32": {},
    "widen": dict(state_dtype=torch.bfloat16),
    "native": dict(state_dtype=torch.bfloat16, state_route="native", state_rounding="stochastic"),
}
SIZES = (777, 1021)
_problem = {}


def _fresh_params(sizes=SIZES):
    if sizes not in _problem:
        g = torch.Generator().manual_seed(21)
        _problem[sizes] = ([torch.randn(n, generator=g) * 0.5 for n in sizes], [torch.rand(n, generator=g) + 0.5 for n in sizes])
    w0, c = _problem[sizes]
    return [w.to(_dev()).requires_grad_(True) for w in w0], [x.to(_dev()) for x in c]


def _closure(params, c):
    m = min(p.numel() for p in params)

    def loss():
        out = sum(0.5 * (ci * p * p).sum() for p, ci in zip(params, c))
        if len(params) > 1:
            out = out + 0.05 * (params[0][:m] * params[1][:m]).sum()
        return out
    return loss


def _make(psgd, kind, params, seed=5, r=10, **kw):
    args = dict(rank_of_modification=r, lr_params=0.05, lr_preconditioner=0.05, grad_clip_max_norm=0.5,
                preconditioner_update_probability=0.5, generator=torch.Generator().manual_seed(seed), placement=None)
    args.update(KINDS[kind])
    args.update(kw)
    torch.cuda.manual_seed(7)                    # the initial U, V of psgd.py:688-689 come from the global generator
    return psgd.UVd(params, **args)


def _make_other(psgd, kind, params, **kw):
    """a NEW optimizer for the resumed half: another generator seed and other hyper-parameters, all of which the load replaces"""
    return _make(psgd, kind, params, seed=99, lr_params=0.2, lr_preconditioner=0.3, grad_clip_max_norm=None,
                 preconditioner_update_probability=1.0, exact_hessian_vector_product=False, **kw)


def _steps(opt, closure, ks):
    for k in ks:
        torch.cuda.manual_seed(100 + k)          # the global generator (the probe vectors) is the caller's business
        opt.step(closure)


def _snapshot(opt, params):
    return [t.detach().clone() for t in (opt._U, opt._V, opt._d)] + [p.detach().clone() for p in params]


def _through_torch_save(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


class _Coins:
    """records every coin the run flips (update_Q of :703 and the two branches of :562 / :588), in order"""

    def __init__(self, monkeypatch, psgd):
        from psgd_tf_amd import sharded
        self.seen = []
        real, real_draw = psgd._draw_branch, sharded.BranchRng.draw

        def draw_branch(p, generator):
            self.seen.append((p, real(p, generator)))
            return self.seen[-1][1]

        def draw(rng, p):
            self.seen.append((p, real_draw(rng, p)))
            return self.seen[-1][1]
        monkeypatch.setattr(psgd, "_draw_branch", draw_branch)
        monkeypatch.setattr(sharded.BranchRng, "draw", draw)

    def take(self):
        out, self.seen = self.seen, []
        return out


_runs = {}


def _reference_and_half(psgd, coins, kind, **kw):
    """(the uninterrupted run's final tensors and coins, the state dict after 3 steps, the parameters after 3 steps): once per case"""
    key = (kind,) + tuple(sorted((k, str(v)) for k, v in kw.items() if k != "group")) + (("group",) if "group" in kw else ())
    if key not in _runs:
        params, c = _fresh_params()
        opt = _make(psgd, kind, params, **kw)
        coins.take()
        _steps(opt, _closure(params, c), range(6))
        ref = (_snapshot(opt, params), coins.take())
        params, c = _fresh_params()
        opt = _make(psgd, kind, params, **kw)
        _steps(opt, _closure(params, c), range(3))
        first = coins.take()
        _runs[key] = (ref, _through_torch_save(opt.state_dict()), [p.detach().clone() for p in params], first)
    return _runs[key]


def _resume(psgd, kind, sd, params3, **kw):
    _, c = _fresh_params()
    params = [p.clone().requires_grad_(True) for p in params3]
    opt = _make_other(psgd, kind, params, **kw)
    opt.load_state_dict(sd)
    return opt, params, _closure(params, c)


def _check_round_trip(psgd, monkeypatch, kind, **kw):
    coins = _Coins(monkeypatch, psgd)
    (want, want_coins), sd, params3, first = _reference_and_half(psgd, coins, kind, **kw)
    opt, params, closure = _resume(psgd, kind, sd, params3, **kw)
    assert float(opt.lr_params) == 0.05 and float(opt.lr_preconditioner) == 0.05 and float(opt.grad_clip_max_norm) == 0.5
    assert float(opt.preconditioner_update_probability) == 0.5 and bool(opt.exact_hessian_vector_product) is True
    coins.take()
    _steps(opt, closure, range(3, 6))
    got = _snapshot(opt, params)
    assert len(first) >= 3 and first + coins.take() == want_coins        # the sequence of update_Q (and branch) coins
    assert {q for p, q in want_coins if p == 0.5} == {True, False}       # both outcomes occurred: the sequence can differ
    for name, a, b in zip(("U", "V", "d", "w0", "w1"), got, want):
        assert _same_bits(a, b), name
    return opt, sd


@pytest.mark.parametrize("kind,tail", [("fp32", "torch"), ("widen", "torch"), ("native", "torch"), ("native", "fused")])
def test_round_trip_is_bit_identical(psgd, monkeypatch, kind, tail):
    opt, sd = _check_round_trip(psgd, monkeypatch, kind, step_tail=tail)
    assert sd["format"] == 1 and sd["rank"] == 10 and sd["row0"] == 0
    assert sd["num_params"] == sd["num_params_global"] == sum(SIZES) and sd["param_sizes"] == list(SIZES)
    assert sd["U"].dtype == opt._store_dtype and sd["U"].device.type == "cpu" and sd["branch_rng"].dtype == torch.uint8
    assert sd["state_dtype"] == str(opt._store_dtype) and sd["state_route"] == ("native" if kind == "native" else "widen")
    assert ("round_seed0" in sd) == ("round_step" in sd) == (kind == "native")
    if kind == "native":
        assert 0 <= sd["round_step"] <= 3 and 0 <= sd["round_seed0"] < 2 ** 62
        assert opt._round_seed0 == sd["round_seed0"] and sd["round_step"] <= opt._round_step <= sd["round_step"] + 3
    if tail == "fused":
        assert opt._tail is not None


def test_pickling_the_tensors_alone_does_not_resume(psgd, monkeypatch):
    """what the issue starts from: U, V, d copied by hand into a new native optimizer give another rounding stream and other coins"""
    coins = _Coins(monkeypatch, psgd)
    (want, _), sd, params3, _ = _reference_and_half(psgd, coins, "native", step_tail="torch")
    _, c = _fresh_params()
    params = [p.clone().requires_grad_(True) for p in params3]
    opt = _make(psgd, "native", params, seed=99)
    for mine, k in ((opt._U, "U"), (opt._V, "V"), (opt._d, "d")):
        mine.copy_(sd[k])
    _steps(opt, _closure(params, c), range(3, 6))
    assert not all(_same_bits(a, b) for a, b in zip(_snapshot(opt, params), want))


def test_placed_state_stays_in_its_arena(psgd, monkeypatch):
    coins = _Coins(monkeypatch, psgd)
    _, sd, params3, _ = _reference_and_half(psgd, coins, "fp32", step_tail="torch")
    plain, pp, pc = _resume(psgd, "fp32", sd, params3)
    placed, qp, qc = _resume(psgd, "fp32", sd, params3, placement="packed")
    assert placed._arena is not None and plain._arena is None
    placed2, _, _ = _resume(psgd, "fp32", sd, params3, placement="packed")       # the pointers before and after a load
    ptrs = [t.data_ptr() for t in (placed2._U, placed2._V, placed2._d)]
    placed2.load_state_dict(sd)
    assert [t.data_ptr() for t in (placed2._U, placed2._V, placed2._d)] == ptrs
    for opt in (placed, placed2):
        assert opt._U is opt._arena.U and opt._V is opt._arena.V and opt._d is opt._arena.d
    assert _same_bits(placed._U, sd["U"].to(_dev())) and _same_bits(placed._d, sd["d"].to(_dev()))
    _steps(plain, pc, [3])
    _steps(placed, qc, [3])
    for a, b in zip(_snapshot(placed, qp), _snapshot(plain, pp)):
        assert _same_bits(a, b)
    assert placed._U is placed._arena.U


# ------------------------------------------------------------------------------------------------ 6. fp32 -> native bf16
N6, R6 = 65539, 20
_ckpt6 = {}


def _fp32_checkpoint(psgd):
    if not _ckpt6:
        params, c = _fresh_params((N6,))
        opt = _make(psgd, "fp32", params, r=R6, preconditioner_update_probability=1.0)
        _steps(opt, _closure(params, c), range(2))
        _ckpt6["sd"] = _through_torch_save(opt.state_dict())
    return _ckpt6["sd"]


def _native6(psgd, seed=31):
    params, _ = _fresh_params((N6,))
    return _make(psgd, "native", params, seed=seed, r=R6)


def test_fp32_checkpoint_into_native_nearest(psgd, monkeypatch):
    sd = _fp32_checkpoint(psgd)
    assert sd["U"].dtype == torch.float32 and "round_seed0" not in sd
    monkeypatch.setattr(psgd, "_NARROW_STAGING_BYTES", 64 * 1024)          # 4 N r / 64 KiB = 80 chunks per factor, 5 for d
    opt = _native6(psgd)
    seed0, step0 = opt._round_seed0, opt._round_step
    opt.load_state_dict(sd, narrow_rounding="nearest")
    for k, mine in (("U", opt._U), ("V", opt._V), ("d", opt._d)):
        assert mine.dtype == torch.bfloat16 and np.array_equal(_codes(mine), _codes(sd[k].to(torch.bfloat16))), k
    assert (opt._round_seed0, opt._round_step) == (seed0, step0)              # absent in the checkpoint: the object keeps its own
    assert float(opt.lr_params) == 0.05 and float(opt.preconditioner_update_probability) == 1.0


def test_fp32_checkpoint_into_native_stochastic(psgd, hip_lib, monkeypatch):
    sd = _fp32_checkpoint(psgd)
    got = {}
    for staging in (64 * 1024, 1024 * 1024):
        monkeypatch.setattr(psgd, "_NARROW_STAGING_BYTES", staging)
        opt = _native6(psgd)
        assert opt._state_rounding == "stochastic"
        opt.load_state_dict(sd)                                               # the optimizer's own rounding, the default seed
        got[staging] = {k: _codes(t) for k, t in (("U", opt._U), ("V", opt._V), ("d", opt._d))}
    for k in ("U", "V", "d"):
        _floor_or_ceil(sd[k], got[64 * 1024][k])
        assert np.array_equal(got[64 * 1024][k], got[1024 * 1024][k]), k
    rne = _codes(sd["U"].to(torch.bfloat16))
    assert 0.1 < float(np.mean(got[64 * 1024]["U"] != rne)) < 0.5            # stochastic indeed: P = E min(f, 1 - f) = 1/4
    # the default seed is uvd_step_rounding_seed(round_seed0, 2^40 + round_step) and the index is the global element index
    seed = psgd.uvd_step_rounding_seed(opt._round_seed0, 2 ** 40 + opt._round_step)
    assert seed not in {psgd.uvd_step_rounding_seed(opt._round_seed0, k) for k in range(64)}
    for tensor, k in enumerate(("U", "V", "d")):
        one = torch.empty(sd[k].numel(), dtype=torch.bfloat16, device=_dev())
        _narrow(hip_lib, sd[k].reshape(-1).to(_dev()), one, index0=0, tensor=tensor, rounding=1, seed=seed)
        assert np.array_equal(_codes(one), got[64 * 1024][k].reshape(-1)), k
    other = _native6(psgd)
    other.load_state_dict(sd, narrow_seed=7)
    assert not np.array_equal(_codes(other._U), got[64 * 1024]["U"])


def test_fp32_checkpoint_into_native_memory(psgd):
    """in the manner of test_step_memory (N = 4M, r = 20): the load's peak over the allocated baseline is the 64-MiB staging
    buffer (+ 16 MiB of slack), not an fp32 image of a factor (4 N r = 320 MB)"""
    N, r = 4 * 1024 * 1024, 20
    assert psgd._NARROW_STAGING_BYTES == 64 << 20
    w = torch.zeros(N, device=_dev(), requires_grad=True)
    opt = psgd.UVd([w], rank_of_modification=r, generator=torch.Generator().manual_seed(1), state_dtype=torch.bfloat16,
                   state_route="native", placement=None)
    sd = opt.state_dict()
    del sd["round_seed0"], sd["round_step"]
    g = torch.Generator().manual_seed(8)
    sd["U"] = torch.randn(N, r, generator=g)
    sd["V"] = sd["U"]
    sd["d"] = torch.rand(N, 1, generator=g) + 0.5
    sd["state_dtype"], sd["state_route"], sd["state_rounding"] = "torch.float32", "widen", "none"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    opt.load_state_dict(sd, narrow_rounding="nearest")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("load memory: %.1f MB over the state (one fp32 factor: %.1f MB)" % (peak / 1e6, 4 * N * r / 1e6))
    assert peak <= (64 << 20) + (16 << 20), peak
    assert torch.equal(opt._U.cpu().view(torch.int16), sd["U"].to(torch.bfloat16).view(torch.int16))
    assert torch.equal(opt._V.view(torch.int16), opt._U.view(torch.int16))
    assert torch.equal(opt._d.cpu().view(torch.int16), sd["d"].to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------------------------------------------------ 7. sharded, one rank
@pytest.fixture(scope="module")
def pg():
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29557", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    yield dist.group.WORLD
    dist.destroy_process_group()


def test_sharded_one_rank_round_trip(psgd, monkeypatch, pg):
    opt, sd = _check_round_trip(psgd, monkeypatch, "native", group=pg)
    assert opt._group is pg and sd["row0"] == 0 and sd["num_params_global"] == sd["num_params"] == sum(SIZES)
    assert "round_seed0" in sd and sd["state_route"] == "native"
    assert torch.equal(sd["branch_rng"], _through_torch_save(sd)["branch_rng"])


# ------------------------------------------------------------------------------------------------ 8. reshard on the device
def test_resharded_rows_on_the_device(psgd, hip_lib):
    """The class drives a row shard only under a real process group, so two shards cannot step in one process: the loaded rows
    of each are checked instead, bit for bit, and -- for an fp32 checkpoint narrowed on load -- that the two shards store the
    codes the unsharded load stores (the stream is keyed by the global element index, from the dict's row0)."""
    from psgd_tf_amd import sharded
    cuts, r = (0, 1024, 1024 + 777), 8
    params, c = _fresh_params((cuts[-1],))
    opt = _make(psgd, "native", params, r=r, preconditioner_update_probability=1.0)
    _steps(opt, _closure(params, c), range(2))
    sd = opt.state_dict()
    parts = sharded.reshard_uvd_state([sd], [1024, 777])
    shards = []
    for part, (lo, hi) in zip(parts, zip(cuts, cuts[1:])):
        w = torch.zeros(hi - lo, device=_dev(), requires_grad=True)
        sh = _make_other(psgd, "native", [w], r=r)
        with pytest.raises(ValueError, match="num_params_global"):
            sh.load_state_dict(part)                                          # strict: this object is not that shard of 1801 rows
        sh.load_state_dict(part, strict=False)
        for k, mine in (("U", sh._U), ("V", sh._V), ("d", sh._d)):
            assert np.array_equal(_codes(mine), _codes(sd[k][lo:hi])), (k, lo)
        assert (sh._round_seed0, sh._round_step) == (sd["round_seed0"], sd["round_step"]) and float(sh.lr_params) == 0.05
        shards.append(sh)
    # an fp32 checkpoint of the same rows: whole, and resharded
    f32 = {k: (v.float() * 1.0009765625 if k in ("U", "V", "d") else v) for k, v in sd.items() if not k.startswith("round_")}
    f32["state_dtype"], f32["state_route"], f32["state_rounding"] = "torch.float32", "widen", "none"
    opt.load_state_dict(f32, narrow_seed=11)
    whole = {k: _codes(t) for k, t in (("U", opt._U), ("V", opt._V), ("d", opt._d))}
    _floor_or_ceil(f32["U"], whole["U"])
    for part, sh, (lo, hi) in zip(sharded.reshard_uvd_state([f32], [1024, 777]), shards, zip(cuts, cuts[1:])):
        sh.load_state_dict(part, strict=False, narrow_seed=11)
        for k, mine in (("U", sh._U), ("V", sh._V), ("d", sh._d)):
            assert np.array_equal(_codes(mine), whole[k][lo:hi]), (k, lo)


# ------------------------------------------------------------------------------------------------ 9. errors
def test_load_errors(psgd):
    params, _ = _fresh_params()
    opt = _make(psgd, "native", params)
    good = opt.state_dict()
    before = _snapshot(opt, params)

    def broken(**kw):
        sd = dict(good)
        sd.update(kw)
        return sd
    with pytest.raises(ValueError, match="'rank'"):
        opt.load_state_dict(broken(rank=11))
    with pytest.raises(ValueError, match="'param_sizes'"):
        opt.load_state_dict(broken(param_sizes=[1021, 777]))
    with pytest.raises(ValueError, match="'format'"):
        opt.load_state_dict(broken(format=2))
    with pytest.raises(ValueError, match="'num_params'"):
        opt.load_state_dict(broken(num_params=5))
    with pytest.raises(ValueError, match="'row0'"):
        opt.load_state_dict(broken(row0=64))
    with pytest.raises(ValueError, match="'num_params_global'"):
        opt.load_state_dict(broken(num_params_global=10 ** 6))
    with pytest.raises(ValueError, match="'hyper'"):
        opt.load_state_dict({k: v for k, v in good.items() if k != "hyper"})
    with pytest.raises(TypeError, match="float16"):
        opt.load_state_dict(broken(U=good["U"].to(torch.float16), V=good["V"].to(torch.float16), d=good["d"].to(torch.float16)))
    with pytest.raises(ValueError, match="narrow_rounding"):
        opt.load_state_dict(good, narrow_rounding="up")
    for a, b in zip(_snapshot(opt, params), before):                          # a refused load changes nothing
        assert _same_bits(a, b)
    opt.load_state_dict(broken(param_sizes=None))                             # None (a resharded dict): the check is skipped
    widen = _make(psgd, "widen", _fresh_params()[0])
    with pytest.raises(TypeError, match="float32"):                           # fp32 narrows into the NATIVE route only
        widen.load_state_dict(broken(U=good["U"].float(), V=good["V"].float(), d=good["d"].float()))
    fp32 = _make(psgd, "fp32", _fresh_params()[0])
    fp32.load_state_dict(good)                                                # bf16 -> fp32: exact widening
    assert torch.equal(fp32._U.cpu(), good["U"].float()) and torch.equal(fp32._d.cpu(), good["d"].float())
    with pytest.raises(ValueError, match="tensor"):
        psgd.uvd_bf16_narrow_(opt._U, opt._U.float(), tensor="Q")
    with pytest.raises(TypeError):
        psgd.uvd_bf16_narrow_(opt._U.float(), opt._U.float(), tensor="U")


# ------------------------------------------------------------------------------------------------ 10. judge, then commit
TINY = [(5, 7), (4, 3), (7,)]
ROUTES = {"packed": dict(placement="packed"), "native": dict(state_dtype=torch.bfloat16, state_route="native", placement=None)}


def _tiny(psgd, route, seed):
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(s, generator=g).to(_dev()).requires_grad_(True) for s in TINY]
    c = [torch.rand(s, generator=g).add(0.5).to(_dev()) for s in TINY]
    torch.cuda.manual_seed(seed)
    opt = psgd.UVd(params, 3, lr_params=0.05 * seed, lr_preconditioner=0.1, generator=torch.Generator().manual_seed(seed),
                   momentum=0.9, preconditioner_fit="whitening", step_tail="fused", **ROUTES[route])
    return opt, params, lambda: sum(0.5 * (ci * p * p).sum() for p, ci in zip(params, c))


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_refused_load_changes_nothing_on_the_device_routes(psgd, route):
    """the two routes of the state that cannot be built without a device: a refused dict leaves the tensors, the momentum buffer
    and the rounding stream as they were, the accepted one gives the twin's next step bit for bit"""
    twin, tparams, tclosure = _tiny(psgd, route, 9)
    for _ in range(2):
        twin.step(tclosure)
    sd = _through_torch_save(twin.state_dict())
    opt, params, closure = _tiny(psgd, route, 3)
    opt.step(closure)

    def held():
        return [t.detach().clone() for t in (opt._U, opt._V, opt._d, opt._momentum_buffer())], (opt._round_seed0, opt._round_step)
    tensors = (opt._U, opt._V, opt._d)
    before = held()
    with pytest.raises(ValueError, match="probe_step"):
        opt.load_state_dict({k: v for k, v in sd.items() if k != "probe_step"})
    after = held()
    assert all(_same_bits(a, b) for a, b in zip(after[0], before[0])) and after[1] == before[1]
    assert all(a is b for a, b in zip(tensors, (opt._U, opt._V, opt._d))) and float(opt.lr_params) == 0.05 * 3
    if route == "packed":
        assert opt._U is opt._arena.U and opt._V is opt._arena.V and opt._d is opt._arena.d and opt._m is None
    else:
        assert opt._arena is None and opt._round_seed0 is not None and before[1][1] == 1
    assert not _same_bits(opt._U, twin._U) and opt.probe_step == 1 and twin.probe_step == 2
    opt.load_state_dict(sd)
    assert all(a is b for a, b in zip(tensors, (opt._U, opt._V, opt._d))) and (opt._round_seed0, opt._round_step) == \
        (twin._round_seed0, twin._round_step)
    with torch.no_grad():
        for p, q in zip(params, tparams):
            p.copy_(q)
    twin.step(tclosure)
    opt.step(closure)
    got = [opt._U, opt._V, opt._d, opt._momentum_buffer()] + params
    want = [twin._U, twin._V, twin._d, twin._momentum_buffer()] + tparams
    assert all(_same_bits(a, b) for a, b in zip(got, want)) and opt.probe_step == twin.probe_step == 3
