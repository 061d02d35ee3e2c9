"""The staged bf16-state UVd kernels (row-sharded optimizer) in ONE process, no process group (GPU).

Two "ranks" run their stages one after the other on one device, each with its own workspace; an exchange is emulated by
concatenating the ranks' send regions (psgd_uvd_bf16_ws_region) and calling psgd_uvd_bf16_fold_gathered_f64 on every rank.
  (a) one rank, row0 = 0, fold of one copy: bit-identical to the one-call functions (state codes and out, both roundings);
  (b) two shards against the fp64 oracle on the GLOBAL problem, with the bars of tests/test_uvd_bf16_gpu.py: every stored
      element |stored - y64| <= 2^-7 |y64| + 1e-5 rms(y64); the share of codes that are not RNE(y64) (stochastic: neither floor
      nor ceil) <= 2 x that of the fp32 kernels + 1e-4; out within 1e-5 of the oracle apply on the stored state;
  (c) the rounding stream is global: with one seed, the codes of shard 1's rows differ from the one-call run's in a share
      <= 0.05 (a stream keyed by the LOCAL row would re-draw them: about a third would differ, P = 2 f (1 - f) over a uniform
      fractional part f); what remains is fp64 fold order moving a value across a rounding boundary;
  (d) row0 moves the stream: the same shard with row0 = 0 and row0 = 448 stores different codes, both floor-or-ceil;
  (e) the first call on a workspace and an output filled with 0xFF gives what a second call gives.
Set PSGD_UVD_BF16_SHARDED_PARITY_OUT to a file name to collect the measured shares of (c).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from tests.uvd_cases import TINY32, check_bf16_state, make_uvd_problem, rel_err, to_bf16_np

pytestmark = pytest.mark.gpu

STEP = 0.01
SHAPES = ((777, 448), (65539, 32832))           # (N, first row of shard 1): shard_rows(N, 1, 2)[0]; both shards end in partial tiles
RANKS = (1, 7, 20, 32)
CALLS = ("apply", "update", "fused")
SEND = 2                                        # PSGD_WS_SEND_F64


@pytest.fixture(scope="module")
def psgd(hip_lib):
    import psgd_tf_amd.preconditioned_stochastic_gradient_descent as m
    return m


def _dev():
    return torch.device("cuda:0")


_problems, _refs = {}, {}


def problem(N, r):
    if (N, r) not in _problems:
        p = make_uvd_problem(N, r, seed=N % 97 + r, d_spread=0.3)
        for k in ("U", "V", "d"):
            p[k] = to_bf16_np(p[k])
        _problems[(N, r)] = p
    return _problems[(N, r)]


def reference(psgd, key, p, update_U, balance):
    """(fp64 oracle state after the update, the fp32 kernels' state on the widened inputs): computed once per case, never changed"""
    k = (key, update_U, balance)
    if k not in _refs:
        q = {n: v.astype(np.float64) for n, v in p.items()}
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=bool(balance), update_U=bool(update_U))
        w = {n: torch.from_numpy(v).to(_dev()) for n, v in p.items()}
        psgd.update_precond_UVd_math_(w["U"], w["V"], w["d"], w["v"], w["h"], STEP, TINY32, balance=bool(balance), update_U=bool(update_U))
        _refs[k] = ({n: q[n] for n in ("U", "V", "d")}, {n: w[n].cpu().numpy() for n in ("U", "V", "d")})
    return _refs[k]


def shard(p, lo, hi):
    t = {}
    for k, a in p.items():
        x = torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(_dev())
        t[k] = x.to(torch.bfloat16) if k in ("U", "V", "d") else x
    return t


class Rank:
    """one rank of the emulation: its rows, its own workspace and output"""

    def __init__(self, lib, t, r, row0, poison=False, ws=None):
        self.lib, self.t, self.N, self.r, self.row0 = lib, t, t["U"].shape[0], r, row0
        need = lib.psgd_uvd_bf16_workspace_bytes(self.N, r)
        self.ws = torch.empty(need, dtype=torch.uint8, device=_dev()) if ws is None else ws
        self.out = torch.empty_like(t["g"])
        if poison:
            self.ws.fill_(0xFF)
            self.out.view(torch.uint8).fill_(0xFF)
        self.tail = (self.ws.data_ptr(), self.ws.numel(), torch.cuda.current_stream().cuda_stream)

    def send(self, stage):
        off, cnt = ctypes.c_int64(0), ctypes.c_int64(0)
        assert self.lib.psgd_uvd_bf16_ws_region(SEND, stage, self.N, self.r, ctypes.byref(off), ctypes.byref(cnt)) == 0
        return self.ws[off.value:off.value + 8 * cnt.value].view(torch.float64)

    def p(self, *names):
        return [self.t[n].data_ptr() for n in names]


def exchange(ranks, stage):
    gathered = torch.cat([k.send(stage) for k in ranks]).contiguous()
    for k in ranks:
        assert k.lib.psgd_uvd_bf16_fold_gathered_f64(stage, gathered.data_ptr(), len(ranks), k.N, k.r, *k.tail) == 0


def staged(ranks, call, update_U, balance, mode, seed):
    """the sequences of include/psgd_hip.h on every rank, with the exchanges between them"""
    def each(fn):
        for k in ranks:
            assert fn(k) == 0
    L = ranks[0].lib
    if call != "apply":
        if balance:
            each(lambda k: L.psgd_uvd_balance_max_bf16(*k.p("U", "V"), k.N, k.r, *k.tail))
            exchange(ranks, 10)
        each(lambda k: L.psgd_uvd_update_gram_bf16(*k.p("U", "V", "d", "v", "h"), k.N, k.r, *k.tail))
        exchange(ranks, 11)
        each(lambda k: L.psgd_uvd_update_rewrite_bf16(*k.p("U", "V", "d", "v", "h"), k.N, k.r, STEP, TINY32, balance, update_U, mode, seed,
                                                      k.row0, *k.tail))
        exchange(ranks, 12)
    if call == "update":
        each(lambda k: L.psgd_uvd_update_d_bf16(*k.p("d"), k.N, k.r, STEP, TINY32, mode, seed, k.row0, *k.tail))
        return
    if call == "apply":
        each(lambda k: L.psgd_uvd_apply_sweep1_bf16(*k.p("V", "d", "g"), k.N, k.r, *k.tail))
    else:
        each(lambda k: L.psgd_uvd_apply_sweep1_d_bf16(*k.p("V", "d", "g"), k.N, k.r, STEP, TINY32, mode, seed, k.row0, *k.tail))
    exchange(ranks, 1)
    each(lambda k: L.psgd_uvd_apply_sweep2_bf16(*k.p("U", "d", "g"), k.out.data_ptr(), k.N, k.r, *k.tail))
    exchange(ranks, 2)
    each(lambda k: L.psgd_uvd_apply_sweep3_bf16(*k.p("V", "d"), k.out.data_ptr(), k.N, k.r, *k.tail))


def one_call(psgd, t, call, update_U, balance, rounding, seed):
    kw = dict(balance=bool(balance), update_U=bool(update_U), rounding=rounding, rounding_seed=seed)
    if call == "apply":
        return psgd.precond_grad_UVd_math(t["U"], t["V"], t["d"], t["g"])
    if call == "update":
        return psgd.update_precond_UVd_math_(t["U"], t["V"], t["d"], t["v"], t["h"], STEP, TINY32, **kw)
    return psgd.update_precond_UVd_math_and_precond_grad(t["U"], t["V"], t["d"], t["v"], t["h"], t["g"], STEP, TINY32, **kw)


def codes(t):
    return {k: t[k].view(torch.int16).cpu().numpy().copy() for k in ("U", "V", "d")}


def widened64(x):
    return x.float().cpu().numpy().astype(np.float64)


def _record(line):
    path = os.environ.get("PSGD_UVD_BF16_SHARDED_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _branches(call):
    return ((0, 0),) if call == "apply" else ((1, 0), (0, 0), (1, 1), (0, 1))


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("N,cut", SHAPES)
def test_one_rank_is_bit_identical_to_the_one_call_functions(psgd, hip_lib, N, cut, r):
    p = problem(N, r)
    for call in CALLS:
        for update_U, balance in _branches(call):
            for rounding in (("nearest",) if call == "apply" else ("nearest", "stochastic")):
                a, b = shard(p, 0, N), shard(p, 0, N)
                want = one_call(psgd, a, call, update_U, balance, rounding, 4242 + r)
                k = Rank(hip_lib, b, r, 0)
                staged([k], call, update_U, balance, int(rounding == "stochastic"), 4242 + r)
                tag = (call, update_U, balance, rounding)
                ca, cb = codes(a), codes(b)
                for n in ("U", "V", "d"):
                    assert np.array_equal(ca[n], cb[n]), (tag, n)
                if call != "update":
                    assert torch.equal(want, k.out), tag


# ------------------------------------------------------------------------------------------------ (b), (c)
@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("N,cut", SHAPES)
def test_two_shards_against_the_oracle_and_the_global_rounding_stream(psgd, hip_lib, N, cut, r):
    p = problem(N, r)
    for call in CALLS:
        for update_U, balance in _branches(call):
            for rounding in (("nearest",) if call == "apply" else ("nearest", "stochastic")):
                seed = 99 + r
                ranks = [Rank(hip_lib, shard(p, 0, cut), r, 0), Rank(hip_lib, shard(p, cut, N), r, cut)]
                staged(ranks, call, update_U, balance, int(rounding == "stochastic"), seed)
                tag = "%s N=%d r=%d update_U=%d balance=%d %s" % (call, N, r, update_U, balance, rounding)
                stored = {n: np.concatenate([widened64(k.t[n]) for k in ranks], 0) for n in ("U", "V", "d")}
                g64 = p["g"].astype(np.float64)
                if call == "apply":
                    for n in ("U", "V", "d"):
                        assert np.array_equal(stored[n], p[n].astype(np.float64)), (tag, n)      # the apply writes no state
                else:
                    y64, widen32 = reference(psgd, (N, r), p, update_U, balance)
                    written = {"d", "U" if update_U else "V"} | ({"U", "V"} if balance else set())
                    for n in ("U", "V"):
                        if n not in written:
                            assert np.array_equal(stored[n], p[n].astype(np.float64)), (tag, n)
                    pn, pw, _ = check_bf16_state(tag, stored, y64, widen32, written, rounding)
                    print("%s p_native=%.3e p_widen=%.3e" % (tag, pn, pw))
                    assert pn <= 2 * pw + 1e-4, (tag, pn, pw)
                    # (c) against the one-call run with the same seed: the codes of shard 1's rows
                    whole = shard(p, 0, N)
                    one_call(psgd, whole, call, update_U, balance, rounding, seed)
                    cw, cs = codes(whole), codes(ranks[1].t)
                    differ = sum(int(np.sum(cw[n][cut:] != cs[n])) for n in written)
                    share = differ / sum(cs[n].size for n in written)
                    line = "%s share of shard-1 codes that differ from the one-call run: %.3e" % (tag, share)
                    print(line)
                    _record(line)
                    assert share <= 0.05, line
                if call != "update":
                    out = np.concatenate([k.out.cpu().numpy() for k in ranks], 0)
                    e = rel_err(out, orc.precond_grad_UVd_math(stored["U"], stored["V"], stored["d"], g64))
                    print(tag + " gradient rel err %.2e" % e)
                    assert e < 1e-5, (tag, e)


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("call", ("update", "fused"))
@pytest.mark.parametrize("r", (7, 32))
def test_row0_moves_the_rounding_stream(psgd, hip_lib, r, call):
    N, cut = SHAPES[0]
    g = problem(N, r)
    p = {k: v[cut:] for k, v in g.items()}                    # shard 1's rows as a problem of their own
    runs = []
    for row0 in (0, cut):
        k = Rank(hip_lib, shard(p, 0, N - cut), r, row0)
        staged([k], call, 1, 1, 1, 31337)                     # balance: every state tensor is written
        runs.append(k)
    ca, cb = codes(runs[0].t), codes(runs[1].t)
    y64, widen32 = reference(psgd, ("shard1", N, r), p, 1, 1)
    for n in ("U", "V", "d"):
        assert not np.array_equal(ca[n], cb[n]), n
    for k in runs:
        stored = {n: widened64(k.t[n]) for n in ("U", "V", "d")}
        pn, pw, _ = check_bf16_state("row0=%d" % k.row0, stored, y64, widen32, {"U", "V", "d"}, "stochastic")
        assert pn <= 2 * pw + 1e-4, (k.row0, pn, pw)          # floor or ceil of the oracle's value


# ------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("N,cut,r", ((777, 448, 7), (65539, 32832, 32)))
def test_first_call_on_poisoned_workspace_and_output(hip_lib, N, cut, r):
    p = problem(N, r)
    for call, update_U, balance in (("apply", 0, 0), ("update", 1, 1), ("fused", 0, 0), ("fused", 1, 1)):
        first = [Rank(hip_lib, shard(p, 0, cut), r, 0, poison=True), Rank(hip_lib, shard(p, cut, N), r, cut, poison=True)]
        staged(first, call, update_U, balance, 1, 5)
        again = [Rank(hip_lib, shard(p, 0, cut), r, 0, ws=first[0].ws), Rank(hip_lib, shard(p, cut, N), r, cut, ws=first[1].ws)]
        staged(again, call, update_U, balance, 1, 5)
        torch.cuda.synchronize()
        for a, b in zip(first, again):
            ca, cb = codes(a.t), codes(b.t)
            for n in ("U", "V", "d"):
                assert np.array_equal(ca[n], cb[n]), (call, n)
                assert torch.isfinite(a.t[n].float()).all(), (call, n)
            if call != "update":
                assert torch.equal(a.out, b.out) and torch.isfinite(a.out).all(), call
