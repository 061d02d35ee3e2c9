"""Guard bands around every operand of the C ABI: no entry point touches memory outside its extents (GPU).

Every case carves its operands out of one pattern-filled arena (tests/guard_bands.py) and calls the C ABI through ctypes with the
pointers and workspace sizes it chose: matrices at their documented alignment and NO BETTER (16 bytes, not 32), fp32 vectors at
skews of 1, 2 and 3 floats (g 1, v 2, h 3, out 3 -- with three skews the fourth vector of the fused calls shares h's), operands the
header allows anywhere (the dense Q, the sparse-LU U12) at an odd float, workspaces of exactly the bytes the size function returns.
Each case runs on an arena of 0xFF bytes (NaN in fp32 / bf16 / f16, huge as a counter) and on one of 0x3F bytes (0.747...), with
the same inputs, and asserts

  1. PSGD_OK;   2. the guards and every read-only operand intact on both arenas;   3. finite outputs;
  4. outputs bit-identical between the two fills (nothing read outside the extents or from unwritten workspace reaches a result);
  5. parity with the fp64 oracle at the bar of the entry point's own test (imported, or restated with its source).

ENTRY_POINTS is the case table: every name in it is called by a case below (`_Ctx.call` refuses others).  COVERED_ELSEWHERE
names the list kernels (psgd_multi_*, psgd_uvd_pack*, psgd_uvd_param_update_multi*: the families with guard bands of their own, in
the files named there) and nothing else.  tests/test_cabi_cpu.py asserts that every exported compute entry point is in one of the two.

Bit-equality (4) relies on run-to-run reproducibility, so every case first runs twice on ordinary tensors and must give the same
bits there; no entry point is exempted from (4).

Notes on the cases:
  - stage forms run as the multi-GPU sequence of a one-rank group: stage, all-gather of one copy of the send region, fold, next
    stage -- which is what covers the psgd_*_fold_gathered_f64 entry points;
  - sparse LU on a bf16 state takes ranks up to 32: of the sparse-LU shapes it runs (12, 12) and (1021, 7);
  - Kron bf16 operands: the entry points take multiples of 8 only (the Python side pads (1, 3), (7, 5) ... to them), so the
    smallest aligned shape is (8, 8) and the smallest that is not a tile multiple is (200, 72);
  - `_ld` views of rank 32 need ld % 4 == 0: in the ld = 65 parent they are refused with PSGD_ERR_ALIGN (asserted, nothing
    written), the width-1 views run in both parents;
  - the fold entry points read their `gathered` operand from the arena as well (frozen, guarded);
  - large Kron routes: for each distinct psgd_kron_dd_route_flags value among the shapes of tests/test_kron_routes_gpu.py the
    smallest shape runs when no side exceeds 1100: (513, 100), (513, 384), (599, 300), (600, 300), (1000, 1024).  Skipped, a side
    above 1100 (flag value: smallest shape) -- 846: (4096, 4097); 862: (2817, 4226); 894: (4096, 4096); 9182: (1024, 2048);
    17358: (2049, 8192); 17374: (768, 3072); 24966: (511, 2560); 25566: (512, 2560); 33158: (128, 4096); 33758: (256, 4096).
    test_large_route_lists_are_the_ones_named pins both lists to psgd_kron_dd_route_flags.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import psgd_oracle as orc
from psgd_tf_amd import _lib
from tests.guard_bands import Arena
from tests.splu_cases import make_splu_problem
from tests.uvd_cases import TINY32, make_uvd_problem, rel_err, to_bf16_np

pytestmark = pytest.mark.gpu

FILLS = (0xFF, 0x3F)
STEP = 0.01
SEND = _lib.PSGD_WS_SEND_F64

# the bars, each from the test of the entry point
UVD_APPLY_TOL, UVD_STATE_TOL, UVD_INCR_TOL = 1e-5, 1e-5, 2e-3      # tests/test_uvd_gpu.py APPLY_TOL, STATE_TOL, INCR_TOL
BLOCK_TOL = 1e-6          # tests/test_uvd_gpu.py test_strided_building_blocks_of_the_wide_rank_path (colsums, axpy, rank2)
WIDE_GRAM_TOL = 5e-7      # tests/test_uvd_gpu.py test_wide_gram_matches_fp64, relative to sqrt(G_ii G_jj)
BF16_STATE_APPLY_TOL = 1e-5   # tests/test_uvd_bf16_gpu.py test_apply, tests/test_splu_bf16_gpu.py (apply on the stored codes)
SPLU_APPLY_TOL, SPLU_STATE_TOL, SPLU_INCR_TOL = 1e-5, 1e-5, 2e-3   # tests/test_splu_gpu.py
DENSE_TOL, DENSE_INCR_TOL = 1e-5, 2e-3                             # tests/test_dense_gpu.py test_update_and_apply_match_fp64
KRON_TOL, KRON_INCR_TOL = 1e-5, 2e-3                               # tests/test_kron_gpu.py TOL, INCR_TOL
KRON_BF16_TOL, KRON_BF16_UPD_TOL, KRON_BF16_UPD_STATE_TOL = 2e-2, 2e-2, 2e-4   # tests/test_kron_gpu.py BF16_TOL, BF16_UPD_TOL, ..._STATE_TOL

ENTRY_POINTS = {
    "uvd": ["psgd_uvd_apply_f32", "psgd_uvd_apply_sweep1_f32", "psgd_uvd_apply_sweep2_f32", "psgd_uvd_apply_sweep3_f32",
            "psgd_uvd_update_f32", "psgd_uvd_balance_max_f32", "psgd_uvd_balance_scale_f32", "psgd_uvd_update_sweep1_f32",
            "psgd_uvd_update_sweep2_f32", "psgd_uvd_update_sweep3_f32", "psgd_uvd_update_apply_f32",
            "psgd_uvd_update_sweep2_fused_f32", "psgd_uvd_fused_post_f32", "psgd_uvd_fused_final_f32", "psgd_uvd_ipuvt_matvec_f32",
            "psgd_uvd_ipuvt_matvec_cols_f32", "psgd_uvd_apply_cols_f32", "psgd_uvd_fold_gathered_f64", "psgd_uvd_colsums_f32",
            "psgd_uvd_axpy_cols_f32", "psgd_uvd_rank2_update_f32"],
    "wide": ["psgd_uvd_gram_wide_f32", "psgd_uvd_wide_apply_cols_f32", "psgd_uvd_wide_update_f32", "psgd_uvd_wide_update_apply_f32",
             "psgd_uvd_wide_colsums_f32", "psgd_uvd_wide_axpy_cols_f32", "psgd_uvd_wide_rank2_update_f32"],
    "ld": ["psgd_uvd_colsums_ld_f32", "psgd_uvd_axpy_cols_ld_f32", "psgd_uvd_rank2_update_ld_f32", "psgd_uvd_update_sweep1_ld_f32"],
    "uvd_bf16": ["psgd_uvd_apply_bf16", "psgd_uvd_update_bf16", "psgd_uvd_update_apply_bf16", "psgd_uvd_bf16_narrow_f32",
                 "psgd_uvd_bf16_fold_gathered_f64", "psgd_uvd_balance_max_bf16", "psgd_uvd_update_gram_bf16",
                 "psgd_uvd_update_rewrite_bf16", "psgd_uvd_update_d_bf16", "psgd_uvd_apply_sweep1_bf16",
                 "psgd_uvd_apply_sweep1_d_bf16", "psgd_uvd_apply_sweep2_bf16", "psgd_uvd_apply_sweep3_bf16"],
    "splu": ["psgd_splu_apply_f32", "psgd_splu_update_f32", "psgd_splu_fold_gathered_f64", "psgd_splu_stage1_f32",
             "psgd_splu_apply_stage2_f32", "psgd_splu_apply_stage3_f32", "psgd_splu_update_stage2_f32",
             "psgd_splu_update_stage3_f32", "psgd_splu_update_stage4_f32", "psgd_splu_apply_bf16", "psgd_splu_update_bf16"],
    "dense": ["psgd_dense_update_f32", "psgd_dense_apply_f32"],
    "tail": ["psgd_uvd_sumsq_f32", "psgd_uvd_check_multi"],
    "kron": ["psgd_kron_dd_apply_f32", "psgd_kron_dd_apply_direct_f32", "psgd_kron_dd_prepare_f32",
             "psgd_kron_dd_apply_prepared_f32", "psgd_kron_dd_update_f32", "psgd_kron_dd_apply_batched_f32",
             "psgd_kron_dd_prepare_batched_f32", "psgd_kron_dd_apply_prepared_batched_f32", "psgd_kron_dd_update_batched_f32"],
    "kron_bf16": ["psgd_kron_dd_apply_bf16", "psgd_kron_bf16_prepare_factors", "psgd_kron_dd_apply_bf16_prepared",
                  "psgd_kron_dd_update_bf16", "psgd_kron_bf16_handoff_reset"],
    "kron_sparse": ["psgd_kron_ds_update_f32", "psgd_kron_ds_apply_f32", "psgd_kron_nd_update_f32", "psgd_kron_nd_apply_f32",
                    "psgd_kron_ns_update_f32", "psgd_kron_ns_apply_f32"],
}
# the list kernels (out of scope here, and only they): a GPU test file that runs each of them by name
COVERED_ELSEWHERE_PATTERNS = ("psgd_multi_", "psgd_uvd_pack", "psgd_uvd_param_update_multi")
COVERED_ELSEWHERE = {
    "psgd_uvd_pack_f32": "tests/test_uvd_momentum_gpu.py", "psgd_uvd_pack_blend_f32": "tests/test_uvd_momentum_gpu.py",
    "psgd_uvd_pack_check_f32": "tests/test_uvd_guard_gpu.py", "psgd_uvd_param_update_multi": "tests/test_uvd_momentum_gpu.py",
    "psgd_uvd_param_update_multi_wd": "tests/test_uvd_momentum_gpu.py", "psgd_uvd_param_update_multi_sr": "tests/test_param_rounding_gpu.py",
    "psgd_multi_sumsq_f32": "tests/test_kron_operands_gpu.py", "psgd_multi_param_update_f32": "tests/test_multi_tail2_gpu.py",
    "psgd_multi_diff_scale_f32": "tests/test_kron_operands_gpu.py", "psgd_multi_blend_f32": "tests/test_kron_operands_gpu.py",
    "psgd_multi_scale_check_f32": "tests/test_kron_operands_gpu.py", "psgd_multi_param_update_wd_f32": "tests/test_multi_tail2_gpu.py",
    "psgd_multi_widen_check": "tests/test_multi_tail_half_gpu.py", "psgd_multi_param_update_t": "tests/test_multi_tail_half_gpu.py",
    "psgd_multi_vec_update_f32": "tests/test_multi_vec_gpu.py", "psgd_multi_vec_apply_f32": "tests/test_multi_vec_gpu.py",
    "psgd_multi_narrow_bf16": "tests/test_kron_operands_gpu.py", "psgd_multi_sumsq_mixed": "tests/test_kron_operands_gpu.py",
    "psgd_multi_param_update_mixed": "tests/test_kron_operands_gpu.py", "psgd_multi_param_update_sr": "tests/test_param_rounding_gpu.py",
    "psgd_multi_param_update_mixed_sr": "tests/test_param_rounding_gpu.py", "psgd_multi_randn_f32": "tests/test_multi_randn_gpu.py",
}
_TABLE = {n for names in ENTRY_POINTS.values() for n in names}


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _ints(xs):
    return (ctypes.c_int * len(xs))(*xs)


class _Ordinary:
    """The interface of Arena on ordinary torch allocations (zeroed, each its own): the run that shows an entry point reproducible
    from call to call before check 4 relies on it.  Nothing is guarded here."""

    def __init__(self):
        self.t = {}

    def take(self, shape, dtype, align=16, skew=0, guard=None, name=None, not_better=True):
        self.t[name] = torch.zeros(shape, dtype=dtype, device="cuda:0")
        return self.t[name]

    def take_bytes(self, n, align=256, guard=None, name=None):
        return self.take((int(n),), torch.uint8, name=name)

    def freeze(self, name):
        pass

    def thaw(self, name):
        pass

    def check(self):
        torch.cuda.synchronize()


class _Ctx:
    """One run of a case on one arena (fill None: on ordinary tensors)."""

    def __init__(self, lib, fill):
        self.lib, self.fill, self.A, self.nx = lib, fill, None, 0
        self.st = torch.cuda.current_stream().cuda_stream

    def arena(self, payload_bytes, tensors=32):
        if self.fill is None:
            self.A = _Ordinary()
        else:
            self.A = Arena(int(payload_bytes) + tensors * (2 * 256 * 1024 + 8192) + (1 << 20), self.fill, torch.device("cuda:0"))
        return self.A

    def put(self, name, arr, align=16, skew=0, dtype=torch.float32, freeze=True):
        src = torch.from_numpy(np.ascontiguousarray(arr))
        t = self.A.take(tuple(src.shape), dtype, align=align, skew=skew, name=name)
        t.copy_(src.to(dtype))
        if freeze:
            self.A.freeze(name)
        return t

    def out(self, name, shape, dtype=torch.float32, align=16, skew=0):
        return self.A.take(shape, dtype, align=align, skew=skew, name=name)

    def ws(self, n, name="ws"):
        assert n > 0, (name, n)
        return self.A.take_bytes(int(n), name=name)

    def call(self, name, *args):
        assert name in _TABLE, name + " is not in ENTRY_POINTS"
        rc = getattr(self.lib, name)(*args)
        assert rc == _lib.PSGD_OK, "%s returned %d (%s)" % (name, rc, self.lib.psgd_error_string(int(rc)).decode())

    def wargs(self, ws):
        return ws.data_ptr(), ws.numel(), self.st

    def exchange(self, fold_name, region, stage, N, r, ws):
        """the exchange of a one-rank group: one copy of the send region, folded back (protocol (a) of the header)"""
        off, cnt = region(SEND, stage, N, r)
        self.nx += 1
        gathered = self.A.take((cnt,), torch.float64, name="gathered%d" % self.nx)       # [world = 1][count], read-only
        gathered.copy_(ws[off:off + 8 * cnt].view(torch.float64))
        self.A.freeze("gathered%d" % self.nx)
        self.call(fold_name, stage, gathered.data_ptr(), 1, N, r, *self.wargs(ws))


def _same_bits(a, b):
    return a.numel() == 0 or torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _both(hip_lib, case, *args):
    """Run case(ctx, *args) -> (outputs, parity): twice on ordinary tensors (the call must be reproducible before check 4 can mean
    anything), then on both fills; checks 1 - 4 here, then parity(outputs of the first guarded run)."""
    plain = []
    for _ in range(2):
        c = _Ctx(hip_lib, None)
        outs, _ = case(c, *args)
        c.A.check()
        plain.append({k: v.clone() for k, v in outs.items()})
    for k in plain[0]:
        assert _same_bits(plain[0][k], plain[1][k]), ("output %r is not reproducible from call to call on ordinary tensors: max |diff| %g"
                                                       % (k, float((plain[0][k].double() - plain[1][k].double()).abs().max())))
    runs = []
    for fill in FILLS:
        c = _Ctx(hip_lib, fill)
        outs, parity = case(c, *args)
        c.A.check()                                   # (synchronises)
        runs.append(({k: v.clone() for k, v in outs.items()}, parity))
        del c
    a, b = runs[0][0], runs[1][0]
    for k in a:
        assert torch.isfinite(a[k].float()).all() and torch.isfinite(b[k].float()).all(), "output %r is not finite" % k
        assert _same_bits(a[k], b[k]), ("output %r depends on the bytes outside the extents / in the untouched workspace: max |diff| %g"
                      % (k, float((a[k].double() - b[k].double()).abs().max())))
    runs[0][1]({k: v.cpu() for k, v in a.items()})


def _np64(t):
    return t.float().numpy().astype(np.float64)


# ================================================================================================ UVd, fp32 state, r <= 32
UVD_SHAPES = [(7, 10), (63, 20), (65, 20), (777, 3), (1000, 1), (1021, 10), (2049, 32), (4099, 7)]
UVD_MODES = ["apply", "apply_sweeps", "update_U", "update_V", "update_sweeps", "update_apply", "fused_sweeps", "ipuvt", "ipuvt_cols",
             "apply_cols", "blocks"]


def _uvd_problem(N, r, balance):
    p = make_uvd_problem(N, r, seed=3 * N + r, uv_gain=2.0 if N >= r else 0.5, d_spread=0.3)       # (tests/test_uvd_gpu.py)
    if balance:
        p["U"] = p["U"] * np.float32(3.0)
    return p


def _uvd_place(c, p, ws_bytes, state_dtype=torch.float32):
    N, r = p["U"].shape
    c.arena(ws_bytes + 3 * N * r * 4 + 64 * N)
    t = {"U": c.put("U", p["U"], dtype=state_dtype), "V": c.put("V", p["V"], dtype=state_dtype),
         "d": c.put("d", p["d"][:, 0], dtype=state_dtype),
         "g": c.put("g", p["g"][:, 0], skew=1), "v": c.put("v", p["v"][:, 0], skew=2), "h": c.put("h", p["h"][:, 0], skew=3)}
    t["ws"] = c.ws(ws_bytes)
    return t


def _uvd_case(c, N, r, mode):
    lib = c.lib
    balance = mode in ("update_U", "update_V", "update_sweeps", "update_apply")
    upd_U = mode in ("update_U", "update_sweeps", "fused_sweeps")
    p = _uvd_problem(N, r, balance)
    t = _uvd_place(c, p, lib.psgd_uvd_workspace_bytes(N, r))
    P = lambda k: t[k].data_ptr()
    w = c.wargs(t["ws"])
    q = {k: v.astype(np.float64) for k, v in p.items()}
    X = lambda stage: c.exchange("psgd_uvd_fold_gathered_f64", _lib.ws_region, stage, N, r, t["ws"])
    outs = {}

    def state_parity(o, with_out):
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=balance, update_U=upd_U)
        for k in ("U", "V"):
            assert rel_err(o[k].numpy(), q[k]) < UVD_STATE_TOL, k
        assert rel_err(o["d"].numpy()[:, None], q["d"]) < UVD_STATE_TOL
        if not balance:
            ch = "U" if upd_U else "V"
            assert np.array_equal(o["V" if upd_U else "U"].numpy(), p["V" if upd_U else "U"])
            assert rel_err(o[ch].numpy().astype(np.float64) - p[ch], q[ch] - p[ch]) < UVD_INCR_TOL
        if with_out:
            assert rel_err(o["out"].numpy()[:, None], orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])) < UVD_APPLY_TOL

    if mode in ("apply", "apply_sweeps"):
        out = outs["out"] = c.out("out", (N,), skew=3)
        if mode == "apply":
            c.call("psgd_uvd_apply_f32", P("U"), P("V"), P("d"), P("g"), out.data_ptr(), N, r, *w)
        else:
            c.call("psgd_uvd_apply_sweep1_f32", P("V"), P("d"), P("g"), N, r, *w)
            X(1)
            c.call("psgd_uvd_apply_sweep2_f32", P("U"), P("d"), P("g"), out.data_ptr(), N, r, 1, *w)
            X(2)
            c.call("psgd_uvd_apply_sweep3_f32", P("V"), P("d"), out.data_ptr(), N, r, 1, *w)
        ref = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])

        def par(o):
            assert rel_err(o["out"].numpy()[:, None], ref) < UVD_APPLY_TOL
        return outs, par

    if mode in ("update_U", "update_V", "update_sweeps", "update_apply", "fused_sweeps"):
        for k in ("U", "V", "d"):
            c.A.thaw(k)
            outs[k] = t[k]
        fused = mode in ("update_apply", "fused_sweeps")
        if fused:
            outs["out"] = c.out("out", (N,), skew=3)
            po = outs["out"].data_ptr()
        if mode in ("update_U", "update_V"):
            c.call("psgd_uvd_update_f32", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, STEP, TINY32, 1, int(upd_U), *w)
        elif mode == "update_apply":
            c.call("psgd_uvd_update_apply_f32", P("U"), P("V"), P("d"), P("v"), P("h"), P("g"), po, N, r, STEP, TINY32, 1, int(upd_U), *w)
        elif mode == "update_sweeps":
            c.call("psgd_uvd_balance_max_f32", P("U"), P("V"), N, r, *w)
            X(10)
            c.call("psgd_uvd_balance_scale_f32", P("U"), P("V"), N, r, *w)
            c.call("psgd_uvd_update_sweep1_f32", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, *w)
            X(11)
            c.call("psgd_uvd_update_sweep2_f32", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, STEP, TINY32, int(upd_U), *w)
            X(12)
            c.call("psgd_uvd_update_sweep3_f32", P("d"), N, r, STEP, TINY32, *w)
        else:
            c.call("psgd_uvd_update_sweep1_f32", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, *w)
            X(11)
            c.call("psgd_uvd_update_sweep2_fused_f32", P("U"), P("V"), P("d"), P("v"), P("h"), P("g"), N, r, STEP, TINY32, int(upd_U), *w)
            X(13)
            c.call("psgd_uvd_fused_post_f32", N, r, STEP, TINY32, int(upd_U), *w)
            c.call("psgd_uvd_fused_final_f32", P("U"), P("V"), P("d"), P("g"), po, N, r, STEP, TINY32, *w)
        return outs, lambda o: state_parity(o, fused)

    if mode == "ipuvt":
        out = outs["out"] = c.out("out", (N,), skew=3)
        c.call("psgd_uvd_ipuvt_matvec_f32", P("U"), P("V"), P("g"), out.data_ptr(), N, r, *w)
        ref = orc.IpUVtmatvec(q["U"], q["V"], q["g"])

        def par(o):
            assert rel_err(o["out"].numpy()[:, None], ref) < UVD_APPLY_TOL
        return outs, par

    if mode in ("ipuvt_cols", "apply_cols"):
        xs = [t["g"], t["v"], t["h"]]                                     # k = 3: skews 1, 2, 3
        os_ = [c.out("out%d" % j, (N,), skew=s) for j, s in enumerate((3, 1, 2))]
        for j, o in enumerate(os_):
            outs["out%d" % j] = o
        if mode == "ipuvt_cols":
            c.call("psgd_uvd_ipuvt_matvec_cols_f32", P("U"), P("V"), _ptrs(xs), _ptrs(os_), 3, N, r, *w)
            refs = [orc.IpUVtmatvec(q["U"], q["V"], q[k]) for k in ("g", "v", "h")]
        else:
            c.call("psgd_uvd_apply_cols_f32", P("U"), P("V"), P("d"), _ptrs(xs), _ptrs(os_), 3, N, r, *w)
            refs = [orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q[k]) for k in ("g", "v", "h")]

        def par(o):
            for j in range(3):
                assert rel_err(o["out%d" % j].numpy()[:, None], refs[j]) < UVD_APPLY_TOL, j
        return outs, par

    assert mode == "blocks"          # the contiguous building blocks of the chunked wide-rank path, on U
    parts = _blocks_start(c, t["U"], N, r, [t["g"], t["v"]], outs, w, None)
    c.A.thaw("U")
    outs["M"] = t["U"]
    return _blocks_finish(c, parts, t["U"], None, N, r, w, q["U"], outs, lambda res: res["M"].numpy())


def _blocks_start(c, M, N, rc, xs, outs, w, ld):
    """colsums and axpy_cols on M (contiguous when ld is None, else the *_ld forms on the view M of row stride ld)"""
    rng = np.random.default_rng(N + rc)
    S = outs["S"] = c.out("S", (2, rc), dtype=torch.float64)
    coef = c.put("coef", rng.standard_normal((2, rc)).astype(np.float32))
    c2 = c.put("c2", rng.standard_normal(2 * rc).astype(np.float32))
    o = [c.out("ax%d" % j, (N,), skew=3 - j) for j in range(2)]
    outs["ax0"], outs["ax1"] = o
    if ld is None:
        c.call("psgd_uvd_colsums_f32", M.data_ptr(), _ptrs(xs), 2, S.data_ptr(), N, rc, *w)
        c.call("psgd_uvd_axpy_cols_f32", M.data_ptr(), _ptrs(xs), _ptrs(o), 2, coef.data_ptr(), N, rc, *w)
    else:
        c.call("psgd_uvd_colsums_ld_f32", M.data_ptr(), ld, _ptrs(xs), 2, S.data_ptr(), N, rc, *w)
        c.call("psgd_uvd_axpy_cols_ld_f32", M.data_ptr(), ld, _ptrs(xs), _ptrs(o), 2, coef.data_ptr(), N, rc, *w)
    return [_np64(x.cpu()) for x in xs], _np64(coef.cpu()), _np64(c2.cpu()), xs, c2


def _blocks_finish(c, parts, M, ld, N, rc, w, M64, outs, get_M):
    """... then the rank-2 update, which writes M; get_M(results) returns the updated [N, rc] block"""
    x64, coef64, c264, (a, b), c2 = parts
    if ld is None:
        c.call("psgd_uvd_rank2_update_f32", M.data_ptr(), a.data_ptr(), b.data_ptr(), c2.data_ptr(), N, rc, *w)
    else:
        c.call("psgd_uvd_rank2_update_ld_f32", M.data_ptr(), ld, a.data_ptr(), b.data_ptr(), c2.data_ptr(), N, rc, *w)

    def par(res):
        want = np.stack([M64.T @ x64[0], M64.T @ x64[1]])
        assert np.linalg.norm(res["S"].numpy() - want) / np.linalg.norm(want) < BLOCK_TOL
        for j in range(2):
            assert rel_err(res["ax%d" % j].numpy(), x64[j] + M64 @ coef64[j]) < BLOCK_TOL, j
        wantM = M64 - (np.outer(x64[0], c264[:rc]) - np.outer(x64[1], c264[rc:]))
        assert rel_err(get_M(res), wantM) < BLOCK_TOL
    return outs, par


@pytest.mark.parametrize("mode", UVD_MODES)
@pytest.mark.parametrize("N,r", UVD_SHAPES)
def test_uvd_f32(hip_lib, N, r, mode):
    _both(hip_lib, _uvd_case, N, r, mode)


@pytest.mark.parametrize("fill", FILLS)
def test_the_check_sees_a_kernel_store_outside_the_declared_extent(hip_lib, fill):
    """Teeth, on the device: the apply is handed an `out` that starts one float BEFORE the extent the test declared (inside the
    arena's guard, memory the test owns), so the kernel's first store lands in the guard and its last float stays unwritten --
    check() must name `out`, the side and the distance.  With the extent declared honestly the same call passes."""
    from tests.guard_bands import GuardError
    N, r = 1021, 10
    for shift in (0, 1):
        c = _Ctx(hip_lib, fill)
        t = _uvd_place(c, _uvd_problem(N, r, False), hip_lib.psgd_uvd_workspace_bytes(N, r))
        out = c.out("out", (N,), skew=3)
        c.call("psgd_uvd_apply_f32", t["U"].data_ptr(), t["V"].data_ptr(), t["d"].data_ptr(), t["g"].data_ptr(),
               out.data_ptr() - 4 * shift, N, r, *c.wargs(t["ws"]))
        if shift == 0:
            c.A.check()
            continue
        name, side, off, _ = c.A.damage()
        assert (name, side, off) == ("out", "before", -4)
        with pytest.raises(GuardError, match="before 'out': 4 byte"):
            c.A.check()


# ================================================================================================ whole-matrix ranks 33 .. 64
WIDE_SHAPES = [(31, 57), (2049, 33), (2049, 41), (2049, 64)]
WIDE_MODES = ["gram", "apply_cols", "update_U", "update_V", "update_apply", "blocks"]


def _wide_problem(N, r):
    p = make_uvd_problem(N, r, seed=N + r, uv_gain=2.0 * r ** 0.5, d_spread=0.3)                  # (test_wide_rank_matches_oracle)
    p["V"] = (0.6 * p["U"] @ np.linalg.qr(np.random.default_rng(r).standard_normal((r, r)))[0] + 0.6 * p["V"]).astype(np.float32)
    return p


def _wide_case(c, N, r, mode):
    lib = c.lib
    p = _wide_problem(N, r)
    size = {"gram": lib.psgd_uvd_gram_wide_scratch_bytes, "apply_cols": lib.psgd_uvd_wide_scratch_bytes,
            "update_U": lib.psgd_uvd_wide_update_scratch_bytes, "update_V": lib.psgd_uvd_wide_update_scratch_bytes,
            "update_apply": lib.psgd_uvd_wide_update_apply_scratch_bytes, "blocks": lib.psgd_uvd_wide_scratch_bytes}[mode](N, r)
    t = _uvd_place(c, p, size)
    P = lambda k: t[k].data_ptr()
    w = c.wargs(t["ws"])
    q = {k: v.astype(np.float64) for k, v in p.items()}
    outs = {}
    if mode == "gram":
        nc = 2 * r + 2
        G = outs["G"] = c.out("G", (nc, nc), dtype=torch.float64)
        c.call("psgd_uvd_gram_wide_f32", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, G.data_ptr(), *w)
        d32, v32, h32 = p["d"], p["v"], p["h"]
        W = np.concatenate([q["U"], q["V"], (d32 * h32).astype(np.float64), (v32 / d32).astype(np.float64)], 1)   # (fp32 columns, as the kernel forms them)
        ref = W.T @ W

        def par(o):
            sc = np.sqrt(np.maximum(np.diag(ref), 1e-60))
            assert np.max(np.abs(o["G"].numpy() - ref) / (sc[:, None] * sc[None, :])) < WIDE_GRAM_TOL
        return outs, par
    if mode == "apply_cols":
        xs = [t["g"], t["v"], t["h"]]
        os_ = [c.out("out%d" % j, (N,), skew=s) for j, s in enumerate((3, 1, 2))]
        for j, o in enumerate(os_):
            outs["out%d" % j] = o
        c.call("psgd_uvd_wide_apply_cols_f32", P("U"), P("V"), P("d"), _ptrs(xs), _ptrs(os_), 3, N, r, *w)
        refs = [orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q[k]) for k in ("g", "v", "h")]

        def par(o):
            for j in range(3):
                assert rel_err(o["out%d" % j].numpy()[:, None], refs[j]) < UVD_APPLY_TOL, j
        return outs, par
    if mode in ("update_U", "update_V", "update_apply"):
        upd_U = mode != "update_V"
        for k in ("U", "V", "d"):
            c.A.thaw(k)
            outs[k] = t[k]
        if mode == "update_apply":
            outs["out"] = c.out("out", (N,), skew=3)
            c.call("psgd_uvd_wide_update_apply_f32", P("U"), P("V"), P("d"), P("v"), P("h"), P("g"), outs["out"].data_ptr(), N, r, STEP,
                   TINY32, int(upd_U), *w)
        else:
            c.call("psgd_uvd_wide_update_f32", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, STEP, TINY32, int(upd_U), *w)

        def par(o):                                                   # (bars of test_wide_rank_matches_oracle: 2 x on this path)
            orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=False, update_U=upd_U)
            for k in ("U", "V"):
                assert rel_err(o[k].numpy(), q[k]) < 2 * UVD_STATE_TOL, k
            assert rel_err(o["d"].numpy()[:, None], q["d"]) < 2 * UVD_STATE_TOL
            ch, fr = ("U", "V") if upd_U else ("V", "U")
            assert np.array_equal(o[fr].numpy(), p[fr])
            assert rel_err(o[ch].numpy().astype(np.float64) - p[ch], q[ch] - p[ch]) < UVD_INCR_TOL
            if mode == "update_apply":
                assert rel_err(o["out"].numpy()[:, None], orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])) < 2 * UVD_APPLY_TOL
        return outs, par
    # blocks
    rng = np.random.default_rng(N + r)
    xs = [t["g"], t["v"]]
    S = outs["S"] = c.out("S", (2, r), dtype=torch.float64)
    coef = c.put("coef", rng.standard_normal((2, r)).astype(np.float32))
    c2 = c.put("c2", rng.standard_normal(2 * r).astype(np.float32))
    o = [c.out("ax%d" % j, (N,), skew=3 - j) for j in range(2)]
    outs["ax0"], outs["ax1"] = o
    c.call("psgd_uvd_wide_colsums_f32", P("U"), _ptrs(xs), 2, S.data_ptr(), N, r, *w)
    c.call("psgd_uvd_wide_axpy_cols_f32", P("U"), _ptrs(xs), _ptrs(o), 2, coef.data_ptr(), N, r, c.st)
    c.A.thaw("V")
    outs["M"] = t["V"]
    c.call("psgd_uvd_wide_rank2_update_f32", P("V"), P("g"), P("v"), c2.data_ptr(), N, r, c.st)
    x64 = [q["g"][:, 0], q["v"][:, 0]]
    coef64, c264 = coef.cpu().numpy().astype(np.float64), c2.cpu().numpy().astype(np.float64)

    def par(res):
        want = np.stack([q["U"].T @ x64[0], q["U"].T @ x64[1]])
        assert np.linalg.norm(res["S"].numpy() - want) / np.linalg.norm(want) < BLOCK_TOL
        for j in range(2):
            assert rel_err(res["ax%d" % j].numpy(), x64[j] + q["U"] @ coef64[j]) < BLOCK_TOL, j
        assert rel_err(res["M"].numpy(), q["V"] - (np.outer(x64[0], c264[:r]) - np.outer(x64[1], c264[r:]))) < BLOCK_TOL
    return outs, par


@pytest.mark.parametrize("mode", WIDE_MODES)
@pytest.mark.parametrize("N,r", WIDE_SHAPES)
def test_uvd_wide(hip_lib, N, r, mode):
    _both(hip_lib, _wide_case, N, r, mode)


# ================================================================================================ *_ld: column views of a parent
# (ld, first column, width): the chunks psgd_tf_amd/uvd_wide.py cuts out of an [N, ld] parent; the last one ends at the parent's
# last byte.  Width-32 views need ld % 4 == 0 (the header): they exist in the ld = 100 parent only.
LD_VIEWS = [(100, 0, 32), (100, 68, 32), (100, 99, 1), (65, 0, 1), (65, 64, 1)]


def _ld_case(c, N, ld, lo, rc, mode):
    lib = c.lib
    rng = np.random.default_rng(N + ld + lo)
    ws_bytes = lib.psgd_uvd_workspace_bytes(N, rc)
    c.arena(ws_bytes + 3 * N * ld * 4 + 64 * N)
    sc = 2.0 / (N * rc) ** 0.5
    Wn = (rng.standard_normal((N, ld)) * sc).astype(np.float32)
    W2n = (rng.standard_normal((N, ld)) * sc).astype(np.float32)
    W = c.put("W", Wn)
    view = W[:, lo:lo + rc]
    assert view.data_ptr() + ((N - 1) * ld + rc) * 4 <= W.data_ptr() + N * ld * 4
    x = c.put("x", rng.standard_normal(N).astype(np.float32), skew=1)
    y = c.put("y", rng.standard_normal(N).astype(np.float32), skew=2)
    ws = c.ws(ws_bytes)
    w = c.wargs(ws)
    outs = {}
    M64 = Wn[:, lo:lo + rc].astype(np.float64)
    if mode == "blocks":
        parts = _blocks_start(c, view, N, rc, [x, y], outs, w, ld)
        c.A.thaw("W")
        outs["W"] = W
        keep = np.ones(ld, dtype=bool)
        keep[lo:lo + rc] = False

        def get_M(res):
            got = res["W"].numpy()
            assert np.array_equal(got[:, keep], Wn[:, keep]), "columns of the parent outside the view were written"
            return got[:, lo:lo + rc]
        return _blocks_finish(c, parts, view, ld, N, rc, w, M64, outs, get_M)
    # the Gram sweep on a pair of views, continued by sweeps 2 and 3 on contiguous copies: the update against the oracle
    W2 = c.put("W2", W2n)
    view2 = W2[:, lo:lo + rc]
    p = dict(U=Wn[:, lo:lo + rc].copy(), V=W2n[:, lo:lo + rc].copy(), d=np.exp(0.3 * rng.standard_normal((N, 1))).astype(np.float32),
             v=x.cpu().numpy()[:, None], h=y.cpu().numpy()[:, None])
    U = c.put("U", p["U"], freeze=False)
    V = c.put("V", p["V"])
    d = c.put("d", p["d"][:, 0], freeze=False)
    c.call("psgd_uvd_update_sweep1_ld_f32", view.data_ptr(), ld, view2.data_ptr(), ld, d.data_ptr(), x.data_ptr(), y.data_ptr(), N, rc, *w)
    c.call("psgd_uvd_update_sweep2_f32", U.data_ptr(), V.data_ptr(), d.data_ptr(), x.data_ptr(), y.data_ptr(), N, rc, STEP, TINY32, 1, *w)
    c.call("psgd_uvd_update_sweep3_f32", d.data_ptr(), N, rc, STEP, TINY32, *w)
    outs.update(U=U, d=d)
    q = {k: a.astype(np.float64) for k, a in p.items()}

    def par(o):
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=False, update_U=True)
        assert rel_err(o["U"].numpy(), q["U"]) < UVD_STATE_TOL and rel_err(o["d"].numpy()[:, None], q["d"]) < UVD_STATE_TOL
        assert rel_err(o["U"].numpy().astype(np.float64) - p["U"], q["U"] - p["U"]) < UVD_INCR_TOL
    return outs, par


@pytest.mark.parametrize("mode", ["blocks", "gram"])
@pytest.mark.parametrize("ld,lo,rc", LD_VIEWS)
@pytest.mark.parametrize("N", [31, 2049])
def test_uvd_ld_views(hip_lib, N, ld, lo, rc, mode):
    _both(hip_lib, _ld_case, N, ld, lo, rc, mode)


@pytest.mark.parametrize("N", [31, 2049])
def test_uvd_ld_view_with_an_unaligned_stride_is_refused_and_nothing_is_written(hip_lib, N):
    """rank 32 reads 16 bytes at a time: ld = 65 is PSGD_ERR_ALIGN (include/psgd_hip.h; the callers copy such a chunk)"""
    c = _Ctx(hip_lib, 0xFF)
    ws_bytes = hip_lib.psgd_uvd_workspace_bytes(N, 32)
    c.arena(ws_bytes + N * 65 * 4 + 64 * N)
    W = c.put("W", np.ones((N, 65), dtype=np.float32))
    x = c.put("x", np.ones(N, dtype=np.float32), skew=1)
    S = c.out("S", (1, 32), dtype=torch.float64)
    c.A.freeze("S")
    ws = c.ws(ws_bytes)
    c.A.freeze("ws")
    assert hip_lib.psgd_uvd_colsums_ld_f32(W.data_ptr(), 65, _ptrs([x]), 1, S.data_ptr(), N, 32, *c.wargs(ws)) == _lib.PSGD_ERR_ALIGN
    assert hip_lib.psgd_uvd_rank2_update_ld_f32(W.data_ptr(), 65, x.data_ptr(), x.data_ptr(), x.data_ptr(), N, 32, *c.wargs(ws)) == _lib.PSGD_ERR_ALIGN
    c.A.check()


# ================================================================================================ UVd, bf16 state
UVD_BF16_SHAPES = [(65, 20), (1021, 10), (2049, 32)]
UVD_BF16_MODES = ["apply", "apply_sweeps", "update_U", "update_V", "update_sweeps", "update_apply", "fused_sweeps"]


def _uvd_bf16_case(c, N, r, mode):
    lib = c.lib
    balance = mode in ("update_U", "update_sweeps", "update_apply")
    upd_U = mode in ("update_U", "update_sweeps", "fused_sweeps")
    p = make_uvd_problem(N, r, seed=3 * r + N % 89, d_spread=0.3)                                     # (tests/test_uvd_bf16_gpu.py problem())
    for k in ("U", "V", "d"):
        p[k] = to_bf16_np(p[k])
    if balance:
        p["U"] = to_bf16_np(p["U"] * np.float32(3.0))
    t = _uvd_place(c, p, lib.psgd_uvd_bf16_workspace_bytes(N, r), state_dtype=torch.bfloat16)
    P = lambda k: t[k].data_ptr()
    w = c.wargs(t["ws"])
    q = {k: v.astype(np.float64) for k, v in p.items()}
    X = lambda stage: c.exchange("psgd_uvd_bf16_fold_gathered_f64", _lib.uvd_bf16_ws_region, stage, N, r, t["ws"])
    outs = {}
    if mode in ("apply", "apply_sweeps"):
        out = outs["out"] = c.out("out", (N,), skew=3)
        if mode == "apply":
            c.call("psgd_uvd_apply_bf16", P("U"), P("V"), P("d"), P("g"), out.data_ptr(), N, r, *w)
        else:
            c.call("psgd_uvd_apply_sweep1_bf16", P("V"), P("d"), P("g"), N, r, *w)
            X(1)
            c.call("psgd_uvd_apply_sweep2_bf16", P("U"), P("d"), P("g"), out.data_ptr(), N, r, *w)
            X(2)
            c.call("psgd_uvd_apply_sweep3_bf16", P("V"), P("d"), out.data_ptr(), N, r, *w)
        ref = orc.precond_grad_UVd_math(q["U"], q["V"], q["d"], q["g"])

        def par(o):
            assert rel_err(o["out"].numpy()[:, None], ref) < BF16_STATE_APPLY_TOL
        return outs, par
    for k in ("U", "V", "d"):
        c.A.thaw(k)
        outs[k] = t[k]
    fused = mode in ("update_apply", "fused_sweeps")
    if fused:
        outs["out"] = c.out("out", (N,), skew=3)
        po = outs["out"].data_ptr()
    bal, uu = int(balance), int(upd_U)
    if mode in ("update_U", "update_V"):
        c.call("psgd_uvd_update_bf16", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, STEP, TINY32, bal, uu, 0, 0, *w)
    elif mode == "update_apply":
        c.call("psgd_uvd_update_apply_bf16", P("U"), P("V"), P("d"), P("v"), P("h"), P("g"), po, N, r, STEP, TINY32, bal, uu, 0, 0, *w)
    else:
        if balance:
            c.call("psgd_uvd_balance_max_bf16", P("U"), P("V"), N, r, *w)
            X(10)
        c.call("psgd_uvd_update_gram_bf16", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, *w)
        X(11)
        c.call("psgd_uvd_update_rewrite_bf16", P("U"), P("V"), P("d"), P("v"), P("h"), N, r, STEP, TINY32, bal, uu, 0, 0, 0, *w)
        X(12)
        if mode == "update_sweeps":
            c.call("psgd_uvd_update_d_bf16", P("d"), N, r, STEP, TINY32, 0, 0, 0, *w)
        else:
            c.call("psgd_uvd_apply_sweep1_d_bf16", P("V"), P("d"), P("g"), N, r, STEP, TINY32, 0, 0, 0, *w)
            X(1)
            c.call("psgd_uvd_apply_sweep2_bf16", P("U"), P("d"), P("g"), po, N, r, *w)
            X(2)
            c.call("psgd_uvd_apply_sweep3_bf16", P("V"), P("d"), po, N, r, *w)

    def par(o):
        orc.update_precond_UVd_math_(q["U"], q["V"], q["d"], q["v"], q["h"], STEP, TINY32, balance=balance, update_U=upd_U)
        stored = {"U": _np64(o["U"]), "V": _np64(o["V"]), "d": _np64(o["d"])[:, None]}
        for k in ("U", "V", "d"):      # the element bound of tests/uvd_cases.py check_bf16_state: the right code or its neighbour
            bound = 2.0 ** -7 * np.abs(q[k]) + 1e-5 * float(np.sqrt(np.mean(q[k] * q[k])))
            assert np.all(np.abs(stored[k] - q[k]) <= bound), (k, float(np.max(np.abs(stored[k] - q[k]) - bound)))
        if not balance:
            fr = "V" if upd_U else "U"
            assert np.array_equal(stored[fr], p[fr].astype(np.float64))
        if fused:
            ref = orc.precond_grad_UVd_math(stored["U"], stored["V"], stored["d"], q["g"])
            assert rel_err(o["out"].numpy()[:, None], ref) < BF16_STATE_APPLY_TOL
    return outs, par


@pytest.mark.parametrize("mode", UVD_BF16_MODES)
@pytest.mark.parametrize("N,r", UVD_BF16_SHAPES)
def test_uvd_bf16_state(hip_lib, N, r, mode):
    _both(hip_lib, _uvd_bf16_case, N, r, mode)


def _narrow_case(c, count):
    c.arena(8 * max(count, 1))
    rng = np.random.default_rng(count)
    n = max(count, 1)                      # count = 0: one-element operands, and the destination must keep its pattern
    src_np = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
    src = c.put("src", src_np, align=16, skew=1)
    dst = c.out("dst", (n,), dtype=torch.bfloat16, align=16, skew=3)            # 2-byte aligned only
    if count == 0:
        c.A.freeze("dst")
    c.call("psgd_uvd_bf16_narrow_f32", src.data_ptr(), dst.data_ptr(), count, 0, 0, 0, 0, c.st)

    def par(o):           # rounding 0 is round to nearest even: the codes of torch's conversion (tests/test_uvd_checkpoint_gpu.py)
        want = torch.from_numpy(src_np).to(torch.bfloat16)
        assert torch.equal(o["dst"].view(torch.int16), want.view(torch.int16))
    return ({"dst": dst} if count else {}), (par if count else (lambda o: None))


@pytest.mark.parametrize("count", [0, 1, 7, 8, 9, 4097])
def test_uvd_bf16_narrow(hip_lib, count):
    _both(hip_lib, _narrow_case, count)


# ================================================================================================ sparse LU
SPLU_SHAPES = [(12, 12), (65, 64), (1021, 7), (273, 41)]
SPLU_NAMES = ("L12", "l3", "U12", "u3")


def _splu_case(c, N, r, mode, bf16=False):
    lib = c.lib
    p = make_splu_problem(N, r, seed=N + r)
    n2 = N - r
    sd = torch.bfloat16 if bf16 else torch.float32
    if bf16:
        for k in SPLU_NAMES:
            p[k] = to_bf16_np(p[k])
    ws_bytes = (lib.psgd_splu_bf16_workspace_bytes if bf16 else lib.psgd_splu_workspace_bytes)(N, r)
    c.arena(ws_bytes + 8 * N * r * 4 + 64 * N, tensors=32)
    # L12 (and every bf16 state tensor) 16-byte aligned; fp32 U12, l3, u3 and the vectors need 4 bytes only
    va = dict(align=16, skew=0) if bf16 else None
    t = {"L12": c.put("L12", p["L12"], dtype=sd), "U12": c.put("U12", p["U12"], dtype=sd, **(va or dict(skew=1)))}
    for k, s in (("l3", 2), ("u3", 3)):
        t[k] = c.put(k, p[k][:, 0], dtype=sd, **(va or dict(skew=s))) if n2 else None
    for k, s in (("g", 1), ("dx", 2), ("dg", 3)):
        t[k] = c.put(k, p[k][:, 0], skew=s)
    ws = c.ws(ws_bytes)
    w = c.wargs(ws)
    P = lambda k: t[k].data_ptr() if t[k] is not None else None
    st4 = (P("L12"), P("l3"), P("U12"), P("u3"))
    q = {k: v.astype(np.float64) for k, v in p.items()}
    X = lambda stage: c.exchange("psgd_splu_fold_gathered_f64", _lib.splu_ws_region, stage, N, r, ws)
    outs = {}
    if mode in ("apply", "apply_stages"):
        out = outs["out"] = c.out("out", (N,), skew=2)
        if bf16:
            c.call("psgd_splu_apply_bf16", *st4, P("g"), out.data_ptr(), N, r, *w)
        elif mode == "apply":
            c.call("psgd_splu_apply_f32", *st4, P("g"), out.data_ptr(), N, r, *w)
        else:
            c.call("psgd_splu_stage1_f32", P("U12"), P("g"), N, r, *w)
            X(1)
            c.call("psgd_splu_apply_stage2_f32", *st4, P("g"), out.data_ptr(), N, r, *w)
            X(2)
            c.call("psgd_splu_apply_stage3_f32", *st4, out.data_ptr(), N, r, *w)
        ref = orc.precond_grad_splu(q["L12"], q["l3"], q["U12"], q["u3"], [q["g"]])[0]

        def par(o):
            assert rel_err(o["out"].numpy()[:, None], ref) < (BF16_STATE_APPLY_TOL if bf16 else SPLU_APPLY_TOL)
        return outs, par
    new = {"L12": c.out("L12n", (N, r), dtype=sd), "U12": c.out("U12n", (r, N), dtype=sd, **(va or dict(skew=3)))}
    for k, s in (("l3", 1), ("u3", 2)):
        new[k] = c.out(k + "n", (n2,), dtype=sd, **(va or dict(skew=s))) if n2 else None
    PN = lambda k: new[k].data_ptr() if new[k] is not None else None
    nw4 = (PN("L12"), PN("l3"), PN("U12"), PN("u3"))
    for k in SPLU_NAMES:
        if new[k] is not None:
            outs[k] = new[k]
    if bf16:
        c.call("psgd_splu_update_bf16", *st4, P("dx"), P("dg"), *nw4, N, r, STEP, TINY32, 0, 0, *w)
    elif mode == "update":
        c.call("psgd_splu_update_f32", *st4, P("dx"), P("dg"), *nw4, N, r, STEP, TINY32, *w)
    else:
        c.call("psgd_splu_stage1_f32", P("U12"), P("dg"), N, r, *w)
        X(1)
        c.call("psgd_splu_update_stage2_f32", *st4, P("dx"), P("dg"), N, r, *w)
        X(2)
        c.call("psgd_splu_update_stage3_f32", *st4, P("dx"), P("dg"), N, r, *w)
        X(3)
        c.call("psgd_splu_update_stage4_f32", *st4, P("dx"), P("dg"), *nw4, N, r, STEP, TINY32, int(n2 > 0), *w)

    def par(o):
        with np.errstate(all="ignore"):
            ref = orc.update_precond_splu(q["L12"], q["l3"], q["U12"], q["u3"], [q["dx"]], [q["dg"]], STEP)
        for k, b in zip(SPLU_NAMES, ref):
            if k not in o:
                continue
            if bf16:        # tests/test_splu_bf16_gpu.py: every stored code is the oracle's nearest code or its neighbour
                from tests.test_splu_bf16_gpu import off_by
                assert off_by([o[k]], [b]).max() <= 1, k
            else:           # tests/test_splu_gpu.py: state and increment
                got = o[k].numpy().astype(np.float64).reshape(b.shape)
                assert rel_err(got, b) < SPLU_STATE_TOL, k
                assert rel_err(got - q[k], b - q[k]) < SPLU_INCR_TOL, k
    return outs, par


@pytest.mark.parametrize("mode", ["apply", "apply_stages", "update", "update_stages"])
@pytest.mark.parametrize("N,r", SPLU_SHAPES)
def test_splu_f32(hip_lib, N, r, mode):
    _both(hip_lib, _splu_case, N, r, mode)


@pytest.mark.parametrize("mode", ["apply", "update"])
@pytest.mark.parametrize("N,r", [(n, r) for n, r in SPLU_SHAPES if r <= 32] + [(65, 32)])      # (65, 32): one tile + 1 at the top rank
def test_splu_bf16_state(hip_lib, N, r, mode):
    _both(hip_lib, _splu_case, N, r, mode, True)


# ================================================================================================ dense
def _dense_case(c, n, mode):
    from tests.test_dense_gpu import _problem
    Q, dx, dg, g = _problem(n, False, seed=n)
    ws_bytes = c.lib.psgd_dense_workspace_bytes(n)
    c.arena(ws_bytes + 3 * n * n * 4)
    tQ = c.put("Q", Q, skew=1)                       # the dense Q may sit at any float
    ws = c.ws(ws_bytes)
    w = c.wargs(ws)
    Q64 = Q.astype(np.float64)
    if mode == "update":
        tdx, tdg = c.put("dx", dx, skew=2), c.put("dg", dg, skew=3)
        Qo = c.out("Qout", (n, n), skew=3)
        c.call("psgd_dense_update_f32", tQ.data_ptr(), tdx.data_ptr(), tdg.data_ptr(), Qo.data_ptr(), n, STEP, TINY32, *w)
        ref = orc.update_precond_dense(Q64, [dx.astype(np.float64)], [dg.astype(np.float64)], step=STEP)

        def par(o):
            got = o["Qout"].numpy()
            assert rel_err(got, ref) < DENSE_TOL
            assert rel_err(got.astype(np.float64) - Q64, ref - Q64) < DENSE_INCR_TOL
        return {"Qout": Qo}, par
    tg = c.put("g", g, skew=1)
    out = c.out("out", (n,), skew=3)
    c.call("psgd_dense_apply_f32", tQ.data_ptr(), tg.data_ptr(), out.data_ptr(), n, *w)
    ref = orc.precond_grad_dense(Q64, [g.astype(np.float64)])[0]

    def par(o):
        assert rel_err(o["out"].numpy().reshape(ref.shape), ref) < DENSE_TOL
    return {"out": out}, par


@pytest.mark.parametrize("mode", ["update", "apply"])
@pytest.mark.parametrize("n", [5, 67, 256, 257])
def test_dense(hip_lib, n, mode):
    _both(hip_lib, _dense_case, n, mode)


# ================================================================================================ step tail: the two that take no list of outputs
def _sumsq_case(c, N):
    c.arena(4 * N + _lib.UVD_SUMSQ_WS_BYTES)
    n = max(N, 1)                     # N = 0: a one-element operand that must not be read (its NaN would reach the sum)
    xs = (np.random.default_rng(N).standard_normal(n) * 3.0).astype(np.float32)
    if N == 0:
        x = c.out("x", (1,), skew=1)
        c.A.freeze("x")
    else:
        x = c.put("x", xs, skew=1 + N % 3)
    out = c.out("out", (1,), dtype=torch.float64, align=8)
    ws = c.A.take_bytes(_lib.UVD_SUMSQ_WS_BYTES, align=8, name="ws")           # exactly PSGD_UVD_SUMSQ_WS_BYTES, 8-byte aligned
    c.call("psgd_uvd_sumsq_f32", x.data_ptr(), N, out.data_ptr(), ws.data_ptr(), ws.numel(), c.st)
    ref = float(np.sum((xs * xs).astype(np.float64))) if N else 0.0             # (tests/test_uvd_tail_gpu.py test_sumsq: fp32 squares, fp64 sum)

    def par(o):
        got = float(o["out"].item())
        assert abs(got - ref) <= 1e-12 * ref                                    # test_sumsq's bar; N = 0: exactly +0 (test_sumsq_of_nothing_is_zero)
        if N == 0:
            assert int(o["out"].view(torch.int64).item()) == 0
    return {"out": out}, par


@pytest.mark.parametrize("N", [0, 1, 3, 4, 5, 63, 64, 65, 255, 257, 4095, 4097, 8193])
def test_uvd_sumsq(hip_lib, N):
    _both(hip_lib, _sumsq_case, N)


CHECK_SIZES = (1, 4097, 0, 63, 8192)


def _check_multi_case(c, dtype, code, bad):
    from psgd_tf_amd.preconditioned_stochastic_gradient_descent import uvd_tail_chunks
    c.arena(16 * sum(CHECK_SIZES))
    rng = np.random.default_rng(code + 10 * bad)
    ts = []
    for i, n in enumerate(CHECK_SIZES):
        a = rng.standard_normal(max(n, 1)).astype(np.float32)
        if bad and i == 1:
            a[-1] = np.inf                                   # the last element of a segment that ends one past a chunk
        ts.append(c.put("p%d" % i, a[:n] if n else a, skew=1 + i % 3, dtype=dtype) if n else None)
    starts = np.cumsum((0,) + CHECK_SIZES[:-1])
    segs = np.array([[t.data_ptr() if t is not None else 0, s, n] for t, s, n in zip(ts, starts, CHECK_SIZES)], dtype=np.int64)
    chunks = uvd_tail_chunks(CHECK_SIZES)
    tsegs = c.put("segs", segs, dtype=torch.int64)
    tchunks = c.put("chunks", chunks, dtype=torch.int64)
    flag = c.put("flag", np.zeros(1, dtype=np.int32), dtype=torch.int32, skew=1, freeze=not bad)      # never zeroed by the kernels
    c.call("psgd_uvd_check_multi", tsegs.data_ptr(), len(CHECK_SIZES), tchunks.data_ptr(), int(chunks.shape[0]), code, 1.0, flag.data_ptr(),
           7, c.st)

    def par(o):                                              # (tests/test_uvd_guard_gpu.py: the stamp exactly when a value is not finite)
        assert int(o["flag"].item()) == (7 if bad else 0)
    return {"flag": flag}, par


@pytest.mark.parametrize("bad", [0, 1])
@pytest.mark.parametrize("dtype,code", [(torch.float32, _lib.DTYPE_F32), (torch.bfloat16, _lib.DTYPE_BF16), (torch.float16, _lib.DTYPE_F16)])
def test_uvd_check_multi(hip_lib, dtype, code, bad):
    _both(hip_lib, _check_multi_case, dtype, code, bad)


# ================================================================================================ Kron dense (x) dense, fp32
KRON_SHAPES = [(1, 3), (3, 3), (33, 129), (129, 33), (151, 16), (85, 10), (16, 40), (257, 257)]


def _tri(rng, n, off=0.05):
    return np.triu(rng.standard_normal((n, n)) * off, 1) + np.diag(np.exp(0.3 * rng.standard_normal(n)))


def _kron_problem(M, N):
    """the data of tests/test_kron_gpu.py test_dense_dense_update (rho != 1), plus a gradient"""
    rng = np.random.default_rng(M * 77 + N)
    Ql, Qr = _tri(rng, M) * 3.0, _tri(rng, N)
    dX = rng.standard_normal((M, N))
    dG = (np.eye(M) + 0.1 * np.diag(rng.uniform(0, 5, M))) @ dX @ (np.eye(N) + 0.1 * np.diag(rng.uniform(0, 5, N)))
    G = rng.standard_normal((M, N))
    return [a.astype(np.float32) for a in (Ql, Qr, dX, dG, G)]


def _kron_update_parity(got_l, got_r, a64):
    Ql_r, Qr_r = orc.update_precond_kron(a64[0], a64[1], a64[2], a64[3], STEP)
    assert rel_err(got_l, Ql_r) < KRON_TOL and rel_err(got_r, Qr_r) < KRON_TOL
    rho = np.sqrt(np.max(np.diag(a64[0])) / np.max(np.diag(a64[1])))
    for got, ref, base in ((got_l, Ql_r, a64[0] / rho), (got_r, Qr_r, a64[1] * rho)):
        if np.linalg.norm(ref - base) > 0:
            assert rel_err(got.astype(np.float64) - base, ref - base) < KRON_INCR_TOL


def _kron_case(c, M, N, mode):
    lib = c.lib
    a32 = _kron_problem(M, N)
    a64 = [a.astype(np.float64) for a in a32]
    ws_bytes = lib.psgd_kron_dd_workspace_bytes(M, N)
    c.arena(ws_bytes + 4 * (2 * M * M + 2 * N * N + 4 * M * N))
    Ql, Qr = c.put("Ql", a32[0]), c.put("Qr", a32[1])
    ws = c.ws(ws_bytes)
    w = c.wargs(ws)
    if mode == "update":
        dX, dG = c.put("dX", a32[2]), c.put("dG", a32[3])
        Lo, Ro = c.out("QlOut", (M, M)), c.out("QrOut", (N, N))
        c.call("psgd_kron_dd_update_f32", Ql.data_ptr(), Qr.data_ptr(), dX.data_ptr(), dG.data_ptr(), Lo.data_ptr(), Ro.data_ptr(), M, N,
               STEP, TINY32, *w)
        return {"QlOut": Lo, "QrOut": Ro}, lambda o: _kron_update_parity(o["QlOut"].numpy(), o["QrOut"].numpy(), a64)
    G = c.put("G", a32[4])
    out = c.out("out", (M, N))
    ptrs = (Ql.data_ptr(), Qr.data_ptr(), G.data_ptr(), out.data_ptr(), M, N)
    if mode == "apply":
        c.call("psgd_kron_dd_apply_f32", *ptrs, *w)
    elif mode == "apply_direct":
        c.call("psgd_kron_dd_apply_direct_f32", *ptrs, *w)
    else:
        c.call("psgd_kron_dd_prepare_f32", Ql.data_ptr(), Qr.data_ptr(), M, N, *w)
        c.call("psgd_kron_dd_apply_prepared_f32", *ptrs, *w)
    ref = orc.precond_grad_kron(a64[0], a64[1], a64[4])

    def par(o):
        assert rel_err(o["out"].numpy(), ref) < KRON_TOL
    return {"out": out}, par


@pytest.mark.parametrize("mode", ["apply", "apply_direct", "prepared", "update"])
@pytest.mark.parametrize("M,N", KRON_SHAPES)
def test_kron_dd_f32(hip_lib, M, N, mode):
    _both(hip_lib, _kron_case, M, N, mode)


def _large_routes():
    """(run, skipped): per distinct route-flag value of the shapes of tests/test_kron_routes_gpu.py its smallest shape -- run when no
    side exceeds 1100.  Host only (psgd_kron_dd_route_flags makes no HIP call)."""
    from tests.test_kron_routes_gpu import ENTRIES
    lib = _lib.load()
    best = {}
    for M, N, _, _ in ENTRIES:
        f = lib.psgd_kron_dd_route_flags(M, N)
        if f not in best or M * N < best[f][0] * best[f][1]:
            best[f] = (M, N)
    run = sorted(s for s in best.values() if max(s) <= 1100)
    skipped = sorted((f, s) for f, s in best.items() if max(s) > 1100)
    return run, skipped


LARGE_ROUTE_SHAPES = [(513, 100), (513, 384), (599, 300), (600, 300), (1000, 1024)]
LARGE_ROUTE_SKIPPED = [(846, (4096, 4097)), (862, (2817, 4226)), (894, (4096, 4096)), (9182, (1024, 2048)), (17358, (2049, 8192)),
                       (17374, (768, 3072)), (24966, (511, 2560)), (25566, (512, 2560)), (33158, (128, 4096)), (33758, (256, 4096))]


def test_large_route_lists_are_the_ones_named(hip_lib):
    """the shapes run below and the routes named as skipped are what the rule gives under the library's route flags today"""
    run, skipped = _large_routes()
    assert run == LARGE_ROUTE_SHAPES and skipped == LARGE_ROUTE_SKIPPED


@pytest.mark.parametrize("mode", ["apply", "apply_direct", "prepared", "update"])
@pytest.mark.parametrize("M,N", LARGE_ROUTE_SHAPES)
def test_kron_dd_f32_large_routes(hip_lib, M, N, mode):
    _both(hip_lib, _kron_case, M, N, mode)


def _kron_batched_case(c, mode):
    lib = c.lib
    shapes = KRON_SHAPES
    Ms, Ns = [m for m, _ in shapes], [n for _, n in shapes]
    ws_bytes = lib.psgd_kron_dd_workspace_bytes_batched(_ints(Ms), _ints(Ns), len(shapes))
    c.arena(ws_bytes + sum(4 * (2 * m * m + 2 * n * n + 4 * m * n) for m, n in shapes), tensors=6 * len(shapes) + 4)
    probs = [_kron_problem(m, n) for m, n in shapes]
    Ql = [c.put("Ql%d" % i, p[0]) for i, p in enumerate(probs)]
    Qr = [c.put("Qr%d" % i, p[1]) for i, p in enumerate(probs)]
    ws = c.ws(ws_bytes)
    w = c.wargs(ws)
    outs = {}
    cnt = len(shapes)
    if mode == "update":
        dX = [c.put("dX%d" % i, p[2]) for i, p in enumerate(probs)]
        dG = [c.put("dG%d" % i, p[3]) for i, p in enumerate(probs)]
        Lo = [c.out("Lo%d" % i, (m, m)) for i, m in enumerate(Ms)]
        Ro = [c.out("Ro%d" % i, (n, n)) for i, n in enumerate(Ns)]
        c.call("psgd_kron_dd_update_batched_f32", _ptrs(Ql), _ptrs(Qr), _ptrs(dX), _ptrs(dG), _ptrs(Lo), _ptrs(Ro), _ints(Ms), _ints(Ns),
               cnt, STEP, TINY32, *w)
        for i in range(cnt):
            outs["L%d" % i], outs["R%d" % i] = Lo[i], Ro[i]

        def par(o):
            for i, p in enumerate(probs):
                _kron_update_parity(o["L%d" % i].numpy(), o["R%d" % i].numpy(), [a.astype(np.float64) for a in p])
        return outs, par
    G = [c.put("G%d" % i, p[4]) for i, p in enumerate(probs)]
    out = [c.out("out%d" % i, s) for i, s in enumerate(shapes)]
    if mode == "apply":
        c.call("psgd_kron_dd_apply_batched_f32", _ptrs(Ql), _ptrs(Qr), _ptrs(G), _ptrs(out), _ints(Ms), _ints(Ns), cnt, *w)
    else:
        c.call("psgd_kron_dd_prepare_batched_f32", _ptrs(Ql), _ptrs(Qr), _ints(Ms), _ints(Ns), cnt, *w)
        c.call("psgd_kron_dd_apply_prepared_batched_f32", _ptrs(Ql), _ptrs(Qr), _ptrs(G), _ptrs(out), _ints(Ms), _ints(Ns), cnt, *w)
    for i in range(cnt):
        outs["out%d" % i] = out[i]

    def par(o):
        for i, p in enumerate(probs):
            a64 = [a.astype(np.float64) for a in p]
            assert rel_err(o["out%d" % i].numpy(), orc.precond_grad_kron(a64[0], a64[1], a64[4])) < KRON_TOL, shapes[i]
    return outs, par


@pytest.mark.parametrize("mode", ["apply", "prepared", "update"])
def test_kron_dd_f32_batched(hip_lib, mode):
    _both(hip_lib, _kron_batched_case, mode)


# ================================================================================================ Kron, bf16 operands
def _kron_bf16_case(c, M, N, mode):
    lib = c.lib
    rng = np.random.default_rng(M + 3 * N)
    Ql, Qr = _tri(rng, M).astype(np.float32), _tri(rng, N).astype(np.float32)
    if mode == "update":
        Ql = Ql * np.float32(3.0)
    dXn, Gn = to_bf16_np(rng.standard_normal((M, N)).astype(np.float32)), to_bf16_np(rng.standard_normal((M, N)).astype(np.float32))
    dGn = to_bf16_np(((np.eye(M) + 0.1 * np.diag(rng.uniform(0, 5, M))) @ dXn @ (np.eye(N) + 0.1 * np.diag(rng.uniform(0, 5, N)))).astype(np.float32))
    ws_bytes = (lib.psgd_kron_dd_update_workspace_bytes_bf16 if mode == "update" else lib.psgd_kron_dd_workspace_bytes_bf16)(M, N)
    c.arena(ws_bytes + 4 * (2 * M * M + 2 * N * N + 4 * M * N))
    tl, tr = c.put("Ql", Ql), c.put("Qr", Qr)
    ws = c.ws(ws_bytes)
    w = c.wargs(ws)
    a64 = [Ql.astype(np.float64), Qr.astype(np.float64), dXn.astype(np.float64), dGn.astype(np.float64), Gn.astype(np.float64)]
    if mode == "update":
        dX, dG = c.put("dX", dXn, dtype=torch.bfloat16), c.put("dG", dGn, dtype=torch.bfloat16)
        Lo, Ro = c.out("QlOut", (M, M)), c.out("QrOut", (N, N))
        c.call("psgd_kron_dd_update_bf16", tl.data_ptr(), tr.data_ptr(), dX.data_ptr(), dG.data_ptr(), Lo.data_ptr(), Ro.data_ptr(), M, N,
               STEP, TINY32, *w)

        def par(o):                                             # (tests/test_kron_gpu.py test_dense_dense_update_bf16)
            rl, rr = orc.update_precond_kron(a64[0], a64[1], a64[2], a64[3], STEP)
            gl, gr = o["QlOut"].numpy(), o["QrOut"].numpy()
            assert rel_err(gl, rl) < KRON_BF16_UPD_STATE_TOL and rel_err(gr, rr) < KRON_BF16_UPD_STATE_TOL
            rho = np.sqrt(np.max(np.diag(a64[0])) / np.max(np.diag(a64[1])))
            assert rel_err(gl.astype(np.float64) - a64[0] / rho, rl - a64[0] / rho) < KRON_BF16_UPD_TOL
            assert rel_err(gr.astype(np.float64) - a64[1] * rho, rr - a64[1] * rho) < KRON_BF16_UPD_TOL
        return {"QlOut": Lo, "QrOut": Ro}, par
    G = c.put("G", Gn, dtype=torch.bfloat16)
    out = c.out("out", (M, N), dtype=torch.bfloat16)
    c.call("psgd_kron_bf16_handoff_reset", ws.data_ptr(), M, N, c.st)          # a fresh workspace is reset once (the header)
    if mode == "apply":
        c.call("psgd_kron_dd_apply_bf16", tl.data_ptr(), tr.data_ptr(), G.data_ptr(), out.data_ptr(), M, N, *w)
    else:
        c.call("psgd_kron_bf16_prepare_factors", tl.data_ptr(), tr.data_ptr(), M, N, *w)
        c.call("psgd_kron_dd_apply_bf16_prepared", G.data_ptr(), out.data_ptr(), M, N, *w)
    ref = orc.precond_grad_kron(a64[0], a64[1], a64[4])

    def par(o):
        assert rel_err(o["out"].float().numpy(), ref) < KRON_BF16_TOL
    return {"out": out}, par


@pytest.mark.parametrize("mode", ["apply", "prepared", "update"])
@pytest.mark.parametrize("M,N", [(8, 8), (200, 72)])
def test_kron_dd_bf16_operands(hip_lib, M, N, mode):
    _both(hip_lib, _kron_bf16_case, M, N, mode)


# ================================================================================================ Kron, sparse formats
SPARSE_SHAPES = [(5, 10), (5, 50), (16, 40), (40, 16)]
SPARSE_FMT = {"ds": 0, "nd": 1, "ns": 2}


def _norm_factor(rng, n):
    q = np.stack([np.exp(0.2 * rng.standard_normal(n)), 0.1 * rng.standard_normal(n)])
    q[1, -1] = 0.0
    return q


def _sparse_case(c, fmt, M, N, gap, mode):
    lib = c.lib
    rng = np.random.default_rng(100 * M + N + SPARSE_FMT[fmt])
    L = _tri(rng, M) if fmt == "ds" else _norm_factor(rng, M)                       # (tests/test_kron_gpu.py _factor_for)
    R = _tri(rng, N) if fmt == "nd" else np.exp(0.2 * rng.standard_normal((1, N)))
    dX, G = rng.standard_normal((M, N)), rng.standard_normal((M, N))
    dG = dX * np.exp(rng.uniform(-1, 1, (M, 1))) * np.exp(rng.uniform(-1, 1, (1, N)))
    a32 = [a.astype(np.float32) for a in (L, R, dX, dG, G)]
    a64 = [a.astype(np.float64) for a in a32]
    ws_bytes = lib.psgd_kron_sparse_workspace_bytes(SPARSE_FMT[fmt], M, N)
    c.arena(ws_bytes + 64 * (M + N + gap) * (M + N + gap))
    rs = N + gap

    def strided(name, a):
        """[M, N] data in an [M, rs] parent whose gap columns keep the arena's pattern; the whole parent is read-only"""
        t = c.out(name, (M, rs))
        t[:, :N].copy_(torch.from_numpy(a))
        c.A.freeze(name)
        return t
    tL = c.put("L", a32[0], skew=0 if fmt == "ds" else 1)
    tR = c.put("R", a32[1].reshape(-1) if fmt != "nd" else a32[1], skew=0 if fmt == "nd" else 2)
    ws = c.ws(ws_bytes)
    w = c.wargs(ws)
    if mode == "update":
        tX, tG = strided("dX", a32[2]), strided("dG", a32[3])
        Lo = c.out("Lout", a32[0].shape, skew=0 if fmt == "ds" else 3)
        Ro = c.out("Rout", tR.shape, skew=0 if fmt == "nd" else 1)
        c.call("psgd_kron_%s_update_f32" % fmt, tL.data_ptr(), tR.data_ptr(), tX.data_ptr(), tG.data_ptr(), rs, 1, Lo.data_ptr(),
               Ro.data_ptr(), M, N, STEP, TINY32, *w)
        rl, rr = orc.update_precond_kron(a64[0], a64[1], a64[2], a64[3], STEP)

        def par(o):
            assert rel_err(o["Lout"].numpy(), rl) < KRON_TOL and rel_err(o["Rout"].numpy().reshape(rr.shape), rr) < KRON_TOL
        return {"Lout": Lo, "Rout": Ro}, par
    tG = strided("G", a32[4])
    out = c.out("out", (M, N))
    c.call("psgd_kron_%s_apply_f32" % fmt, tL.data_ptr(), tR.data_ptr(), tG.data_ptr(), rs, 1, out.data_ptr(), M, N, *w)
    ref = orc.precond_grad_kron(a64[0], a64[1], a64[4])

    def par(o):
        assert rel_err(o["out"].numpy(), ref) < KRON_TOL
    return {"out": out}, par


@pytest.mark.parametrize("mode", ["update", "apply"])
@pytest.mark.parametrize("gap", [0, 3])
@pytest.mark.parametrize("M,N", SPARSE_SHAPES)
@pytest.mark.parametrize("fmt", sorted(SPARSE_FMT))
def test_kron_sparse_formats(hip_lib, fmt, M, N, gap, mode):
    _both(hip_lib, _sparse_case, fmt, M, N, gap, mode)
