"""include/psgd_kron_quad_nd_list_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, the planner
(slice rule, workgroup counts, orders, groups) on hand-computed lists, and the refusals of the class switch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, kron_quad_nd, kron_quad_nd_list as qtl

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_kron_quad_nd_list_hip.h")
T = 64
b = lambda n: -(-n // T)                                  # tiles per edge
u = lambda n: b(n) * (b(n) + 1) // 2                      # upper tiles


def test_header_symbols_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psgd_kron_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(qtl.SIGNATURES) and len(declared) == 4 and all(n.startswith("psgd_kron_qtl_") for n in declared)
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), qtl.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == qtl.SIGNATURES[n][1] for n in declared)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(kron_quad_nd.SIGNATURES))
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert define("PSGD_KRON_QTL_WS_REGIONS") == qtl.WS_REGIONS and define("PSGD_KRON_QTL_STAGES") == qtl.STAGES == len(qtl.STAGE_NAMES)
    assert define("PSGD_KRON_QTL_DEFAULT_SLICE_K") == qtl.DEFAULT_GRAM_SLICE_K
    assert _lib.PSGD_ABI_VERSION == 7 == lib.psgd_abi_version()
    for name in ("KronQuadTensorListPlan", "update_precond_kron_quad_nd_list_", "precond_grad_kron_quad_nd_list"):
        assert getattr(psgd, name) is getattr(qtl, name)


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS, ints = qtl.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE, qtl._ints
    plan = qtl.plan_layers([(70, 5, 9), (3, 3, 3)], gram_slice_k=16)
    A, B, C, gs, raw = plan["raw"]
    table, plan_dev, ws, need = 0x10000, 0x20000, 0x30000, plan["ws_bytes"]      # never dereferenced: the checks fail first
    zero, huge, null = np.array([70, 0], dtype=np.int32), np.array([1 << 20, 3], dtype=np.int32), ctypes.POINTER(ctypes.c_int32)()
    good = dict(A=ints(A), B=ints(B), C=ints(C), k=2, cap=1 << 30, gsk=16)
    outs = (ints(gs.copy()), ints(raw.copy()), plan["ws_off"].copy().ctypes.data_as(qtl._lp), ints(np.zeros(6, dtype=np.int32)))
    for change in (dict(A=null), dict(B=null), dict(C=null), dict(k=0), dict(A=ints(zero)), dict(C=ints(zero)),
                   dict(A=ints(huge), B=ints(huge)), dict(gsk=0), dict(gsk=24), dict(gsk=-16)):
        args = tuple({**good, **change}.values())
        assert lib.psgd_kron_qtl_workspace_bytes(*args) == BAD, change
        assert lib.psgd_kron_qtl_plan(*args, *outs) == BAD, change
    good = dict(table=table, plan_dev=plan_dev, plan=ints(raw), gs=ints(gs), groups=1, A=ints(A), B=ints(B), C=ints(C), k=2, gsk=16)
    wrong_grid = raw.copy()
    wrong_grid[-1] += 1                                                         # the last prefix of the last stage
    bad = [dict(table=None), dict(plan_dev=None), dict(plan=null), dict(gs=null), dict(A=null), dict(C=null), dict(k=0), dict(k=-3),
           dict(B=ints(zero)), dict(groups=0), dict(groups=2), dict(plan=ints(wrong_grid)), dict(gsk=8), dict(gsk=40),
           dict(gsk=32)]                                                        # (32: another slice count than the plan's)
    calls = (lambda a, w: lib.psgd_kron_qtl_apply_f32(*a, *w, None), lambda a, w: lib.psgd_kron_qtl_update_f32(*a, 0.1, 0.95, *w, None))
    for call in calls:
        for change in bad:
            assert call(tuple({**good, **change}.values()), (ws, need)) == BAD, change
        for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
            assert call(tuple(good.values()), bad_ws) == WS


def _slices(n, K, gsk):
    """the slice rule of the header, restated"""
    steps = -(-K // 16)
    S = min(-(-steps * 16 // gsk), max(1, 256 // u(n)))
    per = -(-steps // S)
    return -(-steps // per), per


def test_slice_rule_by_hand():
    p = qtl.plan_layers([(512, 512, 9), (64, 64, 9), (3, 65, 9), (70, 66, 3), (1024, 8, 8)], gram_slice_k=1024)
    # 512 x 512 x 9: sides a, b have 36 upper tiles (256 / 36 = 7) and K = 4608: ceil(288 / 5) = 58 steps, 5 slices; side c is one
    # tile over K = 262144: 256 slices of 64 steps.  64 x 64 x 9: K = 576 < 1024 and 4096.  1024 x 8 x 8: u(1024) = 136, one slice
    assert p["slices"] == [(5, 5, 256), (1, 1, 4), (1, 1, 1), (1, 1, 5), (1, 8, 8)]
    p = qtl.plan_layers([(3, 65, 9), (6, 64, 64)], gram_slice_k=48)
    # (3, 65, 9): K = 585 / 27 / 195 -> 37 / 2 / 13 steps; side b has 3 upper tiles.  (6, 64, 64): K = 4096 / 384 / 384
    assert p["slices"] == [(13, 1, 5), (86, 8, 8)] and _slices(3, 585, 48) == (13, 3) and _slices(6, 4096, 48) == (86, 3)


# (shapes, cap as a function of the per-layer carve sizes, the groups)
PLANS = [
    ([(T + 1, 2 * T + 3, 9), (3, 5, 2), (2 * T, T, 3), (1, T, T)], lambda w: sum(w), [(0, 4)]),
    ([(3, 5, 2), (T, T, 9), (T, T, 9), (3, 5, 2), (3, 5, 2)], lambda w: 2 * w[1], [(0, 2), (2, 5)]),
    ([(T, T, 4), (2 * T, 3 * T, 5), (T, T, 4), (5, T + 1, 3)], lambda w: w[0] + w[3], [(0, 1), (1, 2), (2, 4)]),   # the second is over the cap
]


@pytest.mark.parametrize("gsk", [16, 1024])
@pytest.mark.parametrize("shapes, cap, groups", PLANS)
def test_planner_groups_orders_and_counts(shapes, cap, groups, gsk):
    w = [qtl.plan_layers([s], gram_slice_k=gsk)["ws_bytes"] for s in shapes]
    cap = cap(w)
    p = qtl.plan_layers(shapes, cap, gsk)
    assert p["groups"] == groups
    assert all(sum(w[g0:g1]) <= cap or g1 - g0 == 1 for g0, g1 in groups) and any(w[g0] > cap for g0, _ in groups) == (len(groups) == 3)
    assert p["ws_bytes"] == max(sum(w[g0:g1]) for g0, g1 in groups)
    for g0, g1 in groups:                                                       # the carves of a group tile its block in list order
        assert p["ws_off"][g0:g1, 0].tolist() == [sum(w[g0:i]) for i in range(g0, g1)]
    assert (p["ws_off"] % 256 == 0).all() and (np.diff(p["ws_off"], axis=1) >= 0).all()
    dims = lambda s: [(s[0], s[1] * s[2]), (s[1], s[0] * s[2]), (s[2], s[0] * s[1])]      # (n, K) of the three sides
    sl = [[_slices(n, K, gsk) for n, K in dims(s)] for s in shapes]
    assert p["slices"] == [tuple(S for S, _ in r) for r in sl]
    mode = [lambda A, B, C: b(A) * b(B * C), lambda A, B, C: A * b(B) * b(C), lambda A, B, C: b(A * B) * b(C)]
    place = lambda s, i: sorted(range(3), key=lambda m: (s[m], m))[i]
    counts = dict(gram=lambda i: sum(u(n) * S for (n, _), (S, _) in zip(dims(shapes[i]), sl[i])),
                  fold=lambda i: sum(u(n) for (n, _), (S, _) in zip(dims(shapes[i]), sl[i]) if S > 1),
                  upper=lambda i: sum(u(n) for n in shapes[i]), full=lambda i: sum(b(n) ** 2 for n in shapes[i]))
    keys = dict(gram=lambda i: max(min(K, per * 16) for (_, K), (_, per) in zip(dims(shapes[i]), sl[i])),
                fold=lambda i: max(S for S, _ in sl[i]), upper=lambda i: max(shapes[i]), full=lambda i: max(shapes[i]))
    for m in range(3):
        counts["mode_" + "abc"[m]], keys["mode_" + "abc"[m]] = (lambda i, m=m: mode[m](*shapes[i])), (lambda i, m=m: shapes[i][m])
        counts["apply_%d" % m] = lambda i, m=m: mode[place(shapes[i], m)](*shapes[i])
        keys["apply_%d" % m] = lambda i, m=m: shapes[i][place(shapes[i], m)]
    for stage in qtl.STAGE_NAMES:
        order, prefix = p["order"][stage], p["prefix"][stage]
        assert order == [i for g0, g1 in groups for i in sorted(range(g0, g1), key=lambda i: (-keys[stage](i), i))], stage
        assert prefix == np.concatenate([[0], np.cumsum([counts[stage](i) for i in order])]).tolist(), stage
    if len(groups) == 1 and gsk == 1024:                                        # the first list, by hand
        assert p["slices"] == [(2, 1, 9), (1, 1, 1), (1, 1, 8), (4, 1, 1)]
        assert p["order"]["mode_a"] == [2, 0, 1, 3] and p["prefix"]["mode_a"] == [0, 6, 44, 45, 109]
        assert p["order"]["mode_b"] == [0, 2, 3, 1] and p["prefix"]["mode_b"] == [0, 195, 323, 324, 327]
        assert p["order"]["upper"] == [0, 2, 3, 1] and p["prefix"]["upper"] == [0, 10, 15, 18, 21] and p["prefix"]["full"] == [0, 14, 20, 23, 26]
        assert p["order"]["fold"] == [0, 2, 3, 1] and p["prefix"]["fold"] == [0, 4, 5, 6, 6]       # the last layer has nothing to fold


def test_class_and_plan_refuse_by_name():
    x = [torch.zeros(6, 5, 3, 3, requires_grad=True)]
    quad = dict(preconditioner_fit="whitening", preconditioner_update="quad", any_rank=True)
    with pytest.raises(ValueError, match="quad_tensor_route must be"):
        psgd.Kron(x, quad_tensor=True, quad_tensor_route="group", **quad)
    with pytest.raises(ValueError, match="quad_tensor_route='list'.*needs quad_tensor=True"):
        psgd.Kron(x, quad_tensor_route="list", **quad)
    with pytest.raises(ValueError, match="quad_route"):                          # the matrix switch keeps its own refusal
        psgd.Kron(x, quad_tensor=True, quad_tensor_route="list", quad_route="group", **quad)
    with pytest.raises(ValueError, match="one HIP device"):                      # a good value reaches the device check
        psgd.Kron(x, quad_tensor=True, quad_tensor_route="list", **quad)
    with pytest.raises(ValueError, match="multiple of 16"):
        qtl.plan_layers([(3, 4, 5)], gram_slice_k=40)
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        psgd.KronQuadTensorListPlan([(3, 4, 5)], "cpu")
    Qs, L = psgd.kron_quad_nd_initial_state((3, 4, 5))
    G = torch.zeros(3, 4, 5)
    with pytest.raises(ValueError, match="equal length"):
        psgd.update_precond_kron_quad_nd_list_([Qs, Qs], [L], [G], 0.1)
    with pytest.raises(ValueError, match="L of layer 0 must have shape"):
        psgd.update_precond_kron_quad_nd_list_([Qs], [torch.zeros(2)], [G], 0.1)
    with pytest.raises(ValueError, match="share memory"):
        psgd.precond_grad_kron_quad_nd_list([Qs], [G], [G])
