"""include/psgd_kron_quad_list_hip.h without a GPU: symbols exported and bound, argument checks before any HIP call, the planner on
hand-computed lists, and the refusals of the two list functions and of the class switch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import _lib, kron_quad, kron_quad_diag, kron_quad_list
from tests import kron_quad_cases as qc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "psgd_kron_quad_list_hip.h")
T = qc.T
b = lambda n: -(-n // T)                                  # tiles per edge
u = lambda n: b(n) * (b(n) + 1) // 2                      # upper tiles


def test_header_symbols_are_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(psgd_kron_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(kron_quad_list.SIGNATURES) and len(declared) == 4
    assert all(n.startswith("psgd_kron_qlist_") for n in declared)
    raw, lib = ctypes.CDLL(_lib.LIB_PATH), kron_quad_list.load()
    assert all(hasattr(raw, n) and getattr(lib, n).argtypes == kron_quad_list.SIGNATURES[n][1] for n in declared)
    assert not set(declared) & (set(_lib.SIGNATURES) | set(kron_quad.SIGNATURES) | set(kron_quad_diag.SIGNATURES))
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert define("PSGD_KRON_QLIST_WS_REGIONS") == kron_quad_list.WS_REGIONS and define("PSGD_KRON_QLIST_STAGES") == kron_quad_list.STAGES
    assert int(re.search(r"DEFAULT_GROUP_BYTES\s+\((\d+)ll << 20\)", text).group(1)) << 20 == kron_quad_list.DEFAULT_GROUP_BYTES
    assert lib.psgd_abi_version() == 7


def test_argument_checks_return_before_any_hip_call():
    lib, BAD, WS = kron_quad_list.load(), _lib.PSGD_ERR_BAD_ARG, _lib.PSGD_ERR_WORKSPACE
    ints = kron_quad_list._ints
    plan = kron_quad_list.plan_layers([(70, 5), (3, 3)])
    M, N, gs, raw = plan["raw"]
    table, plan_dev, ws, need = 0x10000, 0x20000, 0x30000, plan["ws_bytes"]       # never dereferenced: the checks fail first
    zero, null = np.array([70, 0], dtype=np.int32), ctypes.POINTER(ctypes.c_int32)()
    for args in ((null, ints(N), 2, 1 << 20), (ints(M), null, 2, 1 << 20), (ints(M), ints(N), 0, 1 << 20), (ints(zero), ints(N), 2, 1 << 20),
                 (ints(M), ints(zero), 2, 1 << 20)):
        assert lib.psgd_kron_qlist_workspace_bytes(*args) == BAD
        assert lib.psgd_kron_qlist_plan(*args, ints(gs.copy()), ints(raw.copy()), plan["ws_off"].copy().ctypes.data_as(kron_quad_list._lp)) == BAD
    good = dict(table=table, plan_dev=plan_dev, plan=ints(raw), gs=ints(gs), groups=1, M=ints(M), N=ints(N), k=2)
    wrong_grid = raw.copy()
    wrong_grid[-1] += 1                                                         # the last prefix of the last stage
    bad = [dict(table=None), dict(plan_dev=None), dict(plan=null), dict(gs=null), dict(M=null), dict(N=null), dict(k=0), dict(k=-3),
           dict(M=ints(zero)), dict(N=ints(zero)), dict(groups=0), dict(groups=2), dict(plan=ints(wrong_grid))]
    calls = (lambda a, w: lib.psgd_kron_qlist_apply_f32(*a, *w, None), lambda a, w: lib.psgd_kron_qlist_update_f32(*a, 0.1, 0.95, *w, None))
    for call in calls:
        for change in bad:
            assert call(tuple({**good, **change}.values()), (ws, need)) == BAD, change
        for bad_ws in ((None, need), (ws, need - 1), (ws + 4, need)):
            assert call(tuple(good.values()), bad_ws) == WS


# (shapes, cap in bytes or a function of the per-layer workspace sizes, the groups)
PLANS = [
    ([(T + 1, 2 * T + 3), (3, 5), (2 * T, T), (T, T)], lambda w: sum(w), [(0, 4)]),
    ([(3, 5), (T, T), (T, T), (3, 5), (3, 5)], lambda w: 2 * w[1], [(0, 2), (2, 5)]),
    ([(T, T), (2 * T, 3 * T), (T, T), (5, T + 1)], lambda w: w[0] + w[3], [(0, 1), (1, 2), (2, 4)]),     # the second is over the cap
]


@pytest.mark.parametrize("shapes, cap, groups", PLANS)
def test_planner_groups_orders_and_counts(shapes, cap, groups):
    lib = kron_quad.load()
    w = [lib.psgd_kron_quad_workspace_bytes(M, N) for M, N in shapes]
    cap = cap(w)
    p = kron_quad_list.plan_layers(shapes, cap)
    assert p["groups"] == groups
    assert all(sum(w[g0:g1]) <= cap or g1 - g0 == 1 for g0, g1 in groups) and any(w[g0] > cap for g0, _ in groups) == (len(groups) == 3)
    assert p["ws_bytes"] == max(sum(w[g0:g1]) for g0, g1 in groups)
    for g0, g1 in groups:                                                       # the carves of a group tile its block in list order
        assert p["ws_off"][g0:g1, 0].tolist() == [sum(w[g0:i]) for i in range(g0, g1)]
    assert (p["ws_off"] % 256 == 0).all() and (np.diff(p["ws_off"], axis=1) > 0).all()
    keys = dict(prod_m=lambda M, N: M, prod_n=lambda M, N: N, prod_min=min, prod_max=max, upper=max, full=max)
    counts = dict(upper=lambda M, N: u(M) + u(N), full=lambda M, N: b(M) ** 2 + b(N) ** 2)
    for stage, key in keys.items():
        order, prefix = p["order"][stage], p["prefix"][stage]
        want = [i for g0, g1 in groups for i in sorted(range(g0, g1), key=lambda i: (-key(*shapes[i]), i))]
        assert order == want, stage
        count = counts.get(stage, lambda M, N: b(M) * b(N))
        assert prefix == np.concatenate([[0], np.cumsum([count(*shapes[i]) for i in order])]).tolist(), stage
    if len(groups) == 1:                                                        # the first list, by hand
        assert p["order"]["prod_m"] == [2, 0, 3, 1] and p["order"]["prod_n"] == [0, 2, 3, 1] and p["order"]["upper"] == [0, 2, 3, 1]
        assert p["prefix"]["prod_m"] == [0, 2, 8, 9, 10] and p["prefix"]["upper"] == [0, 9, 13, 15, 17]
        assert p["prefix"]["full"] == [0, 13, 18, 20, 22]


def test_functions_and_class_refuse_by_name():
    Ql, Qr, L = psgd.kron_quad_initial_state(3, 5)
    G, out = torch.zeros(3, 5), torch.zeros(3, 5)
    upd, app = psgd.update_precond_kron_quad_list_, psgd.precond_grad_kron_quad_list
    with pytest.raises(ValueError, match="equal length"):
        upd([Ql, Ql.clone()], [Qr], [L], [G], 0.1)
    with pytest.raises(TypeError, match="Qr of layer 0 must be float32"):
        app([Ql], [Qr.double()], [G])
    with pytest.raises(ValueError, match="G of layer 0 must be contiguous"):
        app([Ql], [Qr], [torch.zeros(5, 3).T])
    with pytest.raises(ValueError, match="L of layer 0 must have shape"):
        upd([Ql], [Qr], [torch.zeros(3)], [G], 0.1)
    with pytest.raises(ValueError, match="Qr of layer 0 is a scale factor"):
        upd([Ql], [torch.ones(1, 5)], [L], [G], 0.1)
    with pytest.raises(ValueError, match="Ql of layer 0 and Ql of layer 1 share memory"):
        upd([Ql, Ql], [Qr, Qr.clone()], [L, L.clone()], [G, G], 0.1)
    with pytest.raises(ValueError, match="share memory"):
        app([Ql], [Qr], [G], [G])
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        app([Ql, Ql], [Qr, Qr], [G, G], [out, out.clone()])                     # read operands may repeat; then the device is judged
    with pytest.raises(_lib.PsgdHipError, match="no CPU fallback"):
        psgd.KronQuadListPlan([(3, 5)], "cpu")
    x = [torch.zeros(3, 5, requires_grad=True)]
    with pytest.raises(ValueError, match="quad_route"):
        psgd.Kron(x, preconditioner_fit="whitening", preconditioner_update="quad", quad_route="group")
    with pytest.raises(ValueError, match="quad_route"):
        psgd.Kron(x, preconditioner_fit="whitening", quad_route="list")
