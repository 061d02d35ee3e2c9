"""The grouped QUAD update and apply (include/psgd_kron_quad_list_hip.h, psgd_kron_qlist.hip): for every layer of a list the bits
of the per-layer entry points on cloned inputs, and the per-layer bars against the float64 restatement of tests/kron_quad_cases.py
(state 1e-5, increment 2e-3, apply 1e-5).  The lists put single-tile and multi-tile layers, partial tiles, ragged K, both load
routes and both apply orders into one grid; k = 37 takes the bisection deep; the reversed list shows that list order is nothing."""
import functools

import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import kron_quad, kron_quad_list
from tests import kron_quad_cases as qc
from tests.guard_bands import DEFAULT_GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = qc.T
# (M, N, seed of qc.problem: the seeds of qc.CASES, and one found for (5, T + 1))
MIXED = [(1, 1, 0), (1, 7, 1), (7, 1, 2), (T - 1, T + 1, 4), (T, T, 5), (T + 1, 2 * T + 3, 6), (33, 515, 7), (2 * T, 3 * T, 11)]
CYCLE = [(3, 5, 3), (T, T, 5), (5, T + 1, 20)]
LISTS = {"mixed": MIXED, "one-full-tile": [MIXED[4]], "one-ragged": [MIXED[5]], "k37": [CYCLE[i % 3] for i in range(37)],
         "reversed": MIXED[::-1]}
SMALL_CAP = 2 * 3328          # two 1 x 1-sized carves (13 regions of 256 bytes each): groups of two and of one


@functools.lru_cache(maxsize=None)
def _second_step(case):
    """float64 (Ql, Qr, L) after a second update on the same G"""
    p = qc.problem(*case)
    return qc.quad_update_ref(p["new_Ql"], p["new_Qr"], p["new_L"], p["G"].double())


def _states(cases):
    ps = [qc.problem(*c) for c in cases]
    return ps, {k: [p[k].to(DEV).clone() for p in ps] for k in ("Ql", "Qr", "L", "G")}


def _check_apply(cases, ps, listed, single, key):
    for c, p, a, b in zip(cases, ps, listed, single):
        e = qc.err(a, p[key])
        print(c, key, "apply %.2e" % e)
        assert torch.equal(a, b), (c, key)
        assert e < qc.APPLY_BAR, (c, key, e)


def _check_update(cases, listed, single, olds, refs):
    for i, c in enumerate(cases):
        for k, j in (("Ql", 0), ("Qr", 1)):
            new, ref, old = listed[k][i], refs[i][j], olds[i][j]
            e, ei = qc.err(new, ref), qc.err(new.double().cpu() - old, ref - old)
            print(c, k, "state %.2e increment %.2e" % (e, ei))
            assert torch.equal(new, single[k][i]), (c, k)
            assert e < qc.STATE_BAR and ei < qc.INCREMENT_BAR, (c, k, e, ei)
        assert torch.equal(listed["L"][i], single["L"][i]) and qc.err(listed["L"][i], refs[i][2]) < qc.L_BAR, (c, "L")


@pytest.mark.parametrize("name, cap", [(n, None) for n in LISTS] + [("mixed", SMALL_CAP)], ids=lambda v: str(v))
def test_list_has_the_per_layer_bits_and_holds_the_per_layer_bars(name, cap):
    cases = LISTS[name]
    shapes = [c[:2] for c in cases]
    if cap is not None:                                   # (1,1)+(1,7) fit together; every other layer stands alone, five of them over the cap
        sizes = [kron_quad.load().psgd_kron_quad_workspace_bytes(M, N) for M, N in shapes]
        assert sizes[:3] == [3328] * 3 and min(sizes[3:]) > cap
        assert kron_quad_list.plan_layers(shapes, cap)["groups"] == [(0, 2)] + [(i, i + 1) for i in range(2, 8)]
    plan = psgd.KronQuadListPlan(shapes, DEV, **({} if cap is None else dict(max_group_bytes=cap)))
    ps, a = _states(cases)
    _, b = _states(cases)
    k = len(cases)
    single_apply = lambda: [psgd.precond_grad_kron_quad(b["Ql"][i], b["Qr"][i], b["G"][i]) for i in range(k)]
    _check_apply(cases, ps, psgd.precond_grad_kron_quad_list(a["Ql"], a["Qr"], a["G"], plan=plan), single_apply(), "out")
    olds = [(p["Ql"].double(), p["Qr"].double()) for p in ps]
    for call, refs in enumerate(([(p["new_Ql"], p["new_Qr"], p["new_L"]) for p in ps], [_second_step(c) for c in cases])):
        assert psgd.update_precond_kron_quad_list_(a["Ql"], a["Qr"], a["L"], a["G"], qc.STEP, qc.DECAY, plan=plan) is None
        for i in range(k):
            psgd.update_precond_kron_quad_(b["Ql"][i], b["Qr"][i], b["L"][i], b["G"][i], qc.STEP, qc.DECAY)
        _check_update(cases, a, b, olds, refs)
        if call == 0:                                     # the apply on the new state
            _check_apply(cases, ps, psgd.precond_grad_kron_quad_list(a["Ql"], a["Qr"], a["G"], plan=plan), single_apply(), "out_new")
        olds = [r[:2] for r in refs]
    _, again = _states(cases)                             # repeated calls are bit-identical
    for _ in range(2):
        psgd.update_precond_kron_quad_list_(again["Ql"], again["Qr"], again["L"], again["G"], qc.STEP, qc.DECAY, plan=plan)
    assert all(torch.equal(x, y) for key in ("Ql", "Qr", "L") for x, y in zip(again[key], a[key]))


@pytest.mark.parametrize("entry", ["apply", "update"])
def test_list_stays_inside_every_layers_extents(entry):
    """every operand of every layer between guard bands at bases skewed by 4 bytes, over a workspace of exactly the bytes asked
    for that holds NaN (fill 0xFF): the bands untouched, the frozen operands unchanged, the bits those of the aligned call"""
    shapes = [c[:2] for c in MIXED]
    ps, plain = _states(MIXED)
    lib, plan = kron_quad_list.load(), kron_quad_list.plan_layers(shapes)
    M, N, group_start, raw = plan["raw"]
    k, ws_bytes = len(shapes), plan["ws_bytes"]
    floats = sum(m * m + n * n + 2 * m * n + 2 for m, n in shapes)
    arena = Arena(4 * floats + ws_bytes + raw.nbytes + 152 * k + (5 * k + 3) * (2 * DEFAULT_GUARD + 4096), 0xFF, DEV)
    writes = ("out",) if entry == "apply" else ("Ql", "Qr", "L")
    t = []
    for i, ((m, n), p) in enumerate(zip(shapes, ps)):
        shp = dict(Ql=(m, m), Qr=(n, n), L=(2,), G=(m, n), out=(m, n))
        t.append({key: arena.take(s, torch.float32, align=16, skew=1, name="%s%d" % (key, i)) for key, s in shp.items()})
        for key in shp:
            if key != "out":
                t[i][key].copy_(p[key])
            if key not in writes:
                arena.freeze("%s%d" % (key, i))
    ws = arena.take_bytes(ws_bytes)
    rows = torch.zeros((k, 19), dtype=torch.int64)
    for i, (m, n) in enumerate(shapes):
        rows[i, :5] = torch.tensor([t[i][key].data_ptr() for key in ("Ql", "Qr", "L", "G", "out")])
        rows[i, 5] = m | (n << 32)
    rows[:, 6:] = torch.from_numpy(plan["ws_off"])
    table = arena.take((k, 19), torch.int64, align=16, name="table")
    plan_dev = arena.take((raw.size,), torch.int32, align=16, name="plan")
    table.copy_(rows)
    plan_dev.copy_(torch.from_numpy(raw))
    arena.freeze("table")
    arena.freeze("plan")
    ints = kron_quad_list._ints
    head = (table.data_ptr(), plan_dev.data_ptr(), ints(raw), ints(group_start), len(plan["groups"]), ints(M), ints(N), k)
    tail = (ws.data_ptr(), ws_bytes, torch.cuda.current_stream(DEV).cuda_stream)
    if entry == "apply":
        rc = lib.psgd_kron_qlist_apply_f32(*head, *tail)
        plain["out"] = psgd.precond_grad_kron_quad_list(plain["Ql"], plain["Qr"], plain["G"])
    else:
        rc = lib.psgd_kron_qlist_update_f32(*head, qc.STEP, qc.DECAY, *tail)
        psgd.update_precond_kron_quad_list_(plain["Ql"], plain["Qr"], plain["L"], plain["G"], qc.STEP, qc.DECAY)
    assert rc == 0
    arena.check()
    for i in range(k):
        for key in writes:
            assert bool(torch.isfinite(plain[key][i]).all()) and torch.equal(t[i][key], plain[key][i]), (shapes[i], key)


def test_a_plan_refuses_other_shapes():
    plan = psgd.KronQuadListPlan([(3, 5)], DEV)
    Ql, Qr, L = psgd.kron_quad_initial_state(5, 3, device=DEV)
    with pytest.raises(ValueError, match="the plan was made for"):
        psgd.update_precond_kron_quad_list_([Ql], [Qr], [L], [torch.zeros(5, 3, device=DEV)], 0.1, plan=plan)
