"""The grouped order-3 QUAD update and apply (include/psgd_kron_quad_nd_list_hip.h, psgd_kron_qtlist.hip): the bits of the
per-layer entry points wherever no side is split, and the float64 restatement of tests/kron_quad_nd_cases.py (state 1e-5,
increment 2e-3, apply 1e-5, L 1e-5) where the Gram is split along K.  SPLIT holds the smallest shapes at which a split can go
wrong: slices that begin inside a slab of the segmented K (C = 9, 20), a last slice shorter than the others, and a split side of
two tile rows."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import kron_quad_nd_list as qtl
from tests import kron_quad_cases as qc
from tests import kron_quad_nd_cases as nc
from tests.guard_bands import DEFAULT_GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SPLIT = [c for c in nc.CASES if c[:3] in ((3, 65, 9), (4, 68, 20), (70, 66, 3), (6, 64, 64), (3, 4, 130))]
SMALL_CAP = 100_000           # bytes: the plans below fall into three groups or more (asserted)
ONE_SLICE_K = 8192            # above every Gram length of nc.CASES (the longest: 70 * 66 = 4620): S = 1 on every side


def _state(cases, G=None):
    ps = [nc.problem(*c) for c in cases]
    return ([[Q.to(DEV).clone() for Q in p["Qs"]] for p in ps], [p["L"].to(DEV).clone() for p in ps],
            [(p["G"] if G is None or i not in G else G[i]).to(DEV) for i, p in enumerate(ps)])


def run_list(cases, G=None, **plan_kw):
    """apply -> update -> apply through the list route: (per layer [out, Qa, Qb, Qc, L, out_new], the plan)"""
    Qs, Ls, Gs = _state(cases, G)
    plan = psgd.KronQuadTensorListPlan([c[:3] for c in cases], DEV, **plan_kw)
    out = [o.clone() for o in psgd.precond_grad_kron_quad_nd_list(Qs, Gs, plan=plan)]
    assert psgd.update_precond_kron_quad_nd_list_(Qs, Ls, Gs, qc.STEP, qc.DECAY, plan=plan) is None
    new = psgd.precond_grad_kron_quad_nd_list(Qs, Gs, plan=plan)
    return [[out[i], *Qs[i], Ls[i], new[i]] for i in range(len(cases))], plan


def run_layers(cases):
    Qs, Ls, Gs = _state(cases)
    res = []
    for Q, L, G in zip(Qs, Ls, Gs):
        out = psgd.precond_grad_kron_quad_nd(Q, G)
        psgd.update_precond_kron_quad_nd_(Q, L, G, qc.STEP, qc.DECAY)
        res.append([out, *Q, L, psgd.precond_grad_kron_quad_nd(Q, G)])
    return res


same = lambda x, y: all(torch.equal(a, b) for a, b in zip(x, y))


@pytest.mark.parametrize("reverse, cap, gsk", [(False, None, ONE_SLICE_K), (True, None, ONE_SLICE_K), (False, SMALL_CAP, ONE_SLICE_K),
                                               (True, SMALL_CAP, ONE_SLICE_K), (False, None, None)])
def test_unsplit_layers_have_the_per_layer_bits(reverse, cap, gsk):
    """every layer of nc.CASES in one list.  gsk = None is the default gram_slice_k: it splits the sides with K > 2048, which
    then owe the per-layer bits only in the apply."""
    cases = nc.CASES[::-1] if reverse else nc.CASES
    kw = dict(**({} if cap is None else dict(max_group_bytes=cap)), **({} if gsk is None else dict(gram_slice_k=gsk)))
    listed, plan = run_list(cases, **kw)
    assert cap is None or len(plan.groups) >= 3
    assert gsk is None or plan.slices == [(1, 1, 1)] * len(cases)
    for c, S, a, b in zip(cases, plan.slices, listed, run_layers(cases)):
        assert torch.equal(a[0], b[0]), c
        assert S != (1, 1, 1) or same(a, b), c


@pytest.mark.parametrize("gsk", [16, 48])
def test_split_gram_against_float64(gsk):
    listed, plan = run_list(SPLIT, gram_slice_k=gsk)
    print(gsk, plan.slices)
    assert all(max(S) > 1 for S in plan.slices) and plan.slices[2][0] > 1       # (70, 66, 3): side a, two tile rows, is split
    inc = lambda new, old, ref: qc.err(new.double().cpu() - old.double(), ref - old.double())
    for c, (out, Qa, Qb, Qc, L, out_new) in zip(SPLIT, listed):
        p = nc.problem(*c)
        e = dict(apply=max(qc.err(out, p["out"]), qc.err(out_new, p["out_new"])),
                 state=max(qc.err(Q, ref) for Q, ref in zip((Qa, Qb, Qc), p["new_Qs"])),
                 increment=max(inc(Q, old, ref) for Q, old, ref in zip((Qa, Qb, Qc), p["Qs"], p["new_Qs"])),
                 L=float(((L.double().cpu() - p["new_L"]).abs() / p["new_L"]).max()))
        print(c, " ".join("%s %.2e" % kv for kv in sorted(e.items())))
        assert e["apply"] < qc.APPLY_BAR and e["state"] < qc.STATE_BAR and e["increment"] < qc.INCREMENT_BAR and e["L"] < qc.L_BAR, (c, e)
        assert all(torch.equal(Q, Q.T) for Q in (Qa, Qb, Qc)), c                  # one value written twice
    again, _ = run_list(SPLIT, gram_slice_k=gsk)                                # a second call: the same bits
    other, plan2 = run_list(SPLIT[::-1], gram_slice_k=gsk, max_group_bytes=SMALL_CAP)   # nor do list order and cap matter
    assert len(plan2.groups) >= 3 and plan2.slices == plan.slices[::-1]
    assert all(same(a, b) and same(a, o) for a, b, o in zip(listed, again, other[::-1]))


def test_a_nan_stays_in_its_layer():
    G = nc.problem(*SPLIT[1])["G"].clone()
    G[2, 33, 7] = float("nan")
    clean, _ = run_list(SPLIT, gram_slice_k=48)
    dirty, _ = run_list(SPLIT, G={1: G}, gram_slice_k=48)
    assert all(bool(torch.isnan(x).all()) for x in dirty[1][1:5])               # its three factors and L
    assert all(same(a, b) for i, (a, b) in enumerate(zip(clean, dirty)) if i != 1)


@pytest.mark.parametrize("entry", ["apply", "update"])
def test_list_stays_inside_every_layers_extents(entry):
    """every operand of every layer between guard bands at bases skewed by 4 bytes, over a workspace of exactly the bytes asked
    for that holds NaN (fill 0xFF): the bands untouched, the frozen operands unchanged, the bits those of the aligned call"""
    shapes, gsk = [c[:3] for c in SPLIT], 48
    plain, _ = run_list(SPLIT, gram_slice_k=gsk)
    lib, plan = qtl.load(), qtl.plan_layers(shapes, gram_slice_k=gsk)
    A, B, C, group_start, raw = plan["raw"]
    k, ws_bytes = len(shapes), plan["ws_bytes"]
    floats = sum(a * a + b * b + c * c + 2 * a * b * c + 3 for a, b, c in shapes)
    arena = Arena(4 * floats + ws_bytes + raw.nbytes + 8 * qtl._ROW * k + (6 * k + 3) * (2 * DEFAULT_GUARD + 4096), 0xFF, DEV)
    keys = ("Qa", "Qb", "Qc", "L", "G", "out")
    writes = ("out",) if entry == "apply" else ("Qa", "Qb", "Qc", "L")
    t, rows = [], qtl.table_rows(shapes, plan["ws_off"])
    for i, (s, c) in enumerate(zip(shapes, SPLIT)):
        p = nc.problem(*c)
        shp = dict(Qa=(s[0],) * 2, Qb=(s[1],) * 2, Qc=(s[2],) * 2, L=(3,), G=s, out=s)
        t.append({key: arena.take(shp[key], torch.float32, align=16, skew=1, name="%s%d" % (key, i)) for key in keys})
        for key, src in dict(Qa=p["Qs"][0], Qb=p["Qs"][1], Qc=p["Qs"][2], L=p["L"], G=p["G"]).items():
            t[i][key].copy_(src)
        for key in set(keys) - set(writes) - {"out"}:
            arena.freeze("%s%d" % (key, i))
        rows[i, :6] = [t[i][key].data_ptr() for key in keys]
    ws = arena.take_bytes(ws_bytes)
    table = arena.take(rows.shape, torch.int64, align=16, name="table")
    plan_dev = arena.take((raw.size,), torch.int32, align=16, name="plan")
    table.copy_(torch.from_numpy(rows))
    plan_dev.copy_(torch.from_numpy(raw))
    arena.freeze("table")
    arena.freeze("plan")
    ints = qtl._ints
    head = (table.data_ptr(), plan_dev.data_ptr(), ints(raw), ints(group_start), len(plan["groups"]), ints(A), ints(B), ints(C), k, gsk)
    tail = (ws.data_ptr(), ws_bytes, torch.cuda.current_stream(DEV).cuda_stream)
    rc = lib.psgd_kron_qtl_apply_f32(*head, *tail) if entry == "apply" else lib.psgd_kron_qtl_update_f32(*head, qc.STEP, qc.DECAY, *tail)
    assert rc == 0
    arena.check()
    want = dict(out=0, Qa=1, Qb=2, Qc=3, L=4)
    for i in range(k):
        for key in writes:
            x = plain[i][want[key]]
            assert bool(torch.isfinite(x).all()) and torch.equal(t[i][key], x), (shapes[i], key)
