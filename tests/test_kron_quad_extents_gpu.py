"""Guard bands for the two compute entry points of include/psgd_kron_quad_hip.h (tests/test_kron_quad_cpu.py: no kernel without
one), at bases aligned to 16 bytes and no better and at bases skewed by 4 bytes, with a workspace of exactly the bytes asked for.
The arena's fill is the workspace's content on entry: 0xA5 and 0xFF (a NaN as float32 and as float64).  Every written operand
must hold the bits the wrapper produces from whole allocations of the same values -- the dword route of a skewed base and the
16-byte route feed the same fma chains -- so nothing outside the extents, and nothing unwritten inside the workspace, reaches a
result under either fill."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import kron_quad
from tests import kron_quad_cases as qc
from tests.guard_bands import DEFAULT_GUARD, Arena

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = qc.T
ENTRY_POINTS = {"apply": "psgd_kron_quad_apply_f32", "update": "psgd_kron_quad_update_f32"}
WRITES = {"apply": ("out",), "update": ("Ql", "Qr", "L")}
FILLS = [0xA5, 0xFF]
SHAPES = [(3, 5), (T + 1, 2 * T + 3), (T + 4, 2 * T + 4), (2 * T, T)]
_EXACT = {(M, N): seed for M, N, seed in qc.EXACT_CASES}


def _inputs(M, N):
    """(float32 Ql, Qr, L, G on the CPU, step, decay): an exact case where the shape is one, else problem()"""
    if (M, N) in _EXACT:
        p = qc.exact_problem(M, N, _EXACT[(M, N)])
        return p, p["step"], p["decay"]
    return qc.problem(M, N, 14), qc.STEP, qc.DECAY


@pytest.mark.parametrize("fill", FILLS, ids=["fillA5", "fillFF"])
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("M, N", SHAPES)
@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_entry_point_stays_inside_its_extents(entry, M, N, skew, fill):
    p, step, decay = _inputs(M, N)
    lib = kron_quad.load()
    ws_bytes = lib.psgd_kron_quad_workspace_bytes(M, N)
    shapes = dict(Ql=(M, M), Qr=(N, N), L=(2,), G=(M, N), out=(M, N))
    arena = Arena(4 * (M * M + N * N + 2 * M * N + 2) + ws_bytes + 7 * (2 * DEFAULT_GUARD + 4096), fill, DEV)
    t = {k: arena.take(s, torch.float32, align=16, skew=skew, name=k) for k, s in shapes.items()}
    ws = arena.take_bytes(ws_bytes)
    assert all((x.data_ptr() - 4 * skew) % 32 == 16 for x in t.values()) and ws.data_ptr() % 256 == 0 and ws.numel() == ws_bytes
    for k in t:                                                            # (out holds the pattern until it is written)
        if k != "out":
            t[k].copy_(p[k])
        if k not in WRITES[entry]:
            arena.freeze(k)
    ptr = {k: x.data_ptr() for k, x in t.items()}
    stream = torch.cuda.current_stream(DEV).cuda_stream
    plain = {k: p[k].to(DEV).clone() for k in ("Ql", "Qr", "L", "G")}
    if entry == "apply":
        rc = lib.psgd_kron_quad_apply_f32(ptr["Ql"], ptr["Qr"], ptr["G"], ptr["out"], M, N, ws.data_ptr(), ws_bytes, stream)
        plain["out"] = psgd.precond_grad_kron_quad(plain["Ql"], plain["Qr"], plain["G"])
    else:
        rc = lib.psgd_kron_quad_update_f32(ptr["Ql"], ptr["Qr"], ptr["L"], ptr["G"], M, N, step, decay, ws.data_ptr(), ws_bytes, stream)
        psgd.update_precond_kron_quad_(plain["Ql"], plain["Qr"], plain["L"], plain["G"], step, decay)
    assert rc == 0
    arena.check()
    for k in WRITES[entry]:
        assert bool(torch.isfinite(plain[k]).all()) and torch.equal(t[k], plain[k]), k
    if entry == "update":
        assert not torch.equal(t["Ql"].cpu(), p["Ql"]) and not torch.equal(t["Qr"].cpu(), p["Qr"])   # the state did move
        if (M, N) in _EXACT:
            assert torch.equal(t["Ql"].double().cpu(), p["new_Ql"]) and torch.equal(t["Qr"].double().cpu(), p["new_Qr"])
    elif (M, N) in _EXACT:
        assert torch.equal(t["out"].double().cpu(), p["out"])
