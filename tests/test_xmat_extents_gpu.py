"""Guard bands for the three compute entry points of include/psgd_xmat_hip.h (tests/test_cabi_cpu.py: no kernel without one), at
16-byte-aligned bases and bases skewed by 4 bytes.  N = 2T + 4: the 16-byte route with a quad where the runs meet."""
import pytest
import torch

import preconditioned_stochastic_gradient_descent as psgd
from psgd_tf_amd import xmat
from tests.guard_bands import DEFAULT_GUARD, Arena
from tests.xmat_cases import STEP, T, TINY32, problem

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WRITES = {"apply": ("out",), "update": ("a", "b"), "fused": ("a", "b", "out")}


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("N", [5, 1021, 2 * T + 1, 2 * T + 4])
@pytest.mark.parametrize("entry", list(WRITES))
def test_entry_point_stays_inside_its_extents(entry, N, skew):
    p, lib = problem(N), xmat.load()
    ws_bytes = lib.psgd_xmat_workspace_bytes(N)
    arena = Arena(7 * (4 * N + 2 * DEFAULT_GUARD + 4096) + ws_bytes, 0xA5, DEV)
    t = {k: arena.take(N, torch.float32, align=16, skew=skew, name=k) for k in ("a", "b", "v", "h", "g", "out")}
    ws = arena.take_bytes(ws_bytes)
    for k in t:                                                            # (out holds the pattern until it is written)
        if k != "out":
            t[k].copy_(p[k])
        if k not in WRITES[entry]:
            arena.freeze(k)
    ptr = {k: x.data_ptr() for k, x in t.items()}
    stream = torch.cuda.current_stream(DEV).cuda_stream
    plain = {k: p[k].to(DEV) for k in "abvhg"}
    if entry == "apply":
        rc = lib.psgd_xmat_apply_f32(ptr["a"], ptr["b"], ptr["g"], ptr["out"], N, stream)
        plain["out"] = psgd.precond_grad_Xmat_math(plain["a"], plain["b"], plain["g"])
    elif entry == "update":
        rc = lib.psgd_xmat_update_f32(ptr["a"], ptr["b"], ptr["v"], ptr["h"], N, STEP, TINY32, ws.data_ptr(), ws_bytes, stream)
        psgd.update_precond_Xmat_math_(plain["a"], plain["b"], plain["v"], plain["h"], STEP, TINY32)
    else:
        rc = lib.psgd_xmat_update_apply_f32(ptr["a"], ptr["b"], ptr["v"], ptr["h"], ptr["g"], ptr["out"], N, STEP, TINY32,
                                            ws.data_ptr(), ws_bytes, stream)
        plain["out"] = psgd.update_precond_grad_Xmat_math_(*[plain[k] for k in "abvhg"], STEP, TINY32)
    assert rc == 0
    arena.check()
    for k in WRITES[entry]:
        assert torch.equal(t[k], plain[k]), k
    if entry != "apply":
        assert not torch.equal(t["a"].cpu(), p["a"])                       # the state did move
