"""Guard bands around everything a fused step of class SPLU writes or reads through raw pointers: the four factors, the flat
vectors v / h / g, the output, the momentum buffer and the sparse-LU workspace are carved out of one pattern-filled arena
(tests/guard_bands.py), two steps run with every switch on, and no byte outside the extents may have changed.  Every kernel the
step reaches has its own extent test (tests/test_extents_gpu.py); this one holds the class to the sizes it passes."""
import pytest
import torch

from psgd_tf_amd import preconditioned_stochastic_gradient_descent as impl
from tests.guard_bands import Arena
from tests.test_splu_class_gpu import S65, S131, LR, LR_Q, MAX_NORM, _closure, _feed, _fresh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fit, exact", [("hessian", True), ("hessian", False), ("whitening", True)])
@pytest.mark.parametrize("shapes, r", [(S65, 4), (S131, 40)], ids=["N65-r4", "N131-r40"])
@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_two_fused_steps_stay_inside_their_buffers(monkeypatch, fill, shapes, r, fit, exact):
    import preconditioned_stochastic_gradient_descent as psgd
    from psgd_tf_amd import _lib
    dev = torch.device("cuda:0")
    _feed(monkeypatch, shapes)
    params = _fresh(shapes)
    opt = psgd.SPLU(params, r, 1.0, LR, LR_Q, MAX_NORM, 1.0, exact, generator=torch.Generator().manual_seed(2), step_tail="fused",
                    momentum=0.9, weight_decay=0.01, nonfinite="skip", loss_scale=2 ** 4, preconditioner_fit=fit, probe_seed=3)
    N = opt._out.numel()
    ws_bytes = int(_lib.load().psgd_splu_workspace_bytes(N, r))
    arena = Arena(ws_bytes + 8 * N * r * 4 + 64 * N + 16 * (256 * 1024 + 4096), fill, dev)
    # L12 16-byte aligned and no better; U12, l3, u3 aligned to their elements only (include/psgd_hip.h)
    state = {"L12": arena.take((N, r), torch.float32, name="L12"), "l3": arena.take((N - r, 1), torch.float32, skew=2, name="l3"),
             "U12": arena.take((r, N), torch.float32, skew=1, name="U12"), "u3": arena.take((N - r, 1), torch.float32, skew=3, name="u3")}
    for k, t in state.items():
        t.copy_(getattr(opt, "_" + k))
        setattr(opt, "_" + k, t)
    for k in ("v", "h", "g"):
        opt._flat_bufs[k] = arena.take((N,), torch.float32, name=k)
    opt._out = arena.take((N,), torch.float32, name="out")
    opt._m = arena.take((N,), torch.float32, name="m")
    ws = arena.take_bytes(ws_bytes, name="workspace")
    monkeypatch.setattr(impl, "_splu_workspace", lambda device, n, rank: ws)
    closure = _closure(params, shapes)
    for _ in range(2):
        opt.step(closure)
    arena.check()
    assert opt.skipped_steps == 0 and all(getattr(opt, "_" + k) is t for k, t in state.items())
    assert all(bool(torch.isfinite(t).all()) for t in list(state.values()) + [opt._out, opt._m] + [p.detach() for p in params])
