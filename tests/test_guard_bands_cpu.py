"""The guard-band harness (tests/guard_bands.py) on a CPU arena: its check is not vacuous, and it places tensors where asked.

A one-byte change planted with an ordinary tensor assignment at each place a kernel can damage -- just before a tensor, just after
it, in the guard after an exactly-sized workspace, inside a frozen operand -- is reported as exactly that place; a clean arena passes.
"""
import pytest
import torch

from tests.guard_bands import Arena, GuardError

CPU = torch.device("cpu")
GUARD = 4096


def _arena(fill=0xFF):
    a = Arena(1 << 18, fill, CPU, guard=GUARD)
    U = a.take((65, 20), torch.float32, align=16, name="U")
    g = a.take((65,), torch.float32, align=16, skew=1, name="g")
    out = a.take((65,), torch.float32, align=16, skew=3, name="out")
    B = a.take((33, 8), torch.bfloat16, align=16, name="B")
    ws = a.take_bytes(1000, name="ws")
    U.copy_(torch.arange(65 * 20, dtype=torch.float32).view(65, 20))
    g.fill_(1.5)
    B.fill_(2.0)
    a.freeze("U")
    a.freeze("g")
    a.freeze("B")
    return a, U, g, out, B, ws


@pytest.mark.parametrize("fill", [0xFF, 0x3F])
def test_clean_arena_passes(fill):
    a, U, g, out, B, ws = _arena(fill)
    out.fill_(3.0)                      # outputs and workspaces may be written freely
    ws.fill_(7)
    assert a.damage() is None
    a.check()


def test_fresh_views_hold_the_pattern():
    a = Arena(1 << 16, 0xFF, CPU, guard=GUARD)
    assert torch.isnan(a.take((7,), torch.float32)).all()
    assert torch.isnan(a.take((8,), torch.bfloat16, name="b").float()).all()
    assert torch.isnan(a.take((8,), torch.float16, name="h").float()).all()
    b = Arena(1 << 16, 0x3F, CPU, guard=GUARD)
    x = b.take((7,), torch.float32)
    assert torch.isfinite(x).all() and abs(float(x[0]) - 0.747) < 1e-3


@pytest.mark.parametrize("fill", [0xFF, 0x3F])
@pytest.mark.parametrize("name", ["U", "out", "B"])
def test_a_byte_just_before_a_tensor_is_reported(fill, name):
    a = _arena(fill)[0]
    lo, _ = a.extent(name)
    a.buf[lo - 1] = 0x01
    assert a.damage() == (name, "before", -1, 0x01)
    with pytest.raises(GuardError, match="before %r: 1 byte" % name):
        a.check()


@pytest.mark.parametrize("fill", [0xFF, 0x3F])
@pytest.mark.parametrize("name", ["U", "out", "B"])
def test_a_byte_just_after_a_tensor_is_reported(fill, name):
    a = _arena(fill)[0]
    _, hi = a.extent(name)
    a.buf[hi] = 0x02
    assert a.damage() == (name, "after", 0, 0x02)
    with pytest.raises(GuardError, match="after %r: 0 byte" % name):
        a.check()


def test_damage_further_out_names_the_nearest_tensor_and_the_distance():
    a = _arena()[0]
    _, hi = a.extent("g")
    a.buf[hi + 100] = 0
    assert a.damage() == ("g", "after", 100, 0)
    lo, _ = a.extent("out")
    a.buf[hi + 100] = 0xFF
    a.buf[lo - 8] = 0
    assert a.damage() == ("out", "before", -8, 0)


def test_the_guard_after_an_exactly_sized_workspace_is_watched():
    a, U, g, out, B, ws = _arena()
    assert ws.numel() == 1000
    lo, hi = a.extent("ws")
    assert hi - lo == 1000
    ws[999] = 5
    a.check()                                  # the last byte of the workspace is the workspace's
    a.buf[hi] = 5                              # byte 1000 is not
    assert a.damage() == ("ws", "after", 0, 5)
    with pytest.raises(GuardError, match="'ws'"):
        a.check()


def test_a_change_inside_a_frozen_operand_is_reported():
    a, U, g, out, B, ws = _arena()
    U[3, 4] = -1.0                             # element 64: bytes 256 .. 259; -1.0f = 00 00 80 BF, 64.0f = 00 00 80 42
    name, side, off, val = a.damage()
    assert (name, side, off, val) == ("U", "inside", 3 * 80 + 4 * 4 + 3, 0xBF)
    with pytest.raises(GuardError, match="frozen operand 'U' was written: byte 259"):
        a.check()
    U[3, 4] = 64.0
    a.check()
    B.view(torch.int16)[5, 7] += 1             # one bit of a bf16 operand
    assert a.damage()[:3] == ("B", "inside", 2 * (5 * 8 + 7))


def test_a_frozen_operand_rewritten_with_its_own_bits_passes():
    a, U, g, out, B, ws = _arena()
    g.copy_(g.clone())
    a.check()


@pytest.mark.parametrize("dtype,item,align", [(dt, it, al) for dt, it in ((torch.float32, 4), (torch.bfloat16, 2), (torch.float64, 8))
                                              for al in (4, 16, 256) if al >= it])
@pytest.mark.parametrize("skew", [0, 1, 2, 3])
def test_addresses_are_what_was_asked_for(dtype, item, align, skew):
    a = Arena(1 << 16, 0xFF, CPU, guard=512)
    for shape in [(3,), (5, 7), (1,)]:
        t = a.take(shape, dtype, align=align, skew=skew, name="x%d" % len(shape) + str(shape[0]))
        assert t.is_contiguous() and t.shape == shape and t.dtype == dtype
        p = t.data_ptr() - skew * item
        assert p % align == 0
        assert p % (2 * align) != 0, "placed better than asked for"


def test_workspace_alignment_and_zero_sized_operands():
    a = Arena(1 << 16, 0xFF, CPU, guard=512)
    a.take((3,), torch.float32, skew=1)
    ws = a.take_bytes(40)
    assert ws.data_ptr() % 256 == 0 and ws.numel() == 40 and ws.dtype == torch.uint8
    e = a.take((0,), torch.float32, name="empty")
    assert e.numel() == 0
    a.check()


def test_an_arena_that_is_too_small_says_so():
    a = Arena(4096, 0xFF, CPU, guard=1024)
    with pytest.raises(ValueError, match="too small"):
        a.take((1024,), torch.float32)
