"""Guard-band harness: operands carved out of one pattern-filled arena, so that a store outside an operand's extent is seen.

torch's caching allocator rounds every allocation up to 512 bytes and aligns it to 256: a kernel that stores a few elements past
the end of a tensor, or loads a few (masked by a multiplication) from there, passes every test that hands it whole allocations.
An Arena is ONE uint8 buffer filled with a byte `fill`.  take() carves contiguous views out of it at exactly the alignment asked
for (`align` bytes plus `skew` elements -- no better, unless the caller asks), each with `guard` pattern bytes on either side;
take_bytes() carves a workspace of exactly n bytes.  The caller writes its test data into the views, freezes the read-only ones,
runs the kernel, synchronises, and calls check():

  - every byte of the arena outside the taken extents still equals `fill`;
  - every frozen operand is bit-identical to its snapshot.

A failure names the nearest tensor, the side (before / after / inside), the byte offset from that tensor's edge and the value
found.  The default guard (256 KiB) exceeds the largest tile any kernel here stages (256 rows x 64 floats = 64 KiB), so a one-tile
overrun lands in memory the test owns.  Works on any torch.device (tests/test_guard_bands_cpu.py runs it on the CPU).
"""
import numpy as np
import torch

DEFAULT_GUARD = 256 * 1024
BASE_ALIGN = 4096          # the arena's own base is rounded up to this, so `align` up to 4096 means what it says


class GuardError(AssertionError):
    pass


class _Extent:
    __slots__ = ("name", "lo", "hi", "tensor", "snapshot")

    def __init__(self, name, lo, hi, tensor):
        self.name, self.lo, self.hi, self.tensor, self.snapshot = name, lo, hi, tensor, None


class Arena:
    def __init__(self, nbytes, fill, device, guard=DEFAULT_GUARD):
        assert 0 <= int(fill) <= 255
        self.fill, self.guard, self.device = int(fill), int(guard), torch.device(device)
        raw = torch.empty(int(nbytes) + BASE_ALIGN, dtype=torch.uint8, device=self.device)
        head = (-raw.data_ptr()) % BASE_ALIGN
        self.buf = raw[head:head + int(nbytes)]
        self.buf.fill_(self.fill)
        self.base = self.buf.data_ptr()
        self._cursor = 0
        self._extents = []
        self._byname = {}

    # ---------------------------------------------------------------- carving
    def _carve(self, name, nbytes, align, skew_bytes, guard, not_better):
        guard = self.guard if guard is None else int(guard)
        assert align >= 1 and (align & (align - 1)) == 0 and align <= BASE_ALIGN, align
        lo = self._cursor + guard
        lo += (-(self.base + lo)) % align
        if not_better and align < BASE_ALIGN and (self.base + lo) % (2 * align) == 0:
            lo += align                                    # aligned to `align` and NOT to 2 * align
        lo += skew_bytes
        hi = lo + nbytes
        if hi + guard > self.buf.numel():
            raise ValueError("arena of %d bytes is too small: %r needs [%d, %d) plus a guard of %d"
                             % (self.buf.numel(), name, lo, hi, guard))
        self._cursor = hi
        return lo, hi

    def take(self, shape, dtype, align=16, skew=0, guard=None, name=None, not_better=True):
        """A contiguous view of `shape` / `dtype` whose address is `align`-aligned (and, with not_better, not 2 * align-aligned)
        plus `skew` elements, with `guard` pattern bytes before and after it.  The view holds the pattern until written."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape)) if shape else 1
        name = name or "t%d" % len(self._extents)
        assert name not in self._byname, name
        lo, hi = self._carve(name, n * item, align, skew * item, guard, not_better)
        view = self.buf[lo:hi].view(dtype).view(shape) if n else torch.empty(shape, dtype=dtype, device=self.device)
        ext = _Extent(name, lo, hi, view)
        self._extents.append(ext)
        self._byname[name] = ext
        return view

    def take_bytes(self, n, align=256, guard=None, name=None):
        """A workspace of exactly n bytes (uint8 view), `align`-aligned; its contents are the pattern."""
        return self.take((int(n),), torch.uint8, align=align, guard=guard, name=name or "ws%d" % len(self._extents), not_better=False)

    def __getitem__(self, name):
        return self._byname[name].tensor

    def extent(self, name):
        e = self._byname[name]
        return e.lo, e.hi

    # ---------------------------------------------------------------- checking
    def freeze(self, name):
        """Mark an operand read-only: check() compares it bit for bit with what it holds now."""
        e = self._byname[name]
        e.snapshot = self.buf[e.lo:e.hi].clone()

    def thaw(self, name):
        """The operand may be written again (an in-place output that was filled through a freezing helper)."""
        self._byname[name].snapshot = None

    def _nearest(self, off):
        best = None
        for e in self._extents:
            if e.lo <= off < e.hi:
                return e, "inside", off - e.lo
            for side, dist in (("before", e.lo - off), ("after", off - e.hi + 1)):
                if dist > 0 and (best is None or dist < best[3]):
                    best = (e, side, (off - e.lo) if side == "before" else (off - e.hi), dist)
        if best is None:
            return None, "in an empty arena", off
        return best[0], best[1], best[2]

    def damage(self):
        """None, or (name, side, offset, value) of the first damaged byte: side "before" (offset < 0, from the tensor's first
        byte), "after" (offset >= 0, from one past its last byte) or "inside" (a frozen operand; offset from its first byte)."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        outside = self.buf != self.fill
        for e in self._extents:
            outside[e.lo:e.hi] = False
        if bool(outside.any()):
            off = int(torch.nonzero(outside)[0, 0])
            e, side, rel = self._nearest(off)
            return (e.name if e else None, side, rel, int(self.buf[off]))
        for e in self._extents:
            if e.snapshot is not None:
                diff = self.buf[e.lo:e.hi] != e.snapshot
                if bool(diff.any()):
                    off = int(torch.nonzero(diff)[0, 0])
                    return (e.name, "inside", off, int(self.buf[e.lo + off]))
        return None

    def check(self):
        d = self.damage()
        if d is None:
            return
        name, side, rel, val = d
        if side == "inside":
            e = self._byname[name]
            raise GuardError("frozen operand %r was written: byte %d of %d now holds 0x%02X (was 0x%02X)"
                             % (name, rel, e.hi - e.lo, val, int(e.snapshot[rel])))
        where = "%d byte(s) before its first byte" % -rel if side == "before" else "%d byte(s) past its end" % rel
        raise GuardError("guard damaged %s %r: %s, byte holds 0x%02X instead of the fill 0x%02X" % (side, name, where, val, self.fill))
