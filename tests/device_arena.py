"""A poisoned, guarded arena for kernel operands (a plain helper module: no fixtures, no pytest hooks).

Every operand of a call -- inputs, weights, statistics, workspace, outputs -- is a view into ONE uint8 tensor that was filled
with a byte pattern.  What a test gains over torch.empty:

  * scratch and outputs start as poison, not as the zeros of a young process: an element that is never stored, or a workspace
    word that is read before it is written, reaches the comparison with the oracle as NaN (0xFF) or as a huge stale value
    (0x7F; for counters, tickets and sums that a NaN would not upset);
  * every region has GUARD bytes of pattern before and after it, inside memory the test owns: a store past either end is found
    by check() instead of landing in an allocator's slack, and a load past either end picks up poison instead of a finite neighbour;
  * regions start at 16-byte multiples that are never 256-byte multiples: nothing can lean on an allocator's alignment;
  * sizes are exact: take_bytes(n) hands out n bytes, not n rounded up.

    0xFF   float32 / float64: NaN                        int32: -1
    0x7F   float32 3.39e38, float64 1.38e306 (finite)    int32: 2139062143
"""
import numpy as np
import torch

GUARD = 64 * 1024          # larger than any row of any shape the tests use: an overrun of up to a row stays inside the arena
PATTERNS = (0xFF, 0x7F)


class ArenaError(AssertionError):
    pass


class _Region:
    __slots__ = ("name", "begin", "end", "saved")

    def __init__(self, name, begin, end, saved):
        self.name, self.begin, self.end, self.saved = name, begin, end, saved


def _span(bad):
    """First and last index of the True entries of a 1-D bool tensor (it has at least one)."""
    idx = torch.nonzero(bad).reshape(-1)
    return int(idx[0]), int(idx[-1])


class Arena:
    def __init__(self, nbytes, pattern, device="cpu"):
        if pattern not in PATTERNS:
            raise ValueError("pattern must be 0xFF or 0x7F, got %r" % (pattern,))
        self.pattern = int(pattern)
        self.buf = torch.full((int(nbytes),), self.pattern, dtype=torch.uint8, device=device)
        self.base = self.buf.data_ptr()
        if self.base % 16:
            raise ArenaError("allocator returned a block that is not 16-byte aligned")
        self.regions = []
        self.cursor = 0                 # end of the last region (offset into buf)

    # -- carving ------------------------------------------------------------------------------------------------------------
    def _place(self, nbytes, align):
        """Offset of the next region: at least GUARD past the previous one, address a multiple of `align` (>= 16) and, unless
        the operand itself asks for 256 or more, NOT a multiple of 256."""
        if align < 16 or align & (align - 1):
            raise ValueError("align must be a power of two >= 16")
        addr = self.base + self.cursor + GUARD
        if align >= 256:
            addr = -(-addr // align) * align
        else:
            addr = -(-addr // 256) * 256
            addr += align * (1 + len(self.regions) % (256 // align - 1))      # align 16: 16, 32, .. 240 -- every residue but 0
        off = addr - self.base
        if off + nbytes + GUARD > self.buf.numel():
            raise ArenaError("arena of %d bytes is too small: region of %d bytes at %d needs %d"
                             % (self.buf.numel(), nbytes, off, off + nbytes + GUARD))
        return off

    def take(self, shape, dtype, data=None, readonly=False, name=None, align=16):
        """A contiguous `dtype` tensor of `shape` inside the arena.  `data` (numpy array or tensor) is copied in; without it the
        region keeps the pattern.  readonly=True: check() also asserts that the region still holds `data` bit for bit."""
        shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = item * int(np.prod(shape, dtype=np.int64))
        off = self._place(nbytes, align)
        view = self.buf[off:off + nbytes].view(dtype).view(shape)
        if readonly and data is None:
            raise ValueError("a read-only region needs data")
        if data is not None:
            src = torch.as_tensor(np.array(data, order="C") if isinstance(data, np.ndarray) else data)      # (a copy: cached inputs are read-only)
            if tuple(src.shape) != shape:
                raise ValueError("data has shape %s, region %s" % (tuple(src.shape), shape))
            view.copy_(src.to(dtype))
        saved = self.buf[off:off + nbytes].clone() if readonly else None
        self.regions.append(_Region(name or "region%d" % len(self.regions), off, off + nbytes, saved))
        self.cursor = off + nbytes
        return view

    def take_bytes(self, n, name=None, align=16):
        """A workspace of exactly n bytes (uint8), poisoned."""
        return self.take((int(n),), torch.uint8, name=name or "workspace%d" % len(self.regions), align=align)

    def freeze(self, view):
        """From now on the region handed out as `view` is read-only: its bytes as they stand (after the work enqueued so far)
        are snapshotted, and check() asserts that they are still there.  For state that one call produces and later calls
        take as const, such as a workspace that carries a grid.  Freezing again takes a new snapshot."""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        begin = view.data_ptr() - self.base
        for r in self.regions:
            if r.begin == begin and r.end - r.begin == view.numel() * view.element_size():
                r.saved = self.buf[r.begin:r.end].clone()
                return view
        raise ValueError("freeze() takes a whole region handed out by take() or take_bytes()")

    # -- checking -----------------------------------------------------------------------------------------------------------
    def _gaps(self):
        """(begin, end, region before or None, region after or None) of every stretch of guard bytes."""
        out, prev_end, prev = [], 0, None
        for r in self.regions:
            out.append((prev_end, r.begin, prev, r))
            prev_end, prev = r.end, r
        out.append((prev_end, self.buf.numel(), prev, None))
        return out

    def check(self):
        """Synchronises; asserts that every guard byte still holds the pattern and every read-only region its data."""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        gaps = self._gaps()
        ro = [r for r in self.regions if r.saved is not None]
        flags = [(self.buf[b:e] != self.pattern).any() for b, e, _, _ in gaps]
        flags += [(self.buf[r.begin:r.end] != r.saved).any() for r in ro]
        if not flags or not bool(torch.stack(flags).any()):
            return
        problems = []
        for (b, e, before, after), flag in zip(gaps, flags[:len(gaps)]):
            if not bool(flag):
                continue
            bad = self.buf[b:e] != self.pattern
            # a guard between two regions belongs half to each: bytes nearer the earlier region are reported as written AFTER
            # it, the others as written BEFORE the later one
            mid = e if after is None else (b if before is None else (b + e) // 2)
            if before is not None and bool(bad[:mid - b].any()):
                lo, hi = _span(bad[:mid - b])
                problems.append("guard after '%s' changed: bytes +%d .. +%d past its end" % (before.name, lo, hi))
            if after is not None and bool(bad[mid - b:].any()):
                lo, hi = _span(bad[mid - b:])
                problems.append("guard before '%s' changed: bytes -%d .. -%d before its start"
                                % (after.name, e - (mid + lo), e - (mid + hi)))
        for r, flag in zip(ro, flags[len(gaps):]):
            if bool(flag):
                lo, hi = _span(self.buf[r.begin:r.end] != r.saved)
                problems.append("read-only region '%s' changed: bytes %d .. %d of %d" % (r.name, lo, hi, r.end - r.begin))
        raise ArenaError("; ".join(problems))

    def is_pattern(self, view):
        """True when every byte of a region handed out by take() still holds the pattern (an output nobody wrote)."""
        return bool((view.contiguous().view(torch.uint8) == self.pattern).all())
