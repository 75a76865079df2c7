"""tests/device_arena.py on CPU torch: the layout it promises and the writes its check() must see."""
import numpy as np
import pytest
import torch

from tests.device_arena import GUARD, PATTERNS, Arena, ArenaError

AWKWARD = [1, 3, 4, 15, 16, 17, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 65535, 65536, 65537, 100003]


def _off(arena, view):
    return view.data_ptr() - arena.base


@pytest.mark.parametrize("pattern", PATTERNS)
def test_regions_are_16_byte_aligned_never_256_and_guarded(pattern):
    a = Arena(sum(AWKWARD) * 8 + (len(AWKWARD) + 40) * (GUARD + 512), pattern)
    views, residues = [], set()
    for k, nb in enumerate(AWKWARD):
        if k % 3 == 0:
            v = a.take_bytes(nb)
            assert v.dtype == torch.uint8 and v.numel() == nb                      # nothing rounded up
        elif k % 3 == 1:
            v = a.take((nb,), torch.float32)
        else:
            v = a.take((nb, 1), torch.float64)
        assert v.is_contiguous()
        views.append(v)
    for n in range(20):                                                            # enough regions to walk every residue
        views.append(a.take((5,), torch.int32))
    end = 0
    for v, r in zip(views, a.regions):
        addr = v.data_ptr()
        assert addr % 16 == 0 and addr % 256 != 0, addr
        residues.add(addr % 256)
        assert r.begin == _off(a, v) and r.end - r.begin == v.numel() * v.element_size()
        assert r.begin - end >= GUARD                                              # pattern before it ...
        end = r.end
    assert a.buf.numel() - end >= GUARD                                            # ... and one more band at the arena's end
    assert residues == set(range(16, 256, 16))
    a.check()
    # an operand that needs more gets it, the others keep theirs
    v = a.take((7,), torch.float32, align=64)
    assert v.data_ptr() % 64 == 0 and v.data_ptr() % 256 != 0
    v = a.take((7,), torch.float32, align=256)
    assert v.data_ptr() % 256 == 0
    a.check()


def test_patterns_read_as_the_table_says():
    a = Arena(8 * GUARD, 0xFF)
    assert torch.isnan(a.take((4,), torch.float32)).all() and torch.isnan(a.take((4,), torch.float64)).all()
    assert (a.take((4,), torch.int32) == -1).all()
    b = Arena(8 * GUARD, 0x7F)
    f, d, i = b.take((4,), torch.float32), b.take((4,), torch.float64), b.take((4,), torch.int32)
    assert torch.isfinite(f).all() and abs(float(f[0]) - 3.39e38) < 1e36
    assert torch.isfinite(d).all() and abs(float(d[0]) - 1.38e306) < 1e304
    assert (i == 2139062143).all()
    with pytest.raises(ValueError):
        Arena(4 * GUARD, 0x00)
    with pytest.raises(ArenaError):
        Arena(2 * GUARD, 0xFF).take_bytes(16)                                      # no room for both guards: refused, not shrunk


@pytest.mark.parametrize("pattern", PATTERNS)
def test_untouched_and_properly_used_arena_passes(pattern):
    a = Arena(8 * GUARD, pattern)
    x = a.take((3, 5), torch.float32, data=np.arange(15, dtype=np.float32).reshape(3, 5), readonly=True, name="x")
    y = a.take((3, 5), torch.float32, name="y")
    ws = a.take_bytes(1001, name="ws")
    assert a.is_pattern(y) and a.is_pattern(ws)
    a.check()
    y.copy_(2 * x); ws.zero_()                                                     # writes inside regions are the point
    a.check()
    assert not a.is_pattern(y)
    assert torch.equal(x, torch.arange(15, dtype=torch.float32).reshape(3, 5))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("side", ["before", "after"])
def test_a_write_one_byte_outside_a_region_is_named(pattern, side):
    a = Arena(8 * GUARD, pattern)
    a.take((10,), torch.float32, name="first")
    y = a.take((7, 3), torch.float32, name="victim")
    a.take_bytes(33, name="last")
    r = a.regions[1]
    at = r.begin - 1 if side == "before" else r.end
    a.buf[at] = 0x11
    with pytest.raises(ArenaError) as e:
        a.check()
    msg = str(e.value)
    assert ("guard %s 'victim'" % side) in msg and "first" not in msg and "last" not in msg
    assert ("-1 .. -1" if side == "before" else "+0 .. +0") in msg
    a.buf[at] = pattern
    a.check()
    # a row of floats past the end: first and last changed byte
    if side == "after":
        a.buf[r.end + 4:r.end + 16] = 0
        with pytest.raises(ArenaError, match=r"guard after 'victim' changed: bytes \+4 \.\. \+15"):
            a.check()
    else:
        a.buf[r.begin - 12:r.begin - 4] = 0
        with pytest.raises(ArenaError, match=r"guard before 'victim' changed: bytes -12 \.\. -5"):
            a.check()
    del y


def test_writes_at_the_arena_ends_are_named():
    a = Arena(6 * GUARD, 0xFF)
    a.take((4,), torch.float32, name="only")
    a.buf[0] = 0
    with pytest.raises(ArenaError, match="guard before 'only'"):
        a.check()
    a.buf[0] = 0xFF
    a.buf[-1] = 0
    with pytest.raises(ArenaError, match="guard after 'only'"):
        a.check()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_changed_read_only_region_is_named(pattern):
    a = Arena(8 * GUARD, pattern)
    w = a.take((4, 4), torch.float32, data=torch.ones(4, 4), readonly=True, name="weights")
    s = a.take((4,), torch.float64, data=np.zeros(4), name="stats")               # not read-only: may change
    s += 1.0
    a.check()
    w[2, 1] = 1.0                                                                  # same bits: still fine
    a.check()
    w[2, 1] = -1.0
    with pytest.raises(ArenaError, match=r"read-only region 'weights' changed: bytes 3[6-9] \.\. 39 of 64"):
        a.check()
    with pytest.raises(ValueError):
        a.take((2,), torch.float32, readonly=True)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_a_frozen_region_is_held_to_the_bytes_it_had_when_frozen(pattern):
    a = Arena(10 * GUARD, pattern)
    a.take((6,), torch.float32, name="before")
    ws = a.take_bytes(1001, name="grid workspace")
    out = a.take((5,), torch.int32, name="out")
    ws[:500] = 3                                                                   # the producing call writes it ...
    a.check()
    assert a.freeze(ws) is ws                                                      # ... and from here on it is const
    a.check()
    out.fill_(4)                                                                   # other regions may still change
    a.check()
    ws[17] = 3                                                                     # the same byte again: fine
    a.check()
    ws[700] = 0x11                                                                 # a byte that still held the pattern when frozen
    with pytest.raises(ArenaError, match=r"read-only region 'grid workspace' changed: bytes 700 \.\. 700 of 1001"):
        a.check()
    ws[700] = pattern
    ws[3] = 9                                                                      # a byte the producer wrote
    with pytest.raises(ArenaError, match=r"read-only region 'grid workspace' changed: bytes 3 \.\. 3 of 1001"):
        a.check()
    # a second freeze accepts the region as it now stands
    a.freeze(ws)
    a.check()
    assert not a.is_pattern(ws) and a.is_pattern(a.take((2,), torch.float32))


def test_freeze_takes_whole_regions_only():
    a = Arena(8 * GUARD, 0xFF)
    x = a.take((8,), torch.float32, name="x")
    with pytest.raises(ValueError):
        a.freeze(x[2:])                                                            # a part of a region
    with pytest.raises(ValueError):
        a.freeze(x[:4])
    with pytest.raises(ValueError):
        a.freeze(torch.zeros(8))                                                   # not the arena's memory
    ro = a.take((3,), torch.float32, data=np.ones(3, np.float32), readonly=True, name="ro")
    a.freeze(ro)                                                                   # already read-only: a new snapshot of the same bytes
    a.check()
