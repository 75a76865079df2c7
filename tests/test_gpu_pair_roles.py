"""The Winograd pair kernel (mvsnet_amd/csrc/conv3d_c8_wino.hip) as eight waves in two roles, two waves per SIMD.

Waves 0-3 carry 3dconv0_1 (the Winograd sweep and retire()), waves 4-7 carry 3dconv1_0 (the stride-2 sweep, its park and finish); all
eight stage the planes.  No arithmetic moves: every accumulator receives the same products in the same order as in the four-wave
kernel, which stays reachable through the hook MVS_HOOK_PAIR_WAVES4 (`pair_waves4=1`).  So

  1. outputs are the four-wave kernel's bits; on integer data the float64 sums too, on random data to sums_equal's rule (the same
     float32 partials, the float64 atomics in any order);
  2. the new default is exact on integers against the float64 oracle;
  3. a voxel's bits do not depend on the schedule, with either kernel;
  4. both run inside the poisoned, guarded arena;
  5. the launcher refuses what it refused: odd sizes, with the outputs untouched.
"""
import functools

import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L

from tests.device_arena import PATTERNS, Arena
from tests.test_gpu_halo_planes import pair_case, run_pair, sums_equal
from tests.test_gpu_pair_winograd import check_oracle, integer_case

pytestmark = pytest.mark.gpu

DEV = "cuda"
W4 = {"pair_waves4": 1}


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


# (2, 2, 2): every tap is padding somewhere; (4, 8, 16): half a tile; (6, 10, 34): the second tile column holds one pair, partial
# row tile; (6, 8, 66): three tile columns; (12, 16, 64): two tile rows
SHAPES = [(2, 2, 2), (4, 8, 16), (6, 10, 34), (6, 8, 66), (12, 16, 64)]


# ---- 1. same bits as the four-wave kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_roles_give_the_four_wave_bits_on_random_data(shape):
    x, w1, w2, _, _ = pair_case(*shape)
    y1, y2, s1, s2 = run_pair(x, w1, w2, {})
    f1, f2, fs1, fs2 = run_pair(x, w1, w2, W4)
    print("random %s: bit-equal %s %s, max rel sum difference %.3g %.3g"
          % (shape, np.array_equal(y1, f1), np.array_equal(y2, f2), np.abs(s1 / fs1 - 1).max(), np.abs(s2 / fs2 - 1).max()))
    assert np.abs(y1).max() > 0 and np.abs(y2).max() > 0
    assert np.array_equal(y1, f1) and np.array_equal(y2, f2)
    sums_equal(s1, fs1, y1)
    sums_equal(s2, fs2, y2)


@pytest.mark.parametrize("shape", SHAPES)
def test_roles_give_the_four_wave_bits_on_integers(shape):
    x, w1, w2, _, _ = integer_case(*shape)
    y1, y2, s1, s2 = run_pair(x, w1, w2, {})
    f1, f2, fs1, fs2 = run_pair(x, w1, w2, W4)
    assert np.abs(y1).max() > 0 and np.abs(y2).max() > 0
    assert np.array_equal(y1, f1) and np.array_equal(y2, f2)
    assert np.array_equal(s1, fs1) and np.array_equal(s2, fs2)


# ---- 2. exact on integers against the float64 oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[:4])
def test_roles_are_exact_on_integers(shape):
    x, w1, w2, e1, e2 = integer_case(*shape)
    assert L.load().mvs_get_test_hook(L.HOOKS["pair_waves4"]) == 0
    y1, y2, s1, s2 = run_pair(x, w1, w2, {})
    print("integers %s: max |y1 - e1| %g, max |y2 - e2| %g" % (shape, np.abs(y1 - e1).max(), np.abs(y2 - e2).max()))
    assert np.array_equal(y1, e1) and np.array_equal(y2, e2)
    for st, e, c in ((s1, e1, 8), (s2, e2, 16)):
        assert np.array_equal(st[0], e.reshape(-1, c).sum(0))
        assert np.array_equal(st[1], (e.reshape(-1, c) ** 2).sum(0))


# ---- 3. schedule independence ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def default_run(D, H, W):
    x, w1, w2, _, _ = pair_case(D, H, W)
    return run_pair(x, w1, w2, {})


def check_schedule(D, H, W, hooks, waves4):
    """`hooks` (with pair_waves4 = 1 if waves4) against the new default's own default run and against its full-sweep twins."""
    x, w1, w2, e1, e2 = pair_case(D, H, W)
    r1, r2, _, _ = default_run(D, H, W)
    mine = dict(hooks, **W4) if waves4 else hooks
    y1, y2, s1, s2 = run_pair(x, w1, w2, mine)
    f1, f2, fs1, fs2 = run_pair(x, w1, w2, dict(mine, conv_full_sweeps=5))
    g1, g2, gs1, gs2 = run_pair(x, w1, w2, dict(mine, conv_full_sweeps=10))
    print("schedule %s %s: max |y1 - e1| %.3g, bit-equal to the default %s %s, to full sweeps %s %s / %s %s"
          % ((D, H, W), mine, np.abs(y1 - e1).max(), np.array_equal(y1, r1), np.array_equal(y2, r2), np.array_equal(y1, f1),
             np.array_equal(y2, f2), np.array_equal(y1, g1), np.array_equal(y2, g2)))
    check_oracle(y1, y2, s1, s2, e1, e2)
    assert np.array_equal(y1, r1) and np.array_equal(y2, r2)
    for o1, o2, os1, os2 in ((f1, f2, fs1, fs2), (g1, g2, gs1, gs2)):
        assert np.array_equal(y1, o1) and np.array_equal(y2, o2)
        sums_equal(s1, os1, y1)
        sums_equal(s2, os2, y2)
    if waves4:
        # the same schedule with the roles: the same partials
        d1, d2, ds1, ds2 = run_pair(x, w1, w2, hooks)
        assert np.array_equal(y1, d1) and np.array_equal(y2, d2)
        sums_equal(s1, ds1, y1)
        sums_equal(s2, ds2, y2)


@pytest.mark.parametrize("waves4", [0, 1])
@pytest.mark.parametrize("no_span", [0, 1])
@pytest.mark.parametrize("planes", [2, 4, 6])
@pytest.mark.parametrize("hw", [(8, 32), (10, 40)])
def test_roles_chunks(hw, planes, no_span, waves4):
    check_schedule(12, hw[0], hw[1], {"pair_planes": planes, "conv_no_span": no_span}, waves4)


# two 32-wide tiles in one group; the crossing range's segments have (T - 1) % 3 = 2, 1, 0
@pytest.mark.parametrize("waves4", [0, 1])
@pytest.mark.parametrize("depth,g,m", [(48, 2, 3), (36, 2, 3), (40, 2, 5)])
def test_roles_span_crossing(depth, g, m, waves4):
    check_schedule(depth, 8, 64, {"span_force": g << 8 | m}, waves4)


# ---- 4. inside the guarded arena ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves4", [0, 1])
@pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
@pytest.mark.parametrize("shape", [(8, 8, 16), (6, 10, 34)])
def test_roles_in_the_arena(shape, pattern, waves4):
    D, H, W = shape
    x, w1, w2, e1, e2 = pair_case(D, H, W)
    a = Arena(8 << 20, pattern, DEV)
    F32, F64 = torch.float32, torch.float64
    dx = a.take(x.shape, F32, data=x, readonly=True, name="x")
    dw1 = a.take(w1.shape, F32, data=w1, readonly=True, name="w1")
    dw2 = a.take(w2.shape, F32, data=w2, readonly=True, name="w2")
    s1, s2 = a.take((2, 8), F64, name="stats1"), a.take((2, 16), F64, name="stats2")
    for s in (s1, s2):
        L.check(L.load().mvs_zero_f64(L.ptr(s), s.numel(), L.stream_ptr()), "mvs_zero_f64")
    y1, y2 = a.take((D, H, W, 8), F32, name="y1"), a.take((D // 2, H // 2, W // 2, 16), F32, name="y2")
    with L.test_hooks(pair_waves4=waves4):
        L.check(L.load().mvs_conv3d_pair_f32(L.ptr(dx), L.ptr(dw1), L.ptr(dw2), D, H, W, 32, 8, 16, L.ptr(y1), L.ptr(s1),
                                             L.ptr(y2), L.ptr(s2), L.stream_ptr()), "mvs_conv3d_pair_f32")
        torch.cuda.synchronize()
    a.check()
    check_oracle(n(y1), n(y2), n(s1), n(s2), e1, e2)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
# (The launcher also answers MVS_E_SHAPE to an input with a producer BatchNorm.  No entry of the C ABI reaches that: the dispatcher
# in conv3d_c8.hip sends such launches to the direct kernel before it asks this one, and mvs_conv3d_pair_f32 takes plain inputs.)
E_SHAPE = -2      # MVS_E_SHAPE


@pytest.mark.parametrize("waves4", [0, 1])
@pytest.mark.parametrize("shape", [(3, 8, 16), (4, 7, 16), (4, 8, 15)], ids=["odd-D", "odd-H", "odd-W"])
def test_roles_launcher_refuses_odd_sizes(shape, waves4):
    D, H, W = shape
    lib = L.load()
    x = torch.zeros((D, H, W, 32), device=DEV)
    w1, w2 = torch.zeros((3, 3, 3, 32, 8), device=DEV), torch.zeros((3, 3, 3, 32, 16), device=DEV)
    y1 = torch.full((D, H, W, 8), 7.0, device=DEV)
    y2 = torch.full(((D + 1) // 2, (H + 1) // 2, (W + 1) // 2, 16), 7.0, device=DEV)
    with L.test_hooks(pair_waves4=waves4):
        rc = lib.mvs_conv3d_pair_f32(L.ptr(x), L.ptr(w1), L.ptr(w2), D, H, W, 32, 8, 16, L.ptr(y1), None, L.ptr(y2), None,
                                     L.stream_ptr())
    assert rc == E_SHAPE
    assert float(n(y1).min()) == 7.0 == float(n(y1).max()) and float(n(y2).min()) == 7.0 == float(n(y2).max())
