"""The fused 3dconv0_1 + 1_0 launch with 3dconv0_1 as Winograd F(2,3) along w (mvsnet_amd/csrc/conv3d_c8_wino.hip).

Everything goes through mvsnet_amd.model.conv3d_pair with float64 sum buffers, as test_gpu_halo_planes.run_pair does.  The direct
kernel (conv3d_c8.hip) stays reachable through the hook MVS_HOOK_PAIR_DIRECT (`pair_direct=1`).

  1. integers: every product and sum is exact in float32 (x in [-3, 3], w1 EVEN in [-4, 4] so that the transformed weights
     (w0 +- w1 + w2) / 2 are integers, w2 in [-2, 2]), so outputs and float64 sums equal the float64 oracle exactly and the direct
     kernel bit for bit.  The float32 partial sums of squares stay integers below 2^24 at these sizes: the launcher cuts D <= 6 into
     chunks of 2 planes, a wave then holds 2 x 2 x 32 voxels x 8 channels = 4 values per lane and channel, 128 after its fold over
     32 lanes, of E[y1^2] = 27 * 32 * 4 * 8 = 27 648 each: 3.5e6 +- 0.5e6 against 1.7e7 (the waves are added in float64).
  2. random data against the float64 oracle at the launch's existing tolerances.
  3. a voxel's bits do not depend on the range, chunk or segment that computed it, nor on the halo-plane trimming.
  4. the pre-laid-out weights and the in-kernel transform give the same bits; the regulariser agrees between the two kernels.
  5. both kernels' operands inside the poisoned, guarded arena (tests/device_arena.py), at the W = 34 edge too.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S
from mvsnet_amd import _lib as L

from tests.device_arena import PATTERNS, Arena
from tests.test_gpu_halo_planes import pair_case, run_pair, sums_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(DEV)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def check_oracle(y1, y2, s1, s2, e1, e2):
    """The bounds test_gpu_halo_planes.check_pair holds this launch to."""
    np.testing.assert_allclose(y1, e1, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(y2, e2, rtol=1e-4, atol=2e-5)
    for st, e, c in ((s1, e1, 8), (s2, e2, 16)):
        np.testing.assert_allclose(st[0], e.reshape(-1, c).sum(0), rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(st[1], (e.reshape(-1, c) ** 2).sum(0), rtol=1e-4, atol=1e-3)


# ---- 1. exact on integers ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def integer_case(D, H, W):
    rs = np.random.RandomState(7 + D * 1000 + H * 10 + W)
    x = rs.randint(-3, 4, (D, H, W, 32)).astype(np.float32)
    w1 = (2 * rs.randint(-2, 3, (3, 3, 3, 32, 8))).astype(np.float32)
    w2 = rs.randint(-2, 3, (3, 3, 3, 32, 16)).astype(np.float32)
    e1 = O.conv3d_same(x, w1, 1, np.float64)
    e2 = O.conv3d_same(x, w2, 2, np.float64)
    for a in (x, w1, w2, e1, e2):
        a.setflags(write=False)
    return x, w1, w2, e1, e2


# (2, 2, 2): every tap is padding somewhere; (4, 8, 16): half a tile; (6, 10, 34): the second tile column holds one pair, partial
# row tile; (6, 8, 66): three tile columns
@pytest.mark.parametrize("shape", [(2, 2, 2), (4, 8, 16), (6, 10, 34), (6, 8, 66)])
def test_pair_winograd_is_exact_on_integers(shape):
    x, w1, w2, e1, e2 = integer_case(*shape)
    y1, y2, s1, s2 = run_pair(x, w1, w2, {})
    d1, d2, ds1, ds2 = run_pair(x, w1, w2, {"pair_direct": 1})
    print("integers %s: max |y1 - e1| %g, max |y2 - e2| %g, against the direct kernel %g %g; max |y1| %g"
          % (shape, np.abs(y1 - e1).max(), np.abs(y2 - e2).max(), np.abs(y1 - d1).max(), np.abs(y2 - d2).max(), np.abs(e1).max()))
    assert np.array_equal(y1, e1) and np.array_equal(y2, e2)
    for st, e, c in ((s1, e1, 8), (s2, e2, 16)):
        assert np.array_equal(st[0], e.reshape(-1, c).sum(0))
        assert np.array_equal(st[1], (e.reshape(-1, c) ** 2).sum(0))
    assert np.array_equal(y1, d1) and np.array_equal(y2, d2)
    assert np.array_equal(s1, ds1) and np.array_equal(s2, ds2)


# ---- 2. random data against the float64 oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8, 16), (6, 10, 34), (12, 16, 64)])
def test_pair_winograd_matches_oracle(shape):
    x, w1, w2, e1, e2 = pair_case(*shape)
    y1, y2, s1, s2 = run_pair(x, w1, w2, {})
    print("random %s: max |y1 - e1| %.3g (mean %.3g), max |y2 - e2| %.3g"
          % (shape, np.abs(y1 - e1).max(), np.abs(y1 - e1).mean(), np.abs(y2 - e2).max()))
    check_oracle(y1, y2, s1, s2, e1, e2)


# ---- 3. schedule independence ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def default_run(D, H, W):
    x, w1, w2, _, _ = pair_case(D, H, W)
    return run_pair(x, w1, w2, {})


def check_schedule(D, H, W, hooks):
    x, w1, w2, e1, e2 = pair_case(D, H, W)
    r1, r2, _, _ = default_run(D, H, W)
    y1, y2, s1, s2 = run_pair(x, w1, w2, hooks)
    f1, f2, fs1, fs2 = run_pair(x, w1, w2, dict(hooks, conv_full_sweeps=5))
    g1, g2, gs1, gs2 = run_pair(x, w1, w2, dict(hooks, conv_full_sweeps=10))
    print("schedule %s %s: max |y1 - e1| %.3g, bit-equal to the default %s %s, to full sweeps %s %s / %s %s"
          % ((D, H, W), hooks, np.abs(y1 - e1).max(), np.array_equal(y1, r1), np.array_equal(y2, r2), np.array_equal(y1, f1),
             np.array_equal(y2, f2), np.array_equal(y1, g1), np.array_equal(y2, g2)))
    check_oracle(y1, y2, s1, s2, e1, e2)
    # another range length cuts the float32 partial sums elsewhere: against the default schedule the sums are held to the oracle
    # above, and only the full-sweep twins of the SAME schedule add the same partials (sums_equal's rule)
    assert np.array_equal(y1, r1) and np.array_equal(y2, r2)
    for o1, o2, os1, os2 in ((f1, f2, fs1, fs2), (g1, g2, gs1, gs2)):
        assert np.array_equal(y1, o1) and np.array_equal(y2, o2)
        sums_equal(s1, os1, y1)
        sums_equal(s2, os2, y2)


@pytest.mark.parametrize("no_span", [0, 1])
@pytest.mark.parametrize("planes", [2, 4, 6])
@pytest.mark.parametrize("hw", [(8, 32), (10, 40)])
def test_pair_winograd_chunks(hw, planes, no_span):
    check_schedule(12, hw[0], hw[1], {"pair_planes": planes, "conv_no_span": no_span})


# two 32-wide tiles in one group; the crossing range's segments have (T - 1) % 3 = 2, 1, 0 (test_pair_span_crossing_at_small_size)
@pytest.mark.parametrize("depth,g,m", [(48, 2, 3), (36, 2, 3), (40, 2, 5)])
def test_pair_winograd_span_crossing(depth, g, m):
    check_schedule(depth, 8, 64, {"span_force": g << 8 | m})


# ---- 4. weight paths and the regulariser --------------------------------------------------------------------------------------
def test_pair_winograd_prepared_weights_give_the_same_bits():
    """The regulariser's prepared entry hands the kernel 3dconv0_1's transformed weights pre-laid-out; conv3d_pair makes the kernel
    transform them itself.  Both raw outputs are read back from the regulariser's workspace, whose first regions are the raw
    outputs of 3dconv1_0, 2_0, 3_0 and 0_1 in that order, each rounded up to 256 bytes (regnet.hip: carve)."""
    from mvsnet_amd.model import RegNetWeights, regnet_us0
    D, H, W = 8, 8, 16
    params = S.make_regnet_params("normal", seed=61, random_affine=True)
    wts = RegNetWeights(params, DEV)
    assert wts.base == 8 and wts.cin == 32
    cost = t(np.abs(np.random.RandomState(62).standard_normal((D, H, W, 32))).astype(np.float32))
    ws = torch.empty(L.load().mvs_regnet_workspace_bytes(D, H, W, 32, wts.base), device=DEV, dtype=torch.uint8)
    regnet_us0(cost, wts, workspace=ws)
    v0 = D * H * W
    sizes = [(v0 >> (3 * lvl)) * co * 4 for lvl, co in ((1, 16), (2, 32), (3, 64), (0, 8))]
    assert all(s % 256 == 0 for s in sizes)
    off10, off01 = 0, sum(sizes[:3])
    got10 = n(ws[off10:off10 + sizes[0]].view(torch.float32).view(D // 2, H // 2, W // 2, 16))
    got01 = n(ws[off01:off01 + sizes[3]].view(torch.float32).view(D, H, W, 8))
    y1, y2 = n_pair(cost, wts.w[3], wts.w[0])
    assert np.isfinite(got01).all() and np.abs(got01).max() > 0
    assert np.array_equal(got01, y1) and np.array_equal(got10, y2)


def n_pair(x, w1, w2):
    from mvsnet_amd.model import conv3d_pair
    y1, y2 = conv3d_pair(x, w1, w2)
    return n(y1), n(y2)


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 32, 64)])
@pytest.mark.parametrize("entry", ["prepared", "plain"])
def test_regnet_agrees_between_the_pair_kernels(entry, shape):
    """The two entries test_regnet_routes_are_the_recorded_ones drives, default against pair_direct = 1, at the bound
    test_regnet_span_and_fused_pair_equal_the_plain_schedules holds between routes."""
    from mvsnet_amd.model import BN_EPSILON, RegNetWeights, regnet_us0
    lib = L.load()
    D, H, W = shape
    params = S.make_regnet_params("normal", seed=41, random_affine=True)
    wts = RegNetWeights(params, DEV)
    cost = t(np.abs(np.random.RandomState(42).standard_normal((D, H, W, 32))).astype(np.float32))

    def run():
        if entry == "prepared":
            return n(regnet_us0(cost, wts))
        reg = torch.empty((D, H, W), device=DEV, dtype=torch.float32)
        ws = torch.empty(lib.mvs_regnet_workspace_bytes(D, H, W, 32, wts.base), device=DEV, dtype=torch.uint8)
        L.check(lib.mvs_regnet_us0_f32(L.ptr(cost), D, H, W, 32, wts.base, wts.w_ptrs, wts.g_ptrs, wts.b_ptrs, BN_EPSILON,
                                       C.c_void_p(ws.data_ptr()), ws.numel(), L.ptr(reg), L.stream_ptr()), "mvs_regnet_us0_f32")
        return n(reg)

    wino = run()
    with L.test_hooks(pair_direct=1):
        direct = run()
    scale = float(np.abs(direct).max())
    print("regnet %s %s: max |winograd - direct| %.3g = %.3g of max |y|" % (entry, shape, np.abs(wino - direct).max(),
                                                                          np.abs(wino - direct).max() / scale))
    assert np.isfinite(wino).all()
    assert float(np.abs(wino - direct).max()) <= 2e-5 * scale


# ---- 5. inside the guarded arena ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
@pytest.mark.parametrize("shape", [(8, 8, 16), (6, 10, 34)])
def test_pair_winograd_in_the_arena(shape, pattern):
    """No read of poison and no write outside y1, y2 and the sums -- at W = 34 a pair's second column and the 34th staged column of
    the second tile column fall outside the volume."""
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
    L.check(L.load().mvs_conv3d_pair_f32(L.ptr(dx), L.ptr(dw1), L.ptr(dw2), D, H, W, 32, 8, 16, L.ptr(y1), L.ptr(s1), L.ptr(y2),
                                         L.ptr(s2), L.stream_ptr()), "mvs_conv3d_pair_f32")
    torch.cuda.synchronize()
    a.check()
    check_oracle(n(y1), n(y2), n(s1), n(s2), e1, e2)
