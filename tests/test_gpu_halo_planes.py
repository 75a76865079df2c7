"""Halo planes of the stride-1 plane-march kernels (conv3d_c8.hip, conv3d_mfma.hip).

A workgroup's range [d0, d1) stages the input planes d0 - 1 .. d1.  The first and the last of them feed one output plane each, so
they issue only the MFMA tiles whose result is kept (one variant of the last plane per (T - 1) % 3, T = d1 - d0 + 2), and planes
outside the volume issue none.  Every case is held (i) to the float64 oracle at the bounds tests/test_gpu_parity.py uses for the
same layer kinds, and (ii) to the same call with MVS_HOOK_CONV_FULL_SWEEPS = 5 (every staged plane swept in full, in both kernel
families; and = 10: all but the planes outside the volume): the outputs with np.array_equal -- the trimmed MFMAs only ever added to accumulators that are dropped, or added products of staged zeros --
and the float64 BatchNorm sums to 1e-12: the workgroups' float32 partial sums are the same bits, their float64 atomics arrive in
any order, which moves a sum by at most (workgroups x 2.2e-16) of the sum of the partials' magnitudes.

Range lengths are forced through MVS_HOOK_PAIR_PLANES / MVS_HOOK_S1_PLANES / MVS_HOOK_FUSE2_PLANES and the SPAN schedule with a
tile-boundary crossing through MVS_HOOK_SPAN_FORCE, so that small volumes reach interior first / last planes in each variant."""
import functools

import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S
from mvsnet_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(DEV)      # (a copy: the cached inputs are read-only)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / np.abs(b).sum())


def sums_equal(got, ref, y):
    """float64 BatchNorm sums of two schedules that add the same float32 partials in another order."""
    c = y.shape[-1]
    flat = np.abs(y.reshape(-1, c).astype(np.float64))
    np.testing.assert_allclose(got[0], ref[0], rtol=1e-12, atol=1e-12 * flat.sum(0).max())
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-12, atol=0)


# ---- the fused pair (conv3d_c8_kernel<true, false, SPAN>) ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_case(D, H, W):
    rs = np.random.RandomState(D * 1000 + H * 10 + W)
    x = rs.standard_normal((D, H, W, 32)).astype(np.float32)
    w1 = (rs.standard_normal((3, 3, 3, 32, 8)) / np.sqrt(27 * 32)).astype(np.float32)
    w2 = (rs.standard_normal((3, 3, 3, 32, 16)) / np.sqrt(27 * 32)).astype(np.float32)
    e1 = O.conv3d_same(x, w1, 1, np.float64)
    e2 = O.conv3d_same(x, w2, 2, np.float64)
    for a in (x, w1, w2, e1, e2):
        a.setflags(write=False)
    return x, w1, w2, e1, e2


def run_pair(x, w1, w2, hooks):
    from mvsnet_amd.model import conv3d_pair
    s1 = torch.zeros((2, 8), dtype=torch.float64, device=DEV)
    s2 = torch.zeros((2, 16), dtype=torch.float64, device=DEV)
    with L.test_hooks(**hooks):
        y1, y2 = conv3d_pair(t(x), t(w1), t(w2), s1, s2)
        return n(y1), n(y2), n(s1), n(s2)


def check_pair(D, H, W, hooks):
    x, w1, w2, e1, e2 = pair_case(D, H, W)
    y1, y2, s1, s2 = run_pair(x, w1, w2, hooks)
    f1, f2, fs1, fs2 = run_pair(x, w1, w2, dict(hooks, conv_full_sweeps=5))
    g1, g2, _, _ = run_pair(x, w1, w2, dict(hooks, conv_full_sweeps=10))
    print("pair %s %s: max |y1 - e1| %.3g, max |y2 - e2| %.3g, bit-equal %s %s"
          % ((D, H, W), hooks, np.abs(y1 - e1).max(), np.abs(y2 - e2).max(), np.array_equal(y1, f1), np.array_equal(y2, f2)))
    np.testing.assert_allclose(y1, e1, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(y2, e2, rtol=1e-4, atol=2e-5)
    for st, e, c in ((s1, e1, 8), (s2, e2, 16)):
        np.testing.assert_allclose(st[0], e.reshape(-1, c).sum(0), rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(st[1], (e.reshape(-1, c) ** 2).sum(0), rtol=1e-4, atol=1e-3)
    assert np.array_equal(y1, f1) and np.array_equal(y2, f2)
    assert np.array_equal(y1, g1) and np.array_equal(y2, g2)
    sums_equal(s1, fs1, y1)
    sums_equal(s2, fs2, y2)


# D = 2, 4, 6 as one chunk: both halo planes are padding, T = 4, 6, 8 takes each variant of the last plane ((T - 1) % 3 = 0, 2, 1);
# D = 12 in chunks of 2, 4, 6: first and last planes inside the volume in each variant, and the stride-2 part's kd = 2 half
@pytest.mark.parametrize("no_span", [0, 1])
@pytest.mark.parametrize("depth,planes", [(2, 2), (4, 4), (6, 6), (12, 2), (12, 4), (12, 6)])
@pytest.mark.parametrize("hw", [(8, 16), (10, 40)])
def test_pair_halo_planes(hw, depth, planes, no_span):
    check_pair(depth, hw[0], hw[1], {"pair_planes": planes, "conv_no_span": no_span})


# two tiles in one group: D = 48, M = 3 -> [0, 32), [32, 64) across plane 48, [64, 96): both segments of the crossing range have
# (T - 1) % 3 = 2; D = 36, M = 3 -> ranges of 24, segments of 12: 1; D = 40, M = 5 -> ranges of 16, segments of 8: 0
@pytest.mark.parametrize("depth,g,m", [(48, 2, 3), (36, 2, 3), (40, 2, 5)])
def test_pair_span_crossing_at_small_size(depth, g, m):
    check_pair(depth, 8, 32, {"span_force": g << 8 | m})


# ---- conv3d_s1_kernel and the unfused 32 -> 8 kernel through model.conv3d ----------------------------------------------------
S1_SHAPES = [(7, 8, 16, 16, 16), (9, 10, 20, 16, 16), (7, 8, 16, 32, 8), (9, 10, 20, 32, 8),
             (5, 12, 40, 32, 16), (4, 16, 20, 64, 64)]      # D, H, W, Cin, Cout; the last two: 2x8 / 4x4 column tiles


@functools.lru_cache(maxsize=None)
def s1_case(case):
    D, H, W, Cin, Cout = case
    rs = np.random.RandomState(sum(case))
    x = rs.standard_normal((D, H, W, Cin)).astype(np.float32)
    x2 = rs.standard_normal((D, H, W, Cin)).astype(np.float32)
    wgt = (rs.standard_normal((3, 3, 3, Cin, Cout)) / np.sqrt(27 * Cin)).astype(np.float32)
    sc = (1 + 0.3 * rs.standard_normal(Cin)).astype(np.float32); sh = (0.2 * rs.standard_normal(Cin)).astype(np.float32)
    sc2 = (1 + 0.3 * rs.standard_normal(Cin)).astype(np.float32); sh2 = (0.2 * rs.standard_normal(Cin)).astype(np.float32)
    e_plain = O.conv3d_same(x, wgt, 1, np.float64)
    xin = np.maximum(x * sc + sh, 0).astype(np.float64) + np.maximum(x2 * sc2 + sh2, 0)
    e_fused = O.conv3d_same(xin, wgt, 1, np.float64)
    out = (x, x2, wgt, sc, sh, sc2, sh2, e_plain, e_fused)
    for a in out:
        a.setflags(write=False)
    return out


def run_s1(case, hooks):
    from mvsnet_amd.model import conv3d
    x, x2, wgt, sc, sh, sc2, sh2, _, _ = s1_case(case)
    stats = torch.zeros((2, case[4]), dtype=torch.float64, device=DEV)
    with L.test_hooks(**hooks):
        y_plain = n(conv3d(t(x), t(wgt), 1))
        y_fused = n(conv3d(t(x), t(wgt), 1, (t(sc), t(sh)), t(x2), (t(sc2), t(sh2)), stats))
        return y_plain, y_fused, n(stats)


@pytest.mark.parametrize("planes", [1, 2, 3, 4])
@pytest.mark.parametrize("case", S1_SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d_s1_halo_planes(case, planes):
    Cout = case[4]
    e_plain, e_fused = s1_case(case)[7:]
    y_plain, y_fused, st = run_s1(case, {"s1_planes": planes})
    f_plain, f_fused, fst = run_s1(case, {"s1_planes": planes, "conv_full_sweeps": 5})
    g_plain, g_fused, _ = run_s1(case, {"s1_planes": planes, "conv_full_sweeps": 10})
    print("s1 %s planes %d: max err %.3g / %.3g, bit-equal %s %s" % (case, planes, np.abs(y_plain - e_plain).max(),
          np.abs(y_fused - e_fused).max(), np.array_equal(y_plain, f_plain), np.array_equal(y_fused, f_fused)))
    np.testing.assert_allclose(y_plain, e_plain, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(y_fused, e_fused, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(st[0], e_fused.reshape(-1, Cout).sum(0), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(st[1], (e_fused.reshape(-1, Cout) ** 2).sum(0), rtol=1e-4, atol=1e-3)
    assert np.array_equal(y_plain, f_plain) and np.array_equal(y_fused, f_fused)
    assert np.array_equal(y_plain, g_plain) and np.array_equal(y_fused, g_fused)
    sums_equal(st, fst, y_fused)


# ---- the fused 3dconv1_1 + 2_0 launch (FUSE2) through the regulariser ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def regnet_case():
    params = S.make_regnet_params("normal", seed=51, random_affine=True)
    cost = np.abs(np.random.RandomState(52).standard_normal((16, 16, 32, 32))).astype(np.float32)
    exp = O.regnet_us0(cost, params, np.float64)
    cost.setflags(write=False); exp.setflags(write=False)
    return params, cost, exp


@pytest.mark.parametrize("planes", [2, 4, 6])
def test_fuse2_halo_planes_in_regnet(planes):
    """The half-resolution level is (8, 8, 16): chunks of 2, 4 and 6 planes give T = 4, 6, 8 and a short last chunk.  The whole
    regulariser is bit-equal with full sweeps as long as the float64 sums round to the same float32 (scale, shift), which they
    do unless a sum sits within 1e-16 of a rounding boundary."""
    from mvsnet_amd.model import RegNetWeights, regnet_us0
    params, cost, exp = regnet_case()
    wts = RegNetWeights(params, DEV)
    with L.test_hooks(fuse2_planes=planes):
        got = n(regnet_us0(t(cost), wts))
    with L.test_hooks(fuse2_planes=planes, conv_full_sweeps=5):
        full = n(regnet_us0(t(cost), wts))
    with L.test_hooks(conv_no_fuse2=1):
        apart = n(regnet_us0(t(cost), wts))
    print("fuse2 planes %d: rel_l1 to oracle %.3g, to the layers apart %.3g, bit-equal to full sweeps %s"
          % (planes, rel_l1(got, exp), rel_l1(got, apart), np.array_equal(got, full)))
    for ref in (exp, apart):
        assert rel_l1(got, ref) < 2e-5
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=2e-4)
    assert np.array_equal(got, full)
