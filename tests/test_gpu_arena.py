"""Every hot-path entry point with ALL of its operands inside one poisoned, guarded device arena (tests/device_arena.py).

The comparisons are the ones the oracle tests of the same entry points make (same float64 oracle call, same tolerances, taken
from test_gpu_parity.py, test_gpu_halo_planes.py, test_gpu_sweep_every_pixel.py and sweep_reference.check_every_pixel); what is
new is WHERE the operands live.  Inputs, weights, affines, statistics, workspaces and outputs are views into one uint8 tensor
filled with 0xFF (NaN as a float, -1 as an int) or 0x7F (3.4e38 / 2139062143), at 16-byte but never 256-byte multiples, each with
64 KiB of pattern on both sides, workspaces of exactly the queried size.  So:

  * an output element that is never stored, or scratch that is read before it is written (a multiply-by-zero mask hides a finite
    leftover, not a NaN), reaches the oracle comparison;
  * a store or a carve past the stated extent lands in a guard band and arena.check() names it; a changed input is named too;
  * a halo load past a tensor's end picks up poison, not a finite neighbour;
  * float64 accumulators the header says the caller zeroes are zeroed with mvs_zero_f64 inside the arena; everything else
    starts as pattern.

Calls go through the C ABI with small ctypes wrappers in this file.  Section 3 (calls that follow each other) runs two different
inputs back to back through the same scratch, a larger shape between two runs of a smaller one, and one call on a side stream.

The 3-D convolution files and the case that reaches each (dispatch: regnet.hip mvs_conv3d_f32 / mvs_deconv3d_f32,
conv3d_mfma.hip mvs_conv3d_dispatch, deconv3d_mfma.hip mvs_deconv3d_mfma_launch, conv3d_os.hip mvs_conv3d_os_launch; cases are
(D, H, W, Cin, Cout[, stride]) of CONV_CASES / DECONV_CASES / EXTRA_* below, under conv impl `auto` unless stated):

    conv3d_mfma     conv (4,8,8,16,16,1) and (6,16,32,16,16,1): launch_s1<16,16,8>; (5,12,40,32,16,1): the 2x8 column tiles;
                    (5,32,12,64,16,1): the 4x4 column tiles; (8,8,16,32,8,1) FUSED form (x2 given): launch_s1<32,8,8>;
                    the fused 3dconv1_1 + 2_0 launch: RegNetUS0 at (32,32,64) and (40,24,48) (REGNET_ROUTES)
    conv3d_s2_mfma  conv (8,8,16,32,16,2) and (4,4,8,16,32,2); the s2_planes hook cases
    conv3d_os       conv (4,4,4,64,64,1), (6,16,24,32,32,1), (4,16,20,64,64,1), (5,9,12,64,128,2), (6,10,14,64,32,2),
                    (3,6,10,128,128,1); deconv (2,2,4,64,32), (4,4,8,32,16), (3,5,6,128,64); the filled launches: RegNetUS0
                    prepared at (32,32,64) / (40,24,48)
    conv3d_c8       conv (8,8,16,32,8,1) and (7,8,16,32,8,1) PLAIN form; conv3d_pair at (8,8,16) and (10,12,24); the pair_planes
                    and span_force hook cases
    conv3d_k8       EXTRA_CONV (6,10,12,8,32,1), plain form only (the kernel takes no affine, skip or statistics)
    conv3d_c1       EXTRA_CONV (6,10,12,1,8,1) and (5,9,20,1,4,1), plain form only
    conv3d_out      conv (8,16,16,8,1,1) PLAIN form (with statistics the launcher answers MVS_E_SHAPE: scalar); 3dconv6_2 of every
                    RegNetUS0 case
    conv3d_scalar   every case under impl `scalar`; under `auto` conv (6,10,12,8,8,1), (6,10,12,12,6,2), deconv (3,5,6,8,4) and the
                    fused forms of the k8 / c1 / out cases
    deconv3d_mfma   EXTRA_DECONV (3,5,6,32,32): launch_deconv<32,16,8> (no block kernel covers 32 -> 32) and (3,5,6,16,16):
                    launch_deconv<16,16,8>
    deconv3d_c8     deconv (4,8,8,16,8); 3dconv6_0 of every RegNetUS0 case
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S
from mvsnet_amd import _lib as L

from tests import sweep_reference as SR
from tests.device_arena import PATTERNS, Arena
from tests.test_gpu_parity import CONV_CASES, DECONV_CASES

pytestmark = pytest.mark.gpu

DEV = "cuda"
BN_EPSILON = 1e-5
MVS_E_WORKSPACE = -3
F32, F64, U8 = torch.float32, torch.float64, torch.uint8
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


# ---- small helpers -----------------------------------------------------------------------------------------------------------
def arena(pattern, mb=24):
    return Arena(mb << 20, pattern, DEV)


def put(a, name, array, dtype=F32):
    """An input / weight: copied in, read-only."""
    return a.take(np.shape(array), dtype, data=np.ascontiguousarray(array), readonly=True, name=name)


def out(a, name, *shape, dtype=F32):
    return a.take(shape, dtype, name=name)


def zeroed_f64(a, name, *shape):
    """A float64 accumulator the header says the caller zeroes: poisoned region, cleared by mvs_zero_f64 on the stream."""
    s = a.take(shape, F64, name=name)
    L.check(L.load().mvs_zero_f64(L.ptr(s), s.numel(), L.stream_ptr()), "mvs_zero_f64")
    return s


def vp(t_):
    return C.c_void_p(t_.data_ptr())


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / np.abs(b).sum())


def frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


# ==== warp and cost volume ====================================================================================================
@both_patterns
@pytest.mark.parametrize("inverse", [False, True])
def test_homographies(inverse, pattern):
    w = S.make_workload("small")
    D = w.depth_num
    end = w.depth_start + (D - 1) * w.depth_interval
    a = arena(pattern, 2)
    cams = put(a, "cams", w.cams)
    Hm = out(a, "homographies", w.view_num - 1, D, 3, 3)
    T = out(a, "transforms", w.view_num - 1, D, 8)
    L.check(L.load().mvs_homography_transforms_f32(L.ptr(cams), w.view_num, D, w.depth_start, w.depth_interval, end, int(inverse),
                                                   L.ptr(Hm), L.ptr(T), L.stream_ptr()), "mvs_homography_transforms_f32")
    T, Hm = n(T), n(Hm)
    a.check()
    for v in range(1, w.view_num):
        if inverse:
            Ho = O.get_homographies_inv_depth(w.cams[0], w.cams[v], D, w.depth_start, end, np.float64)
        else:
            Ho = O.get_homographies(w.cams[0], w.cams[v], D, w.depth_start, w.depth_interval, np.float64)
        np.testing.assert_allclose(Hm[v - 1], Ho, rtol=2e-5, atol=2e-4)
        np.testing.assert_allclose(T[v - 1], O.homography_to_transform8(Ho, np.float64), rtol=2e-5, atol=2e-4)


@functools.lru_cache(maxsize=None)
def warp_case():
    from mvsnet_amd.homography_warping import homography_to_transform8
    rs = np.random.RandomState(2)
    img = rs.standard_normal((24, 40, 16)).astype(np.float32)
    Hs = []
    for k in range(4):
        Hm = np.eye(3) + 0.03 * rs.standard_normal((3, 3))
        Hm[2, :2] *= 0.01
        Hm[:2, 2] += rs.uniform(-6, 6, 2)
        Hs.append(Hm)
    t8 = [homography_to_transform8(torch.as_tensor(Hm, dtype=torch.float32)).numpy() for Hm in Hs]
    exp = {"zeros": [O.tf_transform_homography(img, Hm, np.float64) for Hm in Hs],
           "clamp": [O.homography_warping_clamp(img, Hm, np.float64) for Hm in Hs]}
    return img, t8, exp


@both_patterns
@pytest.mark.parametrize("border", ["zeros", "clamp"])
def test_warp(border, pattern):
    img, t8, exp = warp_case()
    a = arena(pattern, 2)
    x = put(a, "image", img)
    for k in range(4):
        tr = put(a, "transform%d" % k, t8[k])
        y = out(a, "out%d" % k, *img.shape)
        L.check(L.load().mvs_warp_f32(L.ptr(x), L.ptr(tr), 24, 40, 16, 0 if border == "zeros" else 1, L.ptr(y), L.stream_ptr()),
                "mvs_warp_f32")
        got = n(y)
        bad = ~(np.abs(got - exp[border][k]) <= 1e-4 * (1 + np.abs(exp[border][k])))      # (NaN counts as bad)
        assert bad.mean() < 1e-3, bad.mean()
    a.check()


def cost_volume(a, ref, src, T, d_begin, d_count, variant, negate, name="cost"):
    """mvs_cost_volume_f32 on arena tensors ref (H,W,C), src (N-1,H,W,C), T (N-1,D,8) -> a fresh (d_count,H,W,C) output."""
    H, W, Cc = ref.shape
    y = out(a, name, d_count, H, W, Cc)
    L.check(L.load().mvs_cost_volume_f32(L.ptr(ref), L.ptr(src), L.ptr(T), src.shape[0] + 1, T.shape[1], d_begin, d_count, H, W, Cc,
                                         0 if variant == "mem" else 1, int(negate), 0, L.ptr(y), L.stream_ptr()), "mvs_cost_volume_f32")
    return y


@functools.lru_cache(maxsize=None)
def cv_small_case(variant):
    from mvsnet_amd.homography_warping import homography_transforms
    w = S.make_workload("small")
    T = homography_transforms(torch.as_tensor(w.cams).to(DEV), w.depth_num, w.depth_start, w.depth_interval).cpu().numpy()
    fn = O.variance_cost_mem if variant == "mem" else O.variance_cost_eager
    exp = np.stack([fn(w.features[0], [O.image_projective_transform_bilinear(w.features[v + 1], T[v, d].astype(np.float64), np.float64)
                                       for v in range(w.view_num - 1)], w.view_num, np.float64) for d in range(w.depth_num)])
    return (w,) + frozen(T, exp)


@both_patterns
@pytest.mark.parametrize("variant", ["mem", "eager"])
def test_cost_volume_small(variant, pattern):
    w, T, exp = cv_small_case(variant)
    a = arena(pattern, 16)
    ref, src, Td = put(a, "ref", w.features[0]), put(a, "src", w.features[1:]), put(a, "transforms", T)
    got = n(cost_volume(a, ref, src, Td, 0, w.depth_num, variant, False))
    assert got.shape == (w.depth_num, w.height, w.width, w.channels)
    assert (~(np.abs(got - exp) <= 1e-4)).mean() < 1e-3          # tap flips at near-integer samples
    assert rel_l1(got, exp) < 1e-5
    neg = n(cost_volume(a, ref, src, Td, 0, w.depth_num, variant, True, "negated volume"))
    np.testing.assert_allclose(neg, -got, rtol=1e-4, atol=5e-5)   # the bound of the negated plane below
    one = n(cost_volume(a, ref, src, Td, 3, 1, variant, True, "negated plane"))
    np.testing.assert_allclose(one[0], -got[3], rtol=1e-4, atol=5e-5)   # per-plane kernel vs depth sweep (fp32 cancellation noise)
    # a sub-range into an output of exactly two planes: a store to plane 3 or later of it is an overrun the guards see
    two = n(cost_volume(a, ref, src, Td, 3, 2, variant, False, "planes 3-4"))
    np.testing.assert_allclose(two, got[3:5], rtol=1e-4, atol=5e-5)
    a.check()


@both_patterns
def test_cost_volume_sub_range_of_eight_planes(pattern):
    """d_begin = 3, d_count = 2 of 8 planes on the quarter-pixel grid of the smallest-image test: exact against the oracle."""
    rs = np.random.RandomState(51)
    H, W = 6, 10
    refa = rs.randint(-4, 5, size=(H, W, 32)).astype(np.float32)
    srca = rs.randint(-4, 5, size=(2, H, W, 32)).astype(np.float32)
    shifts = [(0.0, 0.0), (-0.5, 0.25), (0.75, -0.75), (-1.25, 1.0), (1.5, 1.5), (-2.0, -2.0), (0.25, 0.5), (3.0, 0.0)]
    T = np.zeros((2, 8, 8), np.float32); T[:, :, 0] = 1; T[:, :, 4] = 1
    for d, (sx, sy) in enumerate(shifts):
        T[0, d, 2], T[0, d, 5] = sx, sy
        T[1, d, 2], T[1, d, 5] = -sy, sx
    a = arena(pattern, 2)
    got = n(cost_volume(a, put(a, "ref", refa), put(a, "src", srca), put(a, "transforms", T), 3, 2, "mem", False))
    assert got.shape == (2, H, W, 32)
    for k, d in enumerate((3, 4)):
        warped = [O.image_projective_transform_bilinear(srca[v], T[v, d].astype(np.float64), np.float64) for v in range(2)]
        np.testing.assert_allclose(got[k], O.variance_cost_mem(refa, warped, 3, np.float64), rtol=0, atol=2e-5, err_msg="plane %d" % d)
    a.check()


@both_patterns
@pytest.mark.parametrize("hw", [(2, 2), (2, 9), (7, 2), (1, 6), (5, 1)])
def test_cost_volume_smallest_images(hw, pattern):
    rs = np.random.RandomState(51)
    H, W = hw
    refa = rs.randint(-4, 5, size=(H, W, 32)).astype(np.float32)
    srca = rs.randint(-4, 5, size=(2, H, W, 32)).astype(np.float32)
    shifts = [(0.0, 0.0), (-0.5, 0.25), (0.75, -0.75), (-1.25, 1.0), (1.5, 1.5), (-2.0, -2.0), (0.25, 0.5), (3.0, 0.0)]
    T = np.zeros((2, len(shifts), 8), np.float32); T[:, :, 0] = 1; T[:, :, 4] = 1
    for d, (sx, sy) in enumerate(shifts):
        T[0, d, 2], T[0, d, 5] = sx, sy
        T[1, d, 2], T[1, d, 5] = -sy, sx
    a = arena(pattern, 2)
    got = n(cost_volume(a, put(a, "ref", refa), put(a, "src", srca), put(a, "transforms", T), 0, len(shifts), "mem", False))
    a.check()
    for d in range(len(shifts)):
        warped = [O.image_projective_transform_bilinear(srca[v], T[v, d].astype(np.float64), np.float64) for v in range(2)]
        np.testing.assert_allclose(got[d], O.variance_cost_mem(refa, warped, 3, np.float64), rtol=0, atol=2e-5, err_msg="plane %d" % d)


@both_patterns
@pytest.mark.parametrize("Cc", [4, 8, 16, 32, 64])
def test_cost_volume_channel_counts(Cc, pattern):
    """6 x 10 on the quarter-pixel grid (exact products), every channel count the sweep is built for."""
    rs = np.random.RandomState(60 + Cc)
    H, W = 6, 10
    refa = rs.randint(-4, 5, size=(H, W, Cc)).astype(np.float32)
    srca = rs.randint(-4, 5, size=(2, H, W, Cc)).astype(np.float32)
    shifts = [(0.0, 0.0), (-0.5, 0.25), (0.75, -0.75), (W - 1.25, 1.0), (1.5, H - 0.5), (-2.0, -2.0)]
    T = np.zeros((2, len(shifts), 8), np.float32); T[:, :, 0] = 1; T[:, :, 4] = 1
    for d, (sx, sy) in enumerate(shifts):
        T[0, d, 2], T[0, d, 5] = sx, sy
        T[1, d, 2], T[1, d, 5] = -sy, sx
    a = arena(pattern, 2)
    got = n(cost_volume(a, put(a, "ref", refa), put(a, "src", srca), put(a, "transforms", T), 0, len(shifts), "mem", False))
    a.check()
    for d in range(len(shifts)):
        warped = [O.image_projective_transform_bilinear(srca[v], T[v, d].astype(np.float64), np.float64) for v in range(2)]
        np.testing.assert_allclose(got[d], O.variance_cost_mem(refa, warped, 3, np.float64), rtol=0, atol=2e-5, err_msg="plane %d" % d)


# ==== 3-D convolutions ========================================================================================================
def conv3d(a, x, w, stride, y_shape, xa=None, x2=None, x2a=None, stats=None, transpose=False, name="y"):
    """mvs_conv3d_f32 / mvs_deconv3d_f32 on arena tensors into a fresh poisoned output."""
    lib = L.load()
    D, H, W, Cin = x.shape
    y = out(a, name, *y_shape)
    xs, xb = xa if xa is not None else (None, None)
    ss, sb = x2a if x2a is not None else (None, None)
    if transpose:
        L.check(lib.mvs_deconv3d_f32(L.ptr(x), L.ptr(xs), L.ptr(xb), L.ptr(x2), L.ptr(ss), L.ptr(sb), L.ptr(w), D, H, W, Cin,
                                     y_shape[3], L.ptr(y), L.ptr(stats), L.stream_ptr()), "mvs_deconv3d_f32")
    else:
        L.check(lib.mvs_conv3d_f32(L.ptr(x), L.ptr(xs), L.ptr(xb), L.ptr(x2), L.ptr(ss), L.ptr(sb), L.ptr(w), D, H, W, Cin,
                                   y_shape[3], stride, L.ptr(y), L.ptr(stats), L.stream_ptr()), "mvs_conv3d_f32")
    return y


@functools.lru_cache(maxsize=None)
def conv_case(case):
    """Inputs and float64 expectations of test_gpu_parity.test_conv3d_matches_oracle for one case."""
    D, H, W, Cin, Cout, stride = case
    rs = np.random.RandomState(sum(case))
    x = rs.standard_normal((D, H, W, Cin)).astype(np.float32)
    x2 = rs.standard_normal((D, H, W, Cin)).astype(np.float32)
    wgt = (rs.standard_normal((3, 3, 3, Cin, Cout)) / np.sqrt(27 * Cin)).astype(np.float32)
    sc = (1 + 0.3 * rs.standard_normal(Cin)).astype(np.float32); sh = (0.2 * rs.standard_normal(Cin)).astype(np.float32)
    sc2 = (1 + 0.3 * rs.standard_normal(Cin)).astype(np.float32); sh2 = (0.2 * rs.standard_normal(Cin)).astype(np.float32)
    gamma = (1 + 0.2 * rs.standard_normal(Cout)).astype(np.float32); beta = (0.1 * rs.standard_normal(Cout)).astype(np.float32)
    e_plain = O.conv3d_same(x, wgt, stride, np.float64)
    xin = np.maximum(x * sc + sh, 0).astype(np.float64) + np.maximum(x2 * sc2 + sh2, 0)
    e_fused = O.conv3d_same(xin, wgt, stride, np.float64)
    e_bn = O.batch_norm_train(e_fused, gamma, beta, 1e-5, True, np.float64)
    return frozen(x, x2, wgt, sc, sh, sc2, sh2, gamma, beta, e_plain, e_fused, e_bn)


def check_conv_case(case, impl, pattern, fused=True):
    D, H, W, Cin, Cout, stride = case
    x, x2, wgt, sc, sh, sc2, sh2, gamma, beta, e_plain, e_fused, e_bn = conv_case(case)
    a = arena(pattern, 8)
    dx, dw = put(a, "x", x), put(a, "w", wgt)
    L.set_conv_impl(impl)
    try:
        y_plain = n(conv3d(a, dx, dw, stride, e_plain.shape, name="y_plain"))
        np.testing.assert_allclose(y_plain, e_plain, rtol=1e-4, atol=2e-5)
        if fused:
            stats = zeroed_f64(a, "stats", 2, Cout)
            y_fused = n(conv3d(a, dx, dw, stride, e_fused.shape, (put(a, "x_scale", sc), put(a, "x_shift", sh)), put(a, "x2", x2),
                               (put(a, "x2_scale", sc2), put(a, "x2_shift", sh2)), stats, name="y_fused"))
            st = n(stats)
            np.testing.assert_allclose(y_fused, e_fused, rtol=1e-4, atol=2e-5)
            np.testing.assert_allclose(st[0], e_fused.reshape(-1, Cout).sum(0), rtol=1e-4, atol=1e-3)
            np.testing.assert_allclose(st[1], (e_fused.reshape(-1, Cout) ** 2).sum(0), rtol=1e-4, atol=1e-3)
            scale, shift = out(a, "scale", Cout), out(a, "shift", Cout)
            L.check(L.load().mvs_bn_finalize_f32(L.ptr(stats), Cout, float(e_fused.size // Cout), L.ptr(put(a, "gamma", gamma)),
                                                 L.ptr(put(a, "beta", beta)), BN_EPSILON, L.ptr(scale), L.ptr(shift), L.stream_ptr()),
                    "mvs_bn_finalize_f32")
            np.testing.assert_allclose(np.maximum(e_fused * n(scale) + n(shift), 0), e_bn, rtol=1e-4, atol=1e-5)
    finally:
        L.set_conv_impl("auto")
    a.check()


@both_patterns
@pytest.mark.parametrize("impl", ["scalar", "auto"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv3d(case, impl, pattern):
    check_conv_case(case, impl, pattern)


# conv3d_k8.hip (8 -> 32) and conv3d_c1.hip (1 -> 8, 1 -> 4) take the plain form only: no case of CONV_CASES reaches them
EXTRA_CONV = [(6, 10, 12, 8, 32, 1), (6, 10, 12, 1, 8, 1), (5, 9, 20, 1, 4, 1)]


@both_patterns
@pytest.mark.parametrize("case", EXTRA_CONV, ids=lambda c: "x".join(map(str, c)))
def test_conv3d_training_side_kernels(case, pattern):
    check_conv_case(case, "auto", pattern)           # (with affines and statistics the same shapes take the scalar kernel)


@functools.lru_cache(maxsize=None)
def deconv_case(case):
    D, H, W, Cin, Cout = case
    rs = np.random.RandomState(sum(case) + 7)
    x = rs.standard_normal((D, H, W, Cin)).astype(np.float32)
    x2 = rs.standard_normal((D, H, W, Cin)).astype(np.float32)
    wgt = (rs.standard_normal((3, 3, 3, Cout, Cin)) / np.sqrt(27 * Cin)).astype(np.float32)
    sc = (1 + 0.3 * rs.standard_normal(Cin)).astype(np.float32); sh = (0.2 * rs.standard_normal(Cin)).astype(np.float32)
    e_plain = O.conv3d_transpose_same(x, wgt, 2, np.float64)
    xin = np.maximum(x * sc + sh, 0).astype(np.float64) + np.maximum(x2 * sc + sh, 0)
    e_fused = O.conv3d_transpose_same(xin, wgt, 2, np.float64)
    return frozen(x, x2, wgt, sc, sh, e_plain, e_fused)


EXTRA_DECONV = [(3, 5, 6, 32, 32), (3, 5, 6, 16, 16)]        # deconv3d_mfma.hip's own kernels: no block kernel, no packed kernel


@both_patterns
@pytest.mark.parametrize("impl", ["scalar", "auto"])
@pytest.mark.parametrize("case", DECONV_CASES + EXTRA_DECONV, ids=lambda c: "x".join(map(str, c)))
def test_deconv3d(case, impl, pattern):
    D, H, W, Cin, Cout = case
    x, x2, wgt, sc, sh, e_plain, e_fused = deconv_case(case)
    a = arena(pattern, 8)
    dx, dw = put(a, "x", x), put(a, "w", wgt)
    shape = (2 * D, 2 * H, 2 * W, Cout)
    L.set_conv_impl(impl)
    try:
        y_plain = n(conv3d(a, dx, dw, 2, shape, transpose=True, name="y_plain"))
        stats = zeroed_f64(a, "stats", 2, Cout)
        aff = (put(a, "scale", sc), put(a, "shift", sh))
        y_fused = n(conv3d(a, dx, dw, 2, shape, aff, put(a, "x2", x2), aff, stats, transpose=True, name="y_fused"))
        st = n(stats)
    finally:
        L.set_conv_impl("auto")
    a.check()
    np.testing.assert_allclose(y_plain, e_plain, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(y_fused, e_fused, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(st[0], e_fused.reshape(-1, Cout).sum(0), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(st[1], (e_fused.reshape(-1, Cout) ** 2).sum(0), rtol=1e-4, atol=1e-3)


@functools.lru_cache(maxsize=None)
def pair_case(D, H, W):
    rs = np.random.RandomState(D * 1000 + H * 10 + W)
    x = rs.standard_normal((D, H, W, 32)).astype(np.float32)
    w1 = (rs.standard_normal((3, 3, 3, 32, 8)) / np.sqrt(27 * 32)).astype(np.float32)
    w2 = (rs.standard_normal((3, 3, 3, 32, 16)) / np.sqrt(27 * 32)).astype(np.float32)
    return frozen(x, w1, w2, O.conv3d_same(x, w1, 1, np.float64), O.conv3d_same(x, w2, 2, np.float64))


def check_pair(shape, pattern, **hooks):
    D, H, W = shape
    x, w1, w2, e1, e2 = pair_case(D, H, W)
    a = arena(pattern, 8)
    dx, dw1, dw2 = put(a, "x", x), put(a, "w1", w1), put(a, "w2", w2)
    s1, s2 = zeroed_f64(a, "stats1", 2, 8), zeroed_f64(a, "stats2", 2, 16)
    y1, y2 = out(a, "y1", D, H, W, 8), out(a, "y2", D // 2, H // 2, W // 2, 16)
    with L.test_hooks(**hooks):
        L.check(L.load().mvs_conv3d_pair_f32(L.ptr(dx), L.ptr(dw1), L.ptr(dw2), D, H, W, 32, 8, 16, L.ptr(y1), L.ptr(s1), L.ptr(y2),
                                             L.ptr(s2), L.stream_ptr()), "mvs_conv3d_pair_f32")
        torch.cuda.synchronize()
    a.check()
    np.testing.assert_allclose(n(y1), e1, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(n(y2), e2, rtol=1e-4, atol=2e-5)
    for st, e, c in ((n(s1), e1, 8), (n(s2), e2, 16)):
        np.testing.assert_allclose(st[0], e.reshape(-1, c).sum(0), rtol=1e-4, atol=1e-3)
        np.testing.assert_allclose(st[1], (e.reshape(-1, c) ** 2).sum(0), rtol=1e-4, atol=1e-3)


@both_patterns
@pytest.mark.parametrize("shape", [(8, 8, 16), (10, 12, 24)])
def test_conv3d_pair(shape, pattern):
    check_pair(shape, pattern)


@both_patterns
@pytest.mark.parametrize("hooks", [dict(pair_planes=2, conv_no_span=1), dict(pair_planes=4, conv_no_span=0)],
                         ids=["planes2-chunks", "planes4"])
def test_conv3d_pair_halo_plane_hooks(hooks, pattern):
    """test_gpu_halo_planes.test_pair_halo_planes at its smallest volume with interior first / last planes (D = 12, 8 x 16)."""
    check_pair((12, 8, 16), pattern, **hooks)


@both_patterns
def test_conv3d_pair_span_crossing(pattern):
    """test_gpu_halo_planes.test_pair_span_crossing_at_small_size: ranges of 24 planes across the tile boundary at plane 36."""
    check_pair((36, 8, 32), pattern, span_force=2 << 8 | 3)


@both_patterns
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("case", [(7, 8, 16, 16, 16), (7, 8, 16, 32, 8)], ids=lambda c: "x".join(map(str, c)))
def test_conv3d_s1_halo_plane_hook(case, planes, pattern):
    """MVS_HOOK_S1_PLANES at the smallest shapes of test_gpu_halo_planes.S1_SHAPES: conv3d_s1_kernel and the unfused 32 -> 8 kernel."""
    with L.test_hooks(s1_planes=planes):
        check_conv_case(case + (1,), "auto", pattern)


@functools.lru_cache(maxsize=None)
def s2_case(depth):
    cin, cout, H, W = 16, 32, 6, 20
    rs = np.random.RandomState(1000 * cin + 10 * depth)
    x = rs.standard_normal((depth, H, W, cin)).astype(np.float32)
    wgt = (rs.standard_normal((3, 3, 3, cin, cout)) / np.sqrt(27 * cin)).astype(np.float32)
    sc = (1 + 0.3 * rs.standard_normal(cin)).astype(np.float32); sh = (0.2 * rs.standard_normal(cin)).astype(np.float32)
    return frozen(x, wgt, sc, sh, O.conv3d_same(np.maximum(x * sc + sh, 0).astype(np.float64), wgt, 2, np.float64))


@both_patterns
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("depth", [5, 6])
def test_conv3d_s2_planes_hook(depth, planes, pattern):
    x, wgt, sc, sh, e = s2_case(depth)
    a = arena(pattern, 4)
    stats = zeroed_f64(a, "stats", 2, 32)
    with L.test_hooks(s2_planes=planes):
        y = n(conv3d(a, put(a, "x", x), put(a, "w", wgt), 2, e.shape, (put(a, "scale", sc), put(a, "shift", sh)), stats=stats))
    a.check()
    np.testing.assert_allclose(y, e, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(n(stats)[0], e.reshape(-1, 32).sum(0), rtol=1e-4, atol=1e-3)


# ==== RegNetUS0 ===============================================================================================================
class ArenaRegnet:
    """RegNetUS0 parameters inside an arena: the 11 kernels, 10 gammas and betas read-only, and the prepared buffer of exactly
    mvs_regnet_prepared_floats() floats filled by mvs_regnet_prepare_f32 in place."""

    def __init__(self, a, params, pad=True):
        from mvsnet_amd.model import RegNetWeights
        lib = L.load()
        host = RegNetWeights(params, DEV, pad_to_mfma=pad)          # shapes, padding and base only; its tensors are copied in
        self.cin, self.base = host.cin, host.base
        self.w = [put(a, "w%d" % i, n(t_)) for i, t_ in enumerate(host.w)]
        self.gamma = [put(a, "gamma%d" % i, n(t_)) for i, t_ in enumerate(host.gamma)]
        self.beta = [put(a, "beta%d" % i, n(t_)) for i, t_ in enumerate(host.beta)]
        self.w_ptrs, self.g_ptrs, self.b_ptrs = L.ptr_array(self.w), L.ptr_array(self.gamma), L.ptr_array(self.beta)
        nf = lib.mvs_regnet_prepared_floats(self.cin, self.base)
        assert nf > 0
        self.prepared = out(a, "prepared", nf)
        L.check(lib.mvs_regnet_prepare_f32(self.w_ptrs, self.cin, self.base, L.ptr(self.prepared), L.stream_ptr()), "mvs_regnet_prepare_f32")

    def ws_bytes(self, D, H, W):
        return L.load().mvs_regnet_workspace_bytes(D, H, W, self.cin, self.base)

    def run(self, entry, cost, ws, reg, ws_bytes=None):
        """entry: 'prepared' | 'plain' | 'batch'; cost (D,H,W,C) or (B,D,H,W,C).  Returns the library's return code."""
        lib = L.load()
        *batch, D, H, W, Cc = cost.shape
        nb = ws.numel() if ws_bytes is None else ws_bytes
        tail = (BN_EPSILON, vp(ws), nb, L.ptr(reg), L.stream_ptr())
        if entry == "plain":
            return lib.mvs_regnet_us0_f32(L.ptr(cost), D, H, W, Cc, self.base, self.w_ptrs, self.g_ptrs, self.b_ptrs, *tail)
        if entry == "batch":
            return lib.mvs_regnet_us0_batch_f32(L.ptr(cost), batch[0], D, H, W, Cc, self.base, self.w_ptrs, L.ptr(self.prepared),
                                                self.g_ptrs, self.b_ptrs, *tail)
        return lib.mvs_regnet_us0_prepared_f32(L.ptr(cost), D, H, W, Cc, self.base, self.w_ptrs, L.ptr(self.prepared),
                                               self.g_ptrs, self.b_ptrs, *tail)


@functools.lru_cache(maxsize=None)
def regnet_case(mode, shape, batch=1, seed=None):
    """(params, cost, float64 oracle) shared by every test of a (mode, shape); batch = 2: two samples sharing BatchNorm sums.
    Inputs as in test_gpu_parity: parameter seed 11, cost seed 12 (test_regnet_matches_oracle), 13 for 'fat'
    (test_fat_mode_matches_oracle: its rel-L1 bound of 2e-5 belongs to that volume -- with cost seed 12 the 64-channel network
    measured 2.876e-5 under both patterns, the same figure to four digits: fp32 rounding of its 1728- to 3456-term sums, not a
    leak of poison)."""
    D, H, W = shape
    if seed is None:
        seed = 13 if mode == "fat" else 12
    params = S.make_regnet_params(mode, seed=11, random_affine=True)
    Cc = 4 * S.base_filter(mode)
    cost = np.abs(np.random.RandomState(seed).standard_normal((batch, D, H, W, Cc))).astype(np.float32)
    if batch == 1:
        cost = cost[0]
        exp = O.regnet_us0(cost, params, np.float64)
    else:
        exp = np.stack(O.regnet_us0_batch(list(cost), params, np.float64))
    cost.setflags(write=False); exp.setflags(write=False)
    return params, cost, exp


def regnet_mb(shape, Cc=32, batch=1):
    return 12 + int(batch * np.prod(shape) * (Cc + 40) * 4 * 1.25) // (1 << 20)


def check_regnet(mode, shape, entry, pattern, impl="auto", pad=True, **hooks):
    batch = 2 if entry == "batch" else 1
    params, cost, exp = regnet_case(mode, shape, batch)
    weights_mb = 3 * 4 * sum(np.size(p["w"]) for p in params.values()) >> 20          # the kernels and their prepared layouts
    a = arena(pattern, regnet_mb(shape, max(cost.shape[-1], 32), batch) + weights_mb)
    net = ArenaRegnet(a, params, pad)
    if cost.shape[-1] != net.cin:                                   # a narrower mode running zero-padded on the MFMA shapes
        cost = np.pad(cost, [(0, 0)] * (cost.ndim - 1) + [(0, net.cin - cost.shape[-1])])
    dcost = put(a, "cost", cost)
    ws = a.take_bytes(batch * net.ws_bytes(*shape), "workspace")
    reg = out(a, "reg", *exp.shape)
    L.set_conv_impl(impl)
    try:
        with L.test_hooks(**hooks):
            L.check(net.run(entry, dcost, ws, reg), "regnet %s" % entry)
            got = n(reg)
    finally:
        L.set_conv_impl("auto")
    a.check()
    assert got.shape == exp.shape
    assert rel_l1(got, exp) < 2e-5
    np.testing.assert_allclose(got, exp, rtol=1e-3, atol=2e-4)


REGNET_SHAPES = [(8, 8, 8), (8, 16, 16), (16, 8, 24), (40, 24, 48), (32, 32, 64)]      # the last two: pair, fuse2 and filler routes


@both_patterns
@pytest.mark.parametrize("entry", ["prepared", "plain", "batch"])
@pytest.mark.parametrize("shape", REGNET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_regnet(shape, entry, pattern):
    check_regnet("normal", shape, entry, pattern)


@both_patterns
@pytest.mark.parametrize("mode,shape,impl,pad", [("fat", (8, 8, 16), "auto", True), ("lite", (16, 8, 24), "auto", False),
                                                 ("normal", (8, 16, 16), "scalar", True)], ids=["fat", "lite-unpadded", "scalar"])
def test_regnet_other_modes(mode, shape, impl, pad, pattern):
    check_regnet(mode, shape, "prepared", pattern, impl, pad)


@both_patterns
@pytest.mark.parametrize("hooks", [dict(fuse2_planes=4), dict(fuse2_planes=2, conv_full_sweeps=5), dict(conv_no_fuse2=1),
                                   dict(conv_no_span=1), dict(bn_slots=1, pair_slots=1), dict(out_planes=3)],
                         ids=lambda h: "+".join("%s%d" % kv for kv in h.items()))
def test_regnet_schedule_hooks(hooks, pattern):
    """The schedules the hooks force at (16,16,32), test_gpu_halo_planes' volume for the fused 3dconv1_1 + 2_0 launch (its
    half-resolution level is (8,8,16): chunks of 2 and 4 planes, a short last chunk), each with exact scratch full of poison:
    the layers apart, whole depth chunks, one partial row of BatchNorm sums, 3dconv6_2 in several chunks."""
    check_regnet("normal", (16, 16, 32), "prepared", pattern, **hooks)


@both_patterns
def test_conv3d_pair_full_sweeps_hook(pattern):
    check_pair((12, 8, 16), pattern, pair_planes=4, conv_full_sweeps=5)


@both_patterns
@pytest.mark.parametrize("entry", ["prepared", "plain", "batch"])
def test_regnet_workspace_one_byte_short_is_refused_and_nothing_is_touched(entry, pattern):
    shape = (8, 16, 16)
    batch = 2 if entry == "batch" else 1
    params, cost, _exp = regnet_case("normal", shape, batch)
    a = arena(pattern, regnet_mb(shape, 32, batch))
    net = ArenaRegnet(a, params)
    need = batch * net.ws_bytes(*shape)
    ws = a.take_bytes(need - 1, "workspace")
    reg = out(a, "reg", *cost.shape[:-1])
    assert net.run(entry, put(a, "cost", cost), ws, reg) == MVS_E_WORKSPACE
    a.check()
    assert a.is_pattern(reg) and a.is_pattern(ws)


class DepthCall:
    """mvs_depth_from_features_f32 with transforms, cost, workspace and reg as poisoned scratch of exact size."""

    def __init__(self, a, net, w):
        self.a, self.net, self.w = a, net, w
        D, H, W, Cc = w.depth_num, w.height, w.width, w.channels
        self.transforms = out(a, "transforms", w.view_num - 1, D, 8)
        self.cost = out(a, "cost", D, H, W, Cc)
        self.ws = a.take_bytes(net.ws_bytes(D, H, W), "workspace")
        self.reg = out(a, "reg", D, H, W)
        self.cams = put(a, "cams", w.cams)

    def __call__(self, feats, depth, prob, inverse=False):
        w, net = self.w, self.net
        end = float(np.float32(w.depth_start) + (np.float32(w.depth_num) - np.float32(1)) * np.float32(w.depth_interval))
        L.check(L.load().mvs_depth_from_features_f32(
            L.ptr(feats), L.ptr(self.cams), w.view_num, w.depth_num, w.height, w.width, w.channels, net.base, float(w.depth_start),
            float(w.depth_interval), end, int(inverse), 0, net.w_ptrs, L.ptr(net.prepared), net.g_ptrs, net.b_ptrs, BN_EPSILON,
            L.ptr(self.transforms), L.ptr(self.cost), vp(self.ws), self.ws.numel(), L.ptr(self.reg), L.ptr(depth), L.ptr(prob),
            L.stream_ptr()), "mvs_depth_from_features_f32")


@functools.lru_cache(maxsize=None)
def depth_case(name, seed=0):
    w = S.make_workload(name, seed=seed)
    rp = S.make_regnet_params("normal", seed=1, random_affine=True)
    ed, ep = O.inference_mem_from_features(w.features, w.cams, w.depth_num, w.depth_start, w.depth_interval, rp, False, np.float64)
    return w, rp, ed, ep


def depth_mb(w):
    return 16 + int(w.depth_num * w.height * w.width * (w.channels + 40) * 4 * 1.25) // (1 << 20)


def assert_depth(depth, prob, ed, ep):
    abs_rel = float(np.mean(np.abs(depth - ed) / ed))
    assert abs_rel < 1e-4, abs_rel
    assert (~(np.abs(prob - ep) <= 1e-3)).mean() < 0.02


@both_patterns
@pytest.mark.parametrize("name", ["toy", "small"])
def test_depth_from_features(name, pattern):
    w, rp, ed, ep = depth_case(name)
    a = arena(pattern, depth_mb(w))
    call = DepthCall(a, ArenaRegnet(a, rp), w)
    depth, prob = out(a, "depth", w.height, w.width), out(a, "prob", w.height, w.width)
    call(put(a, "features", w.features), depth, prob)
    depth, prob = n(depth), n(prob)
    a.check()
    assert_depth(depth, prob, ed, ep)


# ==== soft-argmin and the winner-take-all tail ================================================================================
@functools.lru_cache(maxsize=None)
def softargmin_case(D, H, W, inverse):
    rs = np.random.RandomState(5)
    reg = (2.0 * rs.standard_normal((D, H, W))).astype(np.float32)
    reg[7 % D, 3 % H, 4 % W] = -60.0                       # near one-hot pixel
    ed, ep = O.softargmin_and_prob(reg, D, 425.0, 2.65, inverse, np.float64)
    return frozen(reg, ed, ep)


@both_patterns
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("shape", [(48, 20, 28), (48, 20, 1), (48, 1, 28)], ids=lambda s: "x".join(map(str, s)))
def test_softargmin_prob(shape, inverse, pattern):
    D, H, W = shape
    reg, ed, ep = softargmin_case(D, H, W, inverse)
    a = arena(pattern, 2)
    depth, prob = out(a, "depth", H, W), out(a, "prob", H, W)
    L.check(L.load().mvs_softargmin_prob_f32(L.ptr(put(a, "reg", reg)), D, H, W, 425.0, 2.65, int(inverse), L.ptr(depth), L.ptr(prob),
                                             L.stream_ptr()), "mvs_softargmin_prob_f32")
    depth, prob = n(depth), n(prob)
    a.check()
    np.testing.assert_allclose(depth, ed, rtol=2e-6)
    assert (~(np.abs(prob - ep) <= 1e-5)).mean() < 5e-3      # bucket indices flip when (depth-start)/interval is within rounding of an integer


@both_patterns
def test_wta_update_and_finish_known_answers(pattern):
    """test_gpu_sweep_every_pixel's known answers: the first maximum is kept, exp_sum is the float32 running sum in plane order."""
    lib = L.load()
    P, W = 6, 70
    rs = np.random.RandomState(4)
    reg = rs.uniform(-2.0, 0.5, size=(P, W)).astype(np.float32)
    reg[3, :20] = reg[1, :20] = 1.0 + 0.01 * np.arange(20, dtype=np.float32)
    reg[4, 10:30] = 2.5
    reg[5, 25:40] = 2.5
    reg[:, 40:50] = -1000.0
    reg[:, 50:60] = -1000.0; reg[2, 50:60] = -0.25
    depths = (425.0 + 30.0 * np.arange(P)).astype(np.float32)
    a = arena(pattern, 4)
    sp = L.stream_ptr()
    dreg = put(a, "reg", reg)
    zeros = np.zeros(W, np.float32)
    state = lambda tag: [a.take((W,), F32, data=zeros, name="%s %s" % (k, tag)) for k in ("max_prob", "depth_image", "exp_sum")]
    pexp = np.empty_like(reg)
    for d in range(P):                                    # the device's own exp of every score: one update from zero
        mp, di, es = state("plane %d" % d)
        L.check(lib.mvs_wta_update_f32(L.ptr(dreg[d]), float(depths[d]), 1, W, L.ptr(mp), L.ptr(di), L.ptr(es), sp))
        pexp[d] = n(es)
        assert torch.equal(mp, es)
    exact = np.exp(reg.astype(np.float64))
    assert np.all(np.abs(pexp - exact) <= 2 * np.spacing(exact.astype(np.float32)))
    mp, di, es = state("sweep")
    for d in range(P):
        L.check(lib.mvs_wta_update_f32(L.ptr(dreg[d]), float(depths[d]), 1, W, L.ptr(mp), L.ptr(di), L.ptr(es), sp))
    prob = out(a, "prob", W)
    L.check(lib.mvs_wta_finish_f32(L.ptr(mp), L.ptr(es), 1, W, L.ptr(prob), sp))
    e_mp = np.zeros(W, np.float32); e_di = np.zeros(W, np.float32); e_es = np.zeros(W, np.float32)
    for d in range(P):
        upd = e_mp < pexp[d]
        e_mp = np.where(upd, pexp[d], e_mp); e_di = np.where(upd, depths[d], e_di); e_es = e_es + pexp[d]
    assert np.array_equal(n(di), e_di) and np.array_equal(n(mp), e_mp) and np.array_equal(n(es), e_es)
    assert np.array_equal(n(prob), e_mp / (e_es + np.float32(1e-7)))
    a.check()


# ==== the ConvGRU cell stages and the recurrent sweep =========================================================================
@both_patterns
def test_convgru_cell_stages(pattern):
    lib = L.load()
    rs = np.random.RandomState(6)
    H, W, Cin, F = 12, 20, 32, 16
    p = S.make_gru_params("normal", seed=8, in_channels=Cin, random_affine=True)["gru1"]
    x = rs.standard_normal((H, W, Cin)).astype(np.float32)
    h = rs.standard_normal((H, W, F)).astype(np.float32)
    a = arena(pattern, 4)
    dx = put(a, "x", x)
    dh = a.take((H, W, F), F32, data=h, name="h")          # updated in place by the blend
    g, c, rh, u = out(a, "g", H, W, 2 * F), out(a, "c", H, W, F), out(a, "rh", H, W, F), out(a, "u", H, W, F)
    st_g, st_c = zeroed_f64(a, "gate stats", 2, 2), zeroed_f64(a, "out stats", 1, 2)
    P = {k: put(a, k, v) for k, v in p.items()}
    sp = L.stream_ptr()
    L.check(lib.mvs_conv2d_cat_f32(L.ptr(dx), Cin, L.ptr(dh), F, L.ptr(P["gates_w"]), L.ptr(P["gates_b"]), H, W, 2 * F, L.ptr(g),
                                   L.ptr(st_g), 2, sp))
    L.check(lib.mvs_gru_gates_f32(L.ptr(g), L.ptr(st_g), L.ptr(P["reset_gamma"]), L.ptr(P["reset_beta"]), L.ptr(P["update_gamma"]),
                                  L.ptr(P["update_beta"]), L.ptr(dh), H, W, F, L.ptr(rh), L.ptr(u), sp))
    L.check(lib.mvs_conv2d_cat_f32(L.ptr(dx), Cin, L.ptr(rh), F, L.ptr(P["out_w"]), L.ptr(P["out_b"]), H, W, F, L.ptr(c), L.ptr(st_c), 1, sp))
    L.check(lib.mvs_gru_blend_f32(L.ptr(c), L.ptr(st_c), L.ptr(P["out_gamma"]), L.ptr(P["out_beta"]), L.ptr(u), H, W, F, L.ptr(dh), sp))
    got = n(dh)
    a.check()
    np.testing.assert_allclose(got, O.conv_gru_cell(x, h, p, np.float64), rtol=1e-4, atol=2e-5)


@pytest.fixture(scope="module")
def stream_set(_lib):
    """One stream set (mvs_gru_prepare: the call that calibrates and synchronises) for the wavefront routes of this file."""
    tok = L.gru_prepare()
    yield
    L.gru_unref(tok)


class SweepCall:
    """mvs_gru_wta_f32 / _batch_f32 with the parameters, transforms, features, a workspace of exactly views x
    mvs_gru_workspace_bytes() and the outputs in one arena.  Cases are sweep_reference.case dicts."""

    def __init__(self, a, cases):
        from mvsnet_amd.model import GRU_CELL_KEYS, wta_depth_values
        lib = L.load()
        self.a, self.cases = a, cases
        c0 = cases[0]
        gp, self.D, self.C = c0["gp"], c0["D"], c0["C"]
        _, self.H, self.W, _ = c0["features"].shape
        self.N = c0["features"].shape[0]
        self.params = [put(a, "%s.%s" % (cell, k), gp[cell][k]) for cell in ("gru1", "gru2", "gru3") for k in GRU_CELL_KEYS]
        self.params += [put(a, "prob_w", gp["prob_w"]), put(a, "prob_b", gp["prob_b"])]
        self.p_ptrs = L.ptr_array(self.params)
        self.filters = tuple(int(gp[c]["out_b"].shape[0]) for c in ("gru1", "gru2", "gru3"))
        self.T, self.dv = [], []
        for i, c in enumerate(cases):
            D = self.D
            if D == 1:
                interval, end, dv = 0.0, c["start"], np.asarray([c["start"]], np.float32)
            else:
                interval = float((np.float32(c["end"]) - np.float32(c["start"])) / (np.float32(D) - np.float32(1)))
                end, dv = c["end"], wta_depth_values(D, c["start"], c["end"], False)
            T = out(a, "transforms%d" % i, self.N - 1, D, 8)
            L.check(lib.mvs_homography_transforms_f32(L.ptr(put(a, "cams%d" % i, c["cams"])), self.N, D, float(c["start"]), interval,
                                                      float(end), 0, None, L.ptr(T), L.stream_ptr()), "mvs_homography_transforms_f32")
            self.T.append(T); self.dv.append(dv)
        self.ws_bytes = lib.mvs_gru_workspace_bytes(self.H, self.W, self.C, *self.filters) * len(cases)
        self.ws = a.take_bytes(self.ws_bytes, "workspace")

    @staticmethod
    def megabytes(cases):
        c = cases[0]
        _, H, W, Cc = c["features"].shape
        f = tuple(int(c["gp"][k]["out_b"].shape[0]) for k in ("gru1", "gru2", "gru3"))
        return 8 + len(cases) * (L.load().mvs_gru_workspace_bytes(H, W, Cc, *f) + 4 * H * W * Cc * 4) * 5 // 4 // (1 << 20)

    def features(self, feats, tag=""):
        return [(put(self.a, "ref%s%d" % (tag, i), f[0]), put(self.a, "src%s%d" % (tag, i), f[1:])) for i, f in enumerate(feats)]

    def __call__(self, feats, depth, prob):
        lib = L.load()
        f1, f2, f3 = self.filters
        flat = [float(x) for dv in self.dv for x in dv]
        dv = (C.c_float * len(flat))(*flat)
        if len(self.cases) == 1:
            L.check(lib.mvs_gru_wta_f32(L.ptr(feats[0][0]), L.ptr(feats[0][1]), L.ptr(self.T[0]), self.N, self.D, self.H, self.W, self.C,
                                        f1, f2, f3, self.p_ptrs, dv, vp(self.ws), self.ws.numel(), L.ptr(depth), L.ptr(prob),
                                        L.stream_ptr()), "mvs_gru_wta_f32")
        else:
            L.check(lib.mvs_gru_wta_batch_f32(L.ptr_array([f[0] for f in feats]), L.ptr_array([f[1] for f in feats]), L.ptr_array(self.T),
                                              len(self.cases), self.N, self.D, self.H, self.W, self.C, f1, f2, f3, self.p_ptrs, dv,
                                              vp(self.ws), self.ws.numel(), L.ptr(depth), L.ptr(prob), L.stream_ptr()),
                    "mvs_gru_wta_batch_f32")


def hold_sweep(pattern, H, W, D, views=(0,), form=0, impl="auto", tag="", **hooks):
    lib = L.load()
    cases = [SR.case("normal", H, W, D, v) for v in views]
    a = arena(pattern, SweepCall.megabytes(cases))
    call = SweepCall(a, cases)
    feats = call.features([c["features"] for c in cases])
    depth, prob = out(a, "depth", len(views), H, W), out(a, "prob", len(views), H, W)
    try:
        L.set_conv_impl(impl)
        L.check(lib.mvs_gru_set_formulation(form), "mvs_gru_set_formulation")
        with L.test_hooks(**hooks):
            call(feats, depth, prob)
            torch.cuda.synchronize()
    finally:
        L.check(lib.mvs_gru_set_formulation(0), "mvs_gru_set_formulation")
        L.set_conv_impl("auto")
    a.check()
    d, p = n(depth), n(prob)
    for i, v in enumerate(views):
        _c, ref = SR.case_scores("normal", H, W, D, v)
        SR.check_every_pixel(d[i], p[i], ref, "arena %s %dx%d D=%d view %d of %d" % (tag, H, W, D, v, len(views)))


SWEEP_ROUTES = [dict(form=0), dict(form=1), dict(form=2), dict(form=0, impl="scalar")]
SWEEP_IDS = ["fused", "wavefront1", "wavefront2", "scalar"]
# (27,41) and (9,47): partial tiles, a single tile row; (19,35) x 1: one plane; (21,37) x 19: a ragged depth (16 + 3 planes)
SWEEP_SHAPES = [(27, 41, 16), (9, 47, 16), (19, 35, 1), (21, 37, 19)]


@both_patterns
@pytest.mark.parametrize("route", SWEEP_ROUTES, ids=SWEEP_IDS)
@pytest.mark.parametrize("shape", SWEEP_SHAPES, ids=lambda s: "%dx%d-D%d" % s)
def test_gru_sweep(shape, route, pattern, stream_set):
    hold_sweep(pattern, *shape, tag=str(route), **route)


@both_patterns
@pytest.mark.parametrize("route", SWEEP_ROUTES, ids=SWEEP_IDS)
def test_gru_sweep_three_views(route, pattern, stream_set):
    hold_sweep(pattern, 27, 41, 16, views=(0, 1, 2), tag="3 views %s" % (route,), **route)


@functools.lru_cache(maxsize=None)
def toy_sweep_case(seed=0):
    """The toy workload as a sweep_reference-style case (its own cameras and depth range)."""
    w = S.make_workload("toy", seed=seed)
    gp = S.make_gru_params("normal", seed=2, in_channels=w.channels, random_affine=True)
    return dict(features=w.features, cams=w.cams, D=w.depth_num, start=w.depth_start, end=w.depth_end, gp=gp, C=w.channels)


def toy_scores(seed=0):
    c = toy_sweep_case(seed)
    return SR.plane_scores(c["features"], c["cams"], c["D"], c["start"], c["end"], c["gp"], False)


@both_patterns
@pytest.mark.parametrize("route", SWEEP_ROUTES, ids=SWEEP_IDS)
def test_gru_sweep_toy(route, pattern, stream_set):
    lib = L.load()
    case = toy_sweep_case()
    a = arena(pattern, SweepCall.megabytes([case]))
    call = SweepCall(a, [case])
    depth, prob = out(a, "depth", call.H, call.W), out(a, "prob", call.H, call.W)
    try:
        L.set_conv_impl(route.get("impl", "auto"))
        L.check(lib.mvs_gru_set_formulation(route["form"]), "mvs_gru_set_formulation")
        call(call.features([case["features"]]), depth, prob)
        torch.cuda.synchronize()
    finally:
        L.check(lib.mvs_gru_set_formulation(0), "mvs_gru_set_formulation")
        L.set_conv_impl("auto")
    a.check()
    SR.check_every_pixel(n(depth), n(prob), toy_scores(), "arena toy %s" % (route,))


# ==== 3. calls that follow each other =========================================================================================
def close_by_atomics(got, ref):
    """The project's bound for results that differ by the arrival order of float64 atomics: 2e-5 of the largest magnitude
    (test_gpu_parity.test_regnet_span_and_fused_pair_equal_the_plain_schedules).  NaN fails."""
    scale = float(np.abs(ref).max())
    assert scale > 0 and np.isfinite(ref).all()
    assert float(np.abs(got - ref).max()) <= 2e-5 * scale


def regnet_alone(pattern, params, cost):
    a = arena(pattern, regnet_mb(cost.shape[:3]))
    net = ArenaRegnet(a, params)
    reg = out(a, "reg", *cost.shape[:3])
    L.check(net.run("prepared", put(a, "cost", cost), a.take_bytes(net.ws_bytes(*cost.shape[:3]), "workspace"), reg), "regnet alone")
    got = n(reg)
    a.check()
    return got


@both_patterns
def test_regnet_two_inputs_back_to_back_through_one_workspace(pattern):
    shape = (32, 32, 64)
    params, cost_a, _ = regnet_case("normal", shape)
    cost_b = np.abs(np.random.RandomState(77).standard_normal(cost_a.shape)).astype(np.float32) * 1.5
    a = arena(pattern, regnet_mb(shape) + 20)
    net = ArenaRegnet(a, params)
    ws = a.take_bytes(net.ws_bytes(*shape), "workspace")
    da, db = put(a, "cost A", cost_a), put(a, "cost B", cost_b)
    ra, rb = out(a, "reg A", *shape), out(a, "reg B", *shape)
    L.check(net.run("prepared", da, ws, ra), "A")           # no synchronisation between the two calls
    L.check(net.run("prepared", db, ws, rb), "B")
    ra, rb = n(ra), n(rb)
    a.check()
    close_by_atomics(ra, regnet_alone(pattern, params, cost_a))
    close_by_atomics(rb, regnet_alone(pattern, params, cost_b))
    assert float(np.abs(ra - rb).max()) > 1e-2 * float(np.abs(ra).max())        # the two inputs really differ


@both_patterns
def test_depth_from_features_two_inputs_back_to_back_through_one_scratch(pattern):
    wa, rp, eda, epa = depth_case("small", 0)
    wb, _, edb, epb = depth_case("small", 5)
    a = arena(pattern, depth_mb(wa) + 8)
    call = DepthCall(a, ArenaRegnet(a, rp), wa)             # same cameras for both: one `cams` region
    fa, fb = put(a, "features A", wa.features), put(a, "features B", wb.features)
    H, W = wa.height, wa.width
    dA, pA, dB, pB = out(a, "depth A", H, W), out(a, "prob A", H, W), out(a, "depth B", H, W), out(a, "prob B", H, W)
    call(fa, dA, pA)
    call(fb, dB, pB)
    dA, pA, dB, pB = n(dA), n(pA), n(dB), n(pB)
    a.check()
    assert_depth(dA, pA, eda, epa)
    assert_depth(dB, pB, edb, epb)
    for w, d_pair, p_pair in ((wa, dA, pA), (wb, dB, pB)):                        # each alone in a fresh arena
        b = arena(pattern, depth_mb(w))
        alone = DepthCall(b, ArenaRegnet(b, rp), w)
        d1, p1 = out(b, "depth", H, W), out(b, "prob", H, W)
        alone(put(b, "features", w.features), d1, p1)
        d1, p1 = n(d1), n(p1)
        b.check()
        close_by_atomics(d_pair, d1)
        close_by_atomics(p_pair, p1)


@both_patterns
def test_gru_sweep_two_inputs_back_to_back_through_one_workspace(pattern, stream_set):
    ca, cb = toy_sweep_case(0), toy_sweep_case(5)
    a = arena(pattern, SweepCall.megabytes([ca]) + 4)
    call = SweepCall(a, [ca])                               # same cameras and depth range for both inputs
    fa, fb = call.features([ca["features"]], " A"), call.features([cb["features"]], " B")
    H, W = call.H, call.W
    dA, pA, dB, pB = out(a, "depth A", H, W), out(a, "prob A", H, W), out(a, "depth B", H, W), out(a, "prob B", H, W)
    call(fa, dA, pA)
    call(fb, dB, pB)
    dA, pA, dB, pB = n(dA), n(pA), n(dB), n(pB)
    a.check()
    SR.check_every_pixel(dA, pA, toy_scores(0), "arena toy A then B: A")
    SR.check_every_pixel(dB, pB, toy_scores(5), "arena toy A then B: B")
    for c, d_pair, p_pair in ((ca, dA, pA), (cb, dB, pB)):
        b = arena(pattern, SweepCall.megabytes([c]))
        alone = SweepCall(b, [c])
        d1, p1 = out(b, "depth", H, W), out(b, "prob", H, W)
        alone(alone.features([c["features"]]), d1, p1)
        d1, p1 = n(d1), n(p1)
        b.check()
        # the fused sweep gives the same bits every time (include/mvsnet_hip.h); the bound for reordered atomics holds a fortiori
        close_by_atomics(p_pair, p1)
        assert np.array_equal(d_pair, d1)


@both_patterns
def test_regnet_a_larger_shape_between_two_runs_of_a_smaller_one(pattern):
    small, large = (8, 16, 16), (40, 24, 48)
    params, cost_s, exp_s = regnet_case("normal", small)
    _, cost_l, exp_l = regnet_case("normal", large)
    a = arena(pattern, regnet_mb(large) + regnet_mb(small))
    net = ArenaRegnet(a, params)
    ws = a.take_bytes(net.ws_bytes(*large), "workspace")
    ds, dl = put(a, "cost small", cost_s), put(a, "cost large", cost_l)
    r1, r2, r3 = out(a, "reg 1", *small), out(a, "reg 2", *large), out(a, "reg 3", *small)
    need_s = net.ws_bytes(*small)
    L.check(net.run("prepared", ds, ws, r1, need_s), "small")
    L.check(net.run("prepared", dl, ws, r2), "large")
    L.check(net.run("prepared", ds, ws, r3, need_s), "small again")
    r1, r2, r3 = n(r1), n(r2), n(r3)
    a.check()
    assert rel_l1(r1, exp_s) < 2e-5 and rel_l1(r2, exp_l) < 2e-5
    close_by_atomics(r3, r1)


@both_patterns
def test_regnet_on_a_side_stream(pattern):
    shape = (32, 32, 64)
    params, cost, exp = regnet_case("normal", shape)
    here = regnet_alone(pattern, params, cost)
    a = arena(pattern, regnet_mb(shape))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net = ArenaRegnet(a, params)
        reg = out(a, "reg", *shape)
        L.check(net.run("prepared", put(a, "cost", cost), a.take_bytes(net.ws_bytes(*shape), "workspace"), reg), "side stream")
    side.synchronize()
    got = n(reg)
    a.check()
    close_by_atomics(got, here)
    assert rel_l1(got, exp) < 2e-5


# ==== 2-D towers ==============================================================================================================
def _gn_relu(x, gamma, beta, relu):
    y = O.group_norm_nhwc(x, gamma, beta, dtype=np.float64)
    return np.maximum(y, 0) if relu else y


# V,H,W,C1,C2,Cout,k,stride: test_gpu_unet.test_conv2d_gn_matches_oracle's list (the tile kernel's shapes, one and two sources) ...
TILE_CASES = [(2, 16, 32, 4, 0, 8, 3, 1), (1, 16, 32, 8, 0, 8, 3, 1), (2, 16, 16, 16, 0, 16, 3, 1), (1, 8, 16, 32, 0, 32, 3, 1),
              (1, 16, 32, 4, 0, 16, 3, 2), (2, 16, 32, 16, 0, 32, 3, 2), (1, 16, 32, 8, 0, 16, 5, 2), (1, 16, 32, 16, 0, 32, 5, 2),
              (1, 16, 16, 8, 8, 8, 3, 1), (2, 8, 16, 16, 16, 16, 3, 1), (1, 8, 16, 64, 64, 64, 3, 1), (1, 10, 20, 16, 0, 24, 3, 1)]
# ... and test_persistent_conv2d_gn_matches_oracle_and_the_tile_kernel's: every instance of the persistent kernel, ragged edges
PERSISTENT_CASES = [(3, 40, 72, 16, 0, 16, 3, 1), (2, 36, 100, 8, 8, 8, 3, 1), (3, 24, 40, 32, 0, 32, 3, 1), (5, 20, 36, 16, 16, 16, 3, 1),
                    (2, 44, 68, 8, 0, 8, 3, 1), (4, 8, 16, 16, 0, 16, 3, 1), (1, 50, 34, 32, 0, 32, 3, 1), (3, 40, 72, 16, 0, 32, 3, 2),
                    (2, 52, 68, 8, 0, 16, 5, 2), (3, 36, 44, 16, 0, 32, 5, 2), (2, 30, 42, 16, 0, 32, 3, 2)]


@functools.lru_cache(maxsize=None)
def conv2d_case(case):
    V, H, W, C1, C2, Cout, k, stride = case
    rs = np.random.RandomState(sum(case))
    x1 = rs.standard_normal((V, H, W, C1)).astype(np.float32) + 0.3
    x2 = (rs.standard_normal((V, H, W, C2)).astype(np.float32) - 0.2) if C2 else None
    w = (rs.standard_normal((k, k, C1 + C2, Cout)) / np.sqrt(k * k * (C1 + C2))).astype(np.float32)
    g1 = (1 + 0.3 * rs.standard_normal(C1)).astype(np.float32); b1 = (0.2 * rs.standard_normal(C1)).astype(np.float32)
    g2 = (1 + 0.3 * rs.standard_normal(max(C2, 1))).astype(np.float32); b2 = (0.2 * rs.standard_normal(max(C2, 1))).astype(np.float32)
    gn1 = C1 % 8 == 0
    exp = []
    for v in range(V):
        xin = _gn_relu(x1[v], g1, b1, True) if gn1 else x1[v].astype(np.float64)
        if C2:
            xin = np.concatenate([xin, _gn_relu(x2[v], g2, b2, False)], -1)          # second source: no ReLU (deconv_gn)
        exp.append(O.convnd_same(xin, w, stride, np.float64))
    return x1, x2, w, g1, b1, g2, b2, np.stack(exp)


def slot_sums(x, SL, rows):
    """Raw group sums of a 'producer' output spread over some of the SL partial rows: (V, C/8, SL, 2) float64."""
    V, Cn = x.shape[0], x.shape[-1]
    xs = x.reshape(V, -1, Cn // 8, 8).astype(np.float64)
    full = np.stack([xs.sum((1, 3)), (xs ** 2).sum((1, 3))], -1)
    o = np.zeros((V, Cn // 8, SL, 2))
    for r, share in rows:
        o[:, :, r % SL] += share * full
    return o


def check_conv2d_gn(case, pattern, **hooks):
    lib = L.load()
    V, H, W, C1, C2, Cout, k, stride = case
    x1, x2, w, g1, b1, g2, b2, exp = conv2d_case(case)
    gn1 = C1 % 8 == 0
    SL = lib.mvs_gn_stat_slots()
    a = arena(pattern, 16)
    s1 = put(a, "stats1", slot_sums(x1, SL, ((0, 0.5), (5, 0.25), (SL - 1, 0.25))), F64) if gn1 else None
    s2 = put(a, "stats2", slot_sums(x2, SL, ((1, 0.75), (SL - 2, 0.25))), F64) if C2 else None
    wp = out(a, "prepared", lib.mvs_conv2d_prepared_floats(k, C1, C2, Cout))          # exactly the queried size
    L.check(lib.mvs_conv2d_prepare_f32(L.ptr(put(a, "w", w)), k, C1, C2, Cout, L.ptr(wp), L.stream_ptr()), "mvs_conv2d_prepare_f32")
    Ho, Wo = -(-H // stride), -(-W // stride)
    y = out(a, "y", V, Ho, Wo, Cout)
    so = zeroed_f64(a, "stats_out", V, Cout // 8, SL, 2)
    P = lambda name, arr, on: L.ptr(put(a, name, arr)) if on else None
    with L.test_hooks(**hooks):
        L.check(lib.mvs_conv2d_gn_f32(L.ptr(put(a, "x1", x1)), L.ptr(s1), P("gamma1", g1, gn1), P("beta1", b1, gn1), C1, 1 if gn1 else 0,
                                      P("x2", x2, C2), L.ptr(s2), P("gamma2", g2, C2), P("beta2", b2, C2), C2, 0,
                                      L.ptr(wp), V, H, W, Cout, k, stride, L.ptr(y), L.ptr(so), L.stream_ptr()), "mvs_conv2d_gn_f32")
        torch.cuda.synchronize()
    got, got_s = n(y), n(so).sum(2)
    a.check()
    for v in range(V):
        np.testing.assert_allclose(got[v], exp[v], rtol=2e-4, atol=2e-4)
        es = exp[v].reshape(-1, Cout // 8, 8)
        np.testing.assert_allclose(got_s[v, :, 0], es.sum((0, 2)), rtol=1e-4, atol=5e-3)
        np.testing.assert_allclose(got_s[v, :, 1], (es ** 2).sum((0, 2)), rtol=1e-4, atol=5e-3)


@both_patterns
@pytest.mark.parametrize("persistent", [1, 0], ids=["persistent", "tile"])
@pytest.mark.parametrize("case", TILE_CASES + PERSISTENT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_gn(case, persistent, pattern):
    check_conv2d_gn(case, pattern, unet_persistent=persistent)


@both_patterns
@pytest.mark.parametrize("grid", [3, 8])
def test_conv2d_gn_persistent_ranges_across_views(grid, pattern):
    """MVS_HOOK_UNET_GRID: ranges of many tiles that cross view boundaries, and a launch where some workgroups get nothing;
    five views, two sources."""
    check_conv2d_gn(PERSISTENT_CASES[3], pattern, unet_grid=grid)


@functools.lru_cache(maxsize=None)
def deconv2d_case(case):
    V, H, W, Cin, Cout = case
    rs = np.random.RandomState(sum(case))
    x = rs.standard_normal((V, H, W, Cin)).astype(np.float32)
    w = (rs.standard_normal((3, 3, Cout, Cin)) / np.sqrt(9 * Cin)).astype(np.float32)
    g = (1 + 0.3 * rs.standard_normal(Cin)).astype(np.float32); b = (0.2 * rs.standard_normal(Cin)).astype(np.float32)
    exp = np.stack([O.convnd_transpose_same(_gn_relu(x[v], g, b, True), w, 2, np.float64) for v in range(V)])
    return x, w, g, b, exp


@both_patterns
@pytest.mark.parametrize("mfma", [False, True], ids=["valu", "mfma"])
@pytest.mark.parametrize("case", [(2, 8, 16, 16, 8), (1, 8, 8, 128, 64), (1, 16, 16, 32, 16), (1, 10, 12, 16, 8)],
                         ids=lambda c: "x".join(map(str, c)))
def test_deconv2d_gn(case, mfma, pattern):
    lib = L.load()
    V, H, W, Cin, Cout = case
    x, w, g, b, exp = deconv2d_case(case)
    SL = lib.mvs_gn_stat_slots()
    a = arena(pattern, 8)
    st = put(a, "stats", slot_sums(x, SL, ((3, 1.0),)), F64)
    y = out(a, "y", V, 2 * H, 2 * W, Cout)
    so = zeroed_f64(a, "stats_out", V, Cout // 8, SL, 2)
    dw = put(a, "w", w)
    wp = None
    if mfma:
        wp = out(a, "prepared", lib.mvs_deconv2d_prepared_floats(Cin, Cout))
        L.check(lib.mvs_deconv2d_prepare_f32(L.ptr(dw), Cin, Cout, L.ptr(wp), L.stream_ptr()), "mvs_deconv2d_prepare_f32")
    L.check(lib.mvs_deconv2d_gn_f32(L.ptr(put(a, "x", x)), L.ptr(st), L.ptr(put(a, "gamma", g)), L.ptr(put(a, "beta", b)), Cin, 1,
                                    L.ptr(dw), L.ptr(wp), V, H, W, Cout, L.ptr(y), L.ptr(so), L.stream_ptr()), "mvs_deconv2d_gn_f32")
    got, got_s = n(y), n(so).sum(2)
    a.check()
    for v in range(V):
        np.testing.assert_allclose(got[v], exp[v], rtol=2e-4, atol=2e-4)
        es = exp[v].reshape(-1, Cout // 8, 8)
        np.testing.assert_allclose(got_s[v, :, 0], es.sum((0, 2)), rtol=1e-4, atol=5e-3)
        np.testing.assert_allclose(got_s[v, :, 1], (es ** 2).sum((0, 2)), rtol=1e-4, atol=5e-3)


@both_patterns
def test_conv2d_prepare_dgrad_equals_prepare_of_the_flipped_kernel(pattern):
    """mvs_conv2d_prepare_dgrad_f32 into a buffer of exactly mvs_conv2d_prepared_floats(ks, cout_fwd, 0, cin_fwd): the same bits as
    mvs_conv2d_prepare_f32 of the kernel flipped along kh, kw with its channel axes swapped (include/mvsnet_hip.h)."""
    lib = L.load()
    k, cin, cout = 3, 16, 32
    w = np.random.RandomState(9).standard_normal((k, k, cin, cout)).astype(np.float32)
    a = arena(pattern, 4)
    nf = lib.mvs_conv2d_prepared_floats(k, cout, 0, cin)
    got, ref = out(a, "dgrad prepared", nf), out(a, "prepared of the flipped kernel", nf)
    L.check(lib.mvs_conv2d_prepare_dgrad_f32(L.ptr(put(a, "w", w)), k, cin, cout, L.ptr(got), L.stream_ptr()), "mvs_conv2d_prepare_dgrad_f32")
    flipped = np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))
    L.check(lib.mvs_conv2d_prepare_f32(L.ptr(put(a, "w flipped", flipped)), k, cout, 0, cin, L.ptr(ref), L.stream_ptr()), "mvs_conv2d_prepare_f32")
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


@both_patterns
@pytest.mark.parametrize("shape", [(3, 64, 80), (2, 6, 10), (5, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_center_images(shape, pattern):
    lib = L.load()
    V, H, W = shape
    rs = np.random.RandomState(H + W)
    u8 = (rs.rand(V, H, W, 3) * rs.choice([30, 255], (V, 1, 1, 3))).astype(np.uint8)
    u8[-1, ..., 1] = 77
    a = arena(pattern, 4)
    d = put(a, "images", u8, U8)
    y = out(a, "out4", V, H, W, 4)
    ws = a.take_bytes(lib.mvs_center_images_workspace_bytes(V), "workspace")
    L.check(lib.mvs_center_images_u8_f32(vp(d), V, H, W, L.ptr(y), vp(ws), L.stream_ptr()), "mvs_center_images_u8_f32")
    got = n(y)
    a.check()
    assert np.all(got[..., 3] == 0) and np.all(got[-1, ..., 1] == 0)
    for v in range(V):
        np.testing.assert_allclose(got[v, ..., :3], O.standardise_image(u8[v], np.float64), rtol=0, atol=2e-6)


# ==== training kernels that take scratch ======================================================================================
def d64(x, grad=False):
    return torch.tensor(np.asarray(x, np.float64)).requires_grad_(grad)


def rel_l1_64(a, b):
    a = np.asarray(a, np.float64)
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30)) if np.isfinite(a).all() else float("inf")


@both_patterns
@pytest.mark.parametrize("C_,H,W,relu", [(8, 24, 40, True), (16, 12, 20, False), (128, 4, 6, True)])
def test_group_norm_forward_and_backward(C_, H, W, relu, pattern):
    """mvs_gn_stats_f32 / mvs_gn_apply_f32 / mvs_gn_bwd_reduce_f32 / mvs_gn_bwd_apply_f32 with sums of exactly
    mvs_gn_bwd_sums_doubles(V, C): test_gpu_backward.test_hip_group_norm_matches_torch_autograd."""
    import torch.nn.functional as F
    lib = L.load()
    rs = np.random.RandomState(C_)
    V = 3
    x = (rs.randn(V, C_, H, W) * 1.3 + 0.2).astype(np.float32)
    gamma = (1.0 + 0.3 * rs.randn(C_)).astype(np.float32); beta = (0.2 * rs.randn(C_)).astype(np.float32)
    g = rs.randn(V, C_, H, W).astype(np.float32)
    xx, gg, bb = d64(x, True), d64(gamma, True), d64(beta, True)
    y64 = F.group_norm(xx, C_ // 8, gg, bb, eps=1e-5)
    if relu:
        y64 = F.relu(y64)
    (y64 * d64(g)).sum().backward()
    a = arena(pattern, 8)
    nhwc = lambda t_: np.ascontiguousarray(np.transpose(t_, (0, 2, 3, 1)))
    dx_, dg_, dgam, dbet = put(a, "x", nhwc(x)), put(a, "g", nhwc(g)), put(a, "gamma", gamma), put(a, "beta", beta)
    stats = zeroed_f64(a, "stats", V, 2, C_)
    y, dx = out(a, "y", V, H, W, C_), out(a, "dx", V, H, W, C_)
    sp = L.stream_ptr()
    L.check(lib.mvs_gn_stats_f32(L.ptr(dx_), V, H * W, C_, L.ptr(stats), sp), "mvs_gn_stats_f32")
    L.check(lib.mvs_gn_apply_f32(L.ptr(dx_), L.ptr(stats), L.ptr(dgam), L.ptr(dbet), 1e-5, int(relu), V, H * W, C_, L.ptr(y), sp), "mvs_gn_apply_f32")
    sums = zeroed_f64(a, "sums", lib.mvs_gn_bwd_sums_doubles(V, C_))
    L.check(lib.mvs_gn_bwd_reduce_f32(L.ptr(dx_), L.ptr(stats), L.ptr(dgam), L.ptr(dbet), 1e-5, int(relu), L.ptr(dg_), V, H * W, C_,
                                      L.ptr(sums), sp), "mvs_gn_bwd_reduce_f32")
    L.check(lib.mvs_gn_bwd_apply_f32(L.ptr(dx_), L.ptr(stats), L.ptr(dgam), L.ptr(dbet), 1e-5, int(relu), L.ptr(dg_), L.ptr(sums),
                                     V, H * W, C_, L.ptr(dx), sp), "mvs_gn_bwd_apply_f32")
    tot = n(sums).reshape(-1, 2, C_).sum(0)
    got_y, got_dx = n(y), n(dx)
    a.check()
    assert rel_l1_64(got_y, nhwc(y64.detach().numpy())) < 1e-6
    assert rel_l1_64(got_dx, nhwc(xx.grad.numpy())) < 1e-5
    assert rel_l1_64(tot[1].astype(np.float32), gg.grad.numpy()) < 1e-5
    assert rel_l1_64(tot[0].astype(np.float32), bb.grad.numpy()) < 1e-5


@both_patterns
@pytest.mark.parametrize("C_,two", [(8, True), (16, False), (64, True)])
def test_bn_relu_backward(C_, two, pattern):
    """test_gpu_backward.test_bn_relu_and_its_backward_match_autograd: mvs_bn_relu_f32, mvs_bn_bwd_reduce_f32 / _apply_f32."""
    import torch.nn.functional as F
    lib = L.load()
    rs = np.random.RandomState(C_)
    shape = (6, 10, 12, C_)
    y = rs.randn(*shape).astype(np.float32) * 1.5 + 0.3
    gamma = (1.0 + 0.3 * rs.randn(C_)).astype(np.float32); beta = (0.2 * rs.randn(C_)).astype(np.float32)
    g1 = rs.randn(*shape).astype(np.float32)
    g2 = rs.randn(*shape).astype(np.float32) if two else None
    yy, gg, bb = d64(y, True), d64(gamma, True), d64(beta, True)
    act = F.relu(F.batch_norm(yy.permute(3, 0, 1, 2)[None], None, None, gg, bb, training=True, eps=1e-5))[0].permute(1, 2, 3, 0)
    ((act * (d64(g1) + (d64(g2) if two else 0.0))).sum()).backward()
    vox = y.size // C_
    y64 = y.astype(np.float64).reshape(-1, C_)
    a = arena(pattern, 8)
    dy, dgam = put(a, "y", y), put(a, "gamma", gamma)
    stats = put(a, "stats", np.stack([y64.sum(0), (y64 ** 2).sum(0)]), F64)          # as the conv kernels emit them
    scale, shift = out(a, "scale", C_), out(a, "shift", C_)
    sp = L.stream_ptr()
    L.check(lib.mvs_bn_finalize_f32(L.ptr(stats), C_, float(vox), L.ptr(dgam), L.ptr(put(a, "beta", beta)), BN_EPSILON, L.ptr(scale),
                                    L.ptr(shift), sp), "mvs_bn_finalize_f32")
    fwd = out(a, "bn_relu", *shape)
    L.check(lib.mvs_bn_relu_f32(L.ptr(dy), L.ptr(scale), L.ptr(shift), None, None, None, vox, C_, L.ptr(fwd), sp), "mvs_bn_relu_f32")
    d1, d2 = put(a, "g1", g1), (put(a, "g2", g2) if two else None)
    sums = zeroed_f64(a, "sums", lib.mvs_bn_bwd_sum_slots(), 2, C_)
    L.check(lib.mvs_bn_bwd_reduce_f32(L.ptr(dy), L.ptr(stats), float(vox), BN_EPSILON, L.ptr(scale), L.ptr(shift), L.ptr(d1), L.ptr(d2),
                                      vox, C_, L.ptr(sums), sp), "mvs_bn_bwd_reduce_f32")
    g_y, g_gamma, g_beta = out(a, "g_y", *shape), out(a, "g_gamma", C_), out(a, "g_beta", C_)
    L.check(lib.mvs_bn_bwd_apply_f32(L.ptr(dy), L.ptr(stats), float(vox), BN_EPSILON, L.ptr(scale), L.ptr(shift), L.ptr(dgam), L.ptr(d1),
                                     L.ptr(d2), L.ptr(sums), vox, C_, L.ptr(g_y), L.ptr(g_gamma), L.ptr(g_beta), sp), "mvs_bn_bwd_apply_f32")
    got = [n(fwd), n(g_y), n(g_gamma), n(g_beta)]
    a.check()
    assert rel_l1_64(got[0], act.detach().numpy()) < 1e-6
    assert rel_l1_64(got[1], yy.grad.numpy()) < 1e-5
    assert rel_l1_64(got[2], gg.grad.numpy()) < 1e-5
    assert rel_l1_64(got[3], bb.grad.numpy()) < 1e-5


@both_patterns
def test_softargmin_backward(pattern):
    """test_gpu_backward.test_softargmin_backward_matches_autograd, depth gradient only and with the probability map's."""
    from oracle import torch_grad as TG
    lib = L.load()
    rs = np.random.RandomState(0)
    D, H, W = 24, 9, 21
    reg = rs.randn(D, H, W).astype(np.float32)
    g = rs.randn(H, W).astype(np.float32)
    gp = rs.randn(H, W).astype(np.float32)
    x = d64(reg, True)
    (TG.soft_argmin(x, 425.0, 2.5) * d64(g)).sum().backward()
    x2 = d64(reg, True)
    P = torch.softmax(-x2, dim=0)
    depth = TG.soft_argmin(x2, 425.0, 2.5)
    idx = ((depth - 425.0) / 2.5).detach()
    l0 = idx.floor().long().clamp(0, D - 1); r0 = idx.ceil().long().clamp(0, D - 1)
    l1 = (l0 - 1).clamp(0, D - 1); r1 = (r0 + 1).clamp(0, D - 1)
    pick = lambda i: torch.gather(P, 0, i[None])[0]
    ((depth * d64(g)).sum() + ((pick(l0) + pick(r0) + pick(l1) + pick(r1)) * d64(gp)).sum()).backward()
    a = arena(pattern, 4)
    dreg, dg, dgp = put(a, "reg", reg), put(a, "g_depth", g), put(a, "g_prob", gp)
    o1, o2 = out(a, "g_reg depth only", D, H, W), out(a, "g_reg", D, H, W)
    L.check(lib.mvs_softargmin_bwd_f32(L.ptr(dreg), L.ptr(dg), None, D, H, W, 425.0, 2.5, 0, L.ptr(o1), L.stream_ptr()), "mvs_softargmin_bwd_f32")
    L.check(lib.mvs_softargmin_bwd_f32(L.ptr(dreg), L.ptr(dg), L.ptr(dgp), D, H, W, 425.0, 2.5, 0, L.ptr(o2), L.stream_ptr()), "mvs_softargmin_bwd_f32")
    got1, got2 = n(o1), n(o2)
    a.check()
    assert rel_l1_64(got1, x.grad.numpy()) < 1e-5
    assert rel_l1_64(got2, x2.grad.numpy()) < 1e-4


# (Cbig, Csmall, stride, kind): every layer shape of RegNetUS0 'normal' (test_gpu_backward.WGRAD_CASES), at its smaller volume
WGRAD_CASES = [(32, 8, 1, "conv"), (8, 32, 1, "conv"), (16, 16, 1, "conv"), (32, 32, 1, "conv"), (64, 64, 1, "conv"), (8, 1, 1, "conv"),
               (32, 16, 2, "conv"), (16, 32, 2, "conv"), (32, 64, 2, "conv"),
               (32, 64, 2, "deconv"), (16, 32, 2, "deconv"), (8, 16, 2, "deconv")]


@functools.lru_cache(maxsize=None)
def wgrad3d_case(cb, cs, stride, kind):
    from oracle import torch_grad as TG
    rs = np.random.RandomState(cb * 100 + cs + stride)
    D, H, W = 8, 8, 16
    big = rs.randn(D, H, W, cb).astype(np.float32)
    small = rs.randn(D // stride, H // stride, W // stride, cs).astype(np.float32)
    w = d64(np.zeros((3, 3, 3, cb, cs)), True)
    if kind == "conv":
        y = TG._conv(d64(big).permute(3, 0, 1, 2)[None], w, stride)[0].permute(1, 2, 3, 0)
        (y * d64(small)).sum().backward()
    else:
        y = TG._deconv(d64(small).permute(3, 0, 1, 2)[None], w)[0].permute(1, 2, 3, 0)
        (y * d64(big)).sum().backward()
    return big, small, w.grad.numpy()


@both_patterns
@pytest.mark.parametrize("cb,cs,stride,kind", WGRAD_CASES)
def test_conv3d_weight_gradient(cb, cs, stride, kind, pattern):
    lib = L.load()
    big, small, exp = wgrad3d_case(cb, cs, stride, kind)
    D, H, W = big.shape[:3]
    need = lib.mvs_conv3d_wgrad_workspace_bytes(D, H, W, cb, cs, stride)
    assert need > 0
    a = arena(pattern, 8 + (need >> 20))
    dw = out(a, "dw", 3, 3, 3, cb, cs)
    ws = a.take_bytes(need, "workspace")
    dbig, dsmall = put(a, "big", big), put(a, "small", small)
    assert lib.mvs_conv3d_wgrad_f32(L.ptr(dbig), L.ptr(dsmall), D, H, W, cb, cs, stride, vp(ws), need - 1, L.ptr(dw), L.stream_ptr()) \
        == MVS_E_WORKSPACE
    torch.cuda.synchronize()
    assert a.is_pattern(dw) and a.is_pattern(ws)           # one byte short: refused, nothing touched
    L.check(lib.mvs_conv3d_wgrad_f32(L.ptr(dbig), L.ptr(dsmall), D, H, W, cb, cs, stride, vp(ws), need, L.ptr(dw), L.stream_ptr()),
            "mvs_conv3d_wgrad_f32")
    got = n(dw)
    a.check()
    assert rel_l1_64(got, exp) < 2e-5


@both_patterns
@pytest.mark.parametrize("cin,cout,cg,off", [(32, 48, 48, 0), (16, 32, 48, 0), (16, 16, 48, 32), (32, 32, 32, 0), (32, 16, 20, 4),
                                             (16, 48, 48, 0)])
def test_conv2d_weight_gradient(cin, cout, cg, off, pattern):
    """test_gpu_backward.test_conv2d_weight_gradient_matches_autograd at its smallest ragged size (3 planes of 9 x 37)."""
    import torch.nn.functional as F
    lib = L.load()
    N, H, W = 3, 9, 37
    rs = np.random.RandomState(cin + cout + H)
    x = rs.randn(N, H, W, cin).astype(np.float32)
    g = rs.randn(N, H, W, cg).astype(np.float32)
    w64 = torch.zeros((3, 3, cin, cout), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(d64(x).permute(0, 3, 1, 2), w64.permute(3, 2, 0, 1), padding=1)
    (y * d64(g[..., off:off + cout]).permute(0, 3, 1, 2)).sum().backward()
    need = lib.mvs_conv2d_wgrad_workspace_bytes(N, H, W, cin, cout)
    a = arena(pattern, 8 + (need >> 20))
    dw = out(a, "dw", 3, 3, cin, cout)
    ws = a.take_bytes(need, "workspace")
    L.check(lib.mvs_conv2d_wgrad_f32(L.ptr(put(a, "x", x)), L.ptr(put(a, "g", g)), cg, off, N, H, W, cin, cout, vp(ws), need, L.ptr(dw),
                                     L.stream_ptr()), "mvs_conv2d_wgrad_f32")
    got = n(dw)
    a.check()
    assert rel_l1_64(got, w64.grad.numpy()) < 2e-6


@functools.lru_cache(maxsize=None)
def cv_bwd_case(shape):
    from oracle import torch_grad as TG
    N, D, H, W, Cc = shape
    cams = S.make_cams(N, H, W, D)
    feats = S.make_features(N, H, W, Cc, seed=5)
    start, interval = float(cams[0, 1, 3, 0]), float(cams[0, 1, 3, 1])
    Hs = np.stack([O.get_homographies(cams[0], cams[v], D, start, interval, np.float32) for v in range(1, N)])
    t8 = O.homography_to_transform8(Hs, np.float32)
    rs = np.random.RandomState(3)
    g1 = rs.randn(D, H, W, Cc).astype(np.float32)
    g2 = rs.randn(*g1.shape).astype(np.float32)
    f = d64(feats, True)
    cost = TG.cost_volume(f, d64(t8)).permute(1, 2, 3, 0)
    (cost * (d64(g1) + d64(g2))).sum().backward()
    return feats, t8, g1, g2, f.grad.numpy()


@both_patterns
@pytest.mark.parametrize("method", ["gather", "scatter"])
@pytest.mark.parametrize("shape", [(3, 16, 16, 32, 32), (2, 8, 24, 24, 16)], ids=lambda s: "x".join(map(str, s)))
def test_cost_volume_backward(shape, method, pattern):
    """test_gpu_backward.test_cost_volume_backward_matches_autograd at its two smallest shapes (32 and 16 channels).  The gather
    route overwrites g_ref / g_src (they start as poison) and takes a workspace of exactly the queried size; the scatter route
    accumulates into gradients the caller zeroed."""
    lib = L.load()
    N, D, H, W, Cc = shape
    feats, t8, g1, g2, exp = cv_bwd_case(shape)
    need = lib.mvs_cost_volume_bwd_workspace_bytes(N, D, H, W, Cc)
    a = arena(pattern, 16 + (need >> 20))
    ref, src, T = put(a, "ref", feats[0]), put(a, "src", feats[1:]), put(a, "transforms", t8)
    d1, d2 = put(a, "g1", g1), put(a, "g2", g2)
    if method == "gather":
        g_ref, g_src = out(a, "g_ref", H, W, Cc), out(a, "g_src", N - 1, H, W, Cc)
        ws = a.take_bytes(need, "workspace")
        L.check(lib.mvs_cost_volume_bwd_gather_f32(L.ptr(ref), L.ptr(src), L.ptr(T), N, D, H, W, Cc, L.ptr(d1), L.ptr(d2), vp(ws), need,
                                                   L.ptr(g_ref), L.ptr(g_src), L.stream_ptr()), "mvs_cost_volume_bwd_gather_f32")
    else:
        g_ref = a.take((H, W, Cc), F32, data=np.zeros((H, W, Cc), np.float32), name="g_ref")
        g_src = a.take((N - 1, H, W, Cc), F32, data=np.zeros((N - 1, H, W, Cc), np.float32), name="g_src")
        L.check(lib.mvs_cost_volume_bwd_f32(L.ptr(ref), L.ptr(src), L.ptr(T), N, D, H, W, Cc, L.ptr(d1), L.ptr(d2), L.ptr(g_ref),
                                            L.ptr(g_src), L.stream_ptr()), "mvs_cost_volume_bwd_f32")
    got = np.concatenate([n(g_ref)[None], n(g_src)], 0)
    a.check()
    assert rel_l1_64(got, exp) < 1e-4
