"""The preconditions of tests/view_count_cases.py, on the CPU: what the GPU tests of tests/test_gpu_view_counts.py lean on so that
they cannot pass vacuously."""
import itertools

import numpy as np
import pytest

from tests import view_count_cases as V

H, W, D = 6, 10, 24                          # the size the GPU file runs band_case at


def test_band_shifts_are_quarter_pixels_with_24_different_integer_parts():
    sh = V.band_shifts(H, W)
    assert sh.shape == (V.BAND_PERIOD, 2)
    assert np.array_equal(sh * 4, np.round(sh * 4))
    assert len(set(V.band_integer_parts(H, W))) == V.BAND_PERIOD
    assert len(set(V.FRACTIONS)) == 12 and all(0 <= f < 1 for fr in V.FRACTIONS for f in fr)
    assert np.array_equal(np.floor(sh), np.array(V.band_integer_parts(H, W), np.float64))


@pytest.mark.parametrize("n_src", range(1, V.MAX_BAND_SRC + 1))
def test_band_case_views_differ_on_every_plane_and_visit_every_band(n_src):
    ref, src, T = V.band_case(n_src, H, W, 8, D)
    assert ref.dtype == src.dtype == T.dtype == np.float32
    assert src.shape == (n_src, H, W, 8) and T.shape == (n_src, D, 8)
    for a in (ref, src):
        assert np.array_equal(a, np.round(a)) and a.min() >= -4 and a.max() <= 4
    # pure translations
    assert np.all(T[..., [0, 4]] == 1) and not T[..., [1, 3, 6, 7]].any()
    sx, sy = T[..., 2].astype(np.float64), T[..., 5].astype(np.float64)
    assert np.array_equal(sx * 4, np.round(sx * 4)) and np.array_equal(sy * 4, np.round(sy * 4))
    ip = np.stack([np.floor(sx), np.floor(sy)], -1)
    fr = np.stack([sx, sy], -1) - ip
    for d in range(D):
        for a, b in itertools.combinations(range(n_src), 2):
            assert not np.array_equal(ip[a, d], ip[b, d]), (d, a, b)
            assert not np.array_equal(fr[a, d], fr[b, d]), (d, a, b)
    for v in range(n_src):
        seen = set()
        for d in range(D):
            seen |= V.bands_of_shift(sx[v, d], sy[v, d], H, W)
        assert seen == set(V.BANDS), (v, set(V.BANDS) - seen)
        assert {(300.0, -300.0), (-300.0, 300.0)} <= {(sx[v, d], sy[v, d]) for d in range(D)}


@pytest.mark.parametrize("C", [8, 32, 64])
def test_band_case_no_two_views_warp_to_the_same_image(C):
    """Float64 oracle.  Were two warped images of a plane equal, a kernel that blends one view's block with another view's weights
    could still produce that plane."""
    n_src = V.MAX_BAND_SRC
    warped = V.band_warped(n_src, H, W, C, D)
    assert warped.shape == (n_src, D, H, W, C)
    for d in range(D):
        for a, b in itertools.combinations(range(n_src), 2):
            assert not np.array_equal(warped[a, d], warped[b, d]), (d, a, b)
        assert sum(1 for v in range(n_src) if not warped[v, d].any()) <= 1, d
    # fewer views are the first views of more: same features per (n_src, C) seed aside, the shifts are shared
    for n in range(1, n_src):
        assert np.array_equal(V.band_case(n, H, W, C, D)[2], V.band_case(n_src, H, W, C, D)[2][:n])


@pytest.mark.parametrize("variant", ["mem", "eager"])
def test_band_case_is_exact_in_float32(variant):
    """The bound the GPU test takes from the border-band test (atol 2e-5) presumes exact products and sums; the float32 oracle,
    which divides where the kernel multiplies by a rounded reciprocal, stays 10x inside it at 10 views and 64 channels."""
    from oracle import mvsnet_oracle as O
    n_src, C = V.MAX_BAND_SRC, 64
    ref, src, T = V.band_case(n_src, H, W, C, D)
    exp = V.band_expected(n_src, H, W, C, D, variant)
    fn = O.variance_cost_mem if variant == "mem" else O.variance_cost_eager
    for d in range(D):
        w32 = [O.image_projective_transform_bilinear(src[v], T[v, d], np.float32) for v in range(n_src)]
        for v in range(n_src):
            assert np.array_equal(w32[v].astype(np.float64), V.band_warped(n_src, H, W, C, D)[v, d])
        assert np.abs(fn(ref, w32, n_src + 1, np.float32) - exp[d]).max() <= 2e-6


@pytest.mark.parametrize("shape", V.CAMERA_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("N", V.CAMERA_VIEW_COUNTS)
def test_camera_case_float32_oracle_is_inside_the_gpu_bounds(N, shape):
    """The GPU test holds the kernel to rel-L1 < 1e-5 and a share below 2e-3 of voxels off by more than 1e-4.  The float32 oracle on
    the same float32 transforms: rel-L1 at most 4.9e-7 and no such voxel, so the bounds leave the kernel 20x the reference's own
    rounding and not one tap flip is owed to the inputs."""
    Hh, Ww, C, Dd = shape
    c = V.camera_case(N, Hh, Ww, C, Dd)
    assert c["features"].shape == (N, Hh, Ww, C) and c["t8"].shape == (N - 1, Dd, 8) and c["interval"] == V.CAMERA_INTERVAL
    for variant in ("mem", "eager"):
        e64 = V.camera_expected(N, Hh, Ww, C, Dd, variant)
        e32 = V.camera_volume_f32(N, Hh, Ww, C, Dd, variant).astype(np.float64)
        rel = float(np.abs(e32 - e64).sum() / np.abs(e64).sum())
        worst = float(np.abs(e32 - e64).max())
        print("camera_case N=%d %s %s: float32 oracle rel-L1 %.3g, worst voxel %.3g" % (N, shape, variant, rel, worst))
        assert rel <= 4.9e-7
        assert worst <= 1e-4
    cov = V.camera_coverage(N, Hh, Ww, C, Dd)
    print("camera_case N=%d %s: coverage per view %s" % (N, shape, np.round(cov, 3)))
    assert cov.shape == (N - 1,) and cov.min() >= 0.85
