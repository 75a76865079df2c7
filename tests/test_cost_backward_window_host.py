"""The candidate window of the cost-volume backward's gather pass (cvb_pass2_kernel, backward.hip), restated in numpy float32 and
held against the true contributors under every camera family of tests/camera_families.py.  No GPU.

Pass 2 gives one lane a source pixel s and lets it look for the reference pixels that sampled s: it maps s, s + (1, 0) and
s + (0, 1) through the adjugate of the plane's homography, sizes a window round the image of s by those forward differences plus
half a pixel, clips it by the image, and tests every reference pixel in it with the forward map.  A contributor outside the
window is lost without a sign: the entry returns success and an incomplete gradient.  `window` below restates that arithmetic
line by line -- adjugate, three inverse maps, bx / by, the skip of planes that map s beyond 1e8, the ceil / floor bounds, the
whole row / column range where a half-width is not below the image extent (NaN and infinity included).

The TRUE contributors of (view, plane) are every (source pixel, reference pixel) pair in which the reference pixel's `warp_point`
cell -- floor of the sample point and its three neighbours -- touches the source pixel inside the image, zero-weight corners
included.

What this file is and is not: it MODELS the kernel's arithmetic in numpy float32 (no fused multiply-adds, numpy's division); it
does not prove the kernel.  It documents the bound the window rests on (the note on extreme minification in backward.hip), fails
without a GPU when the window arithmetic restated here stops covering a family, and must be kept in step with the kernel by hand;
tests/test_gpu_cost_backward_cameras.py holds the kernel itself to float64 under the same families.

Measured here (3 views, 24 x 32 pixels, 8 planes): in-image pairs over both source views, the largest half-width a source pixel
with contributors asks for, pairs the window misses, and pairs a window cut at 8 pixels -- the kernel's form before the image
bound -- would miss (below 8 pixels of half-width the cut changes nothing):

    family       pairs   half-width   missed   missed when cut at 8 pixels
    roll30       38084      1.98         0         0
    roll90       35904      1.55         0         0
    roll180      41376      1.57         0         0
    zoom0.5      49152      2.69         0         0
    zoom0.25     49152      4.92         0         0
    zoom2        12384      1.02         0         0
    zoom4         3072      0.76         0         0
    wide25       26840      1.81         0         0
    wide45        4728      2.38         0         0
    tilt20       24472      1.67         0         0
    random0      49152      3.53         0         0
    random1      48828      4.16         0         0
    random2      24302      1.63         0         0
    random3      18378      1.96         0         0
    zoom0.125    49152      9.35         0      1536   (0.18 % of the bilinear weight)
    zoom0.1      49152     11.84         0     16904   (7.93 % of the bilinear weight)
"""
import numpy as np
import pytest

from tests import camera_families as CF

N, H, W, D = 3, 24, 32, 8
MIN_PAIRS = 100
f32 = np.float32


def warp_point(t, x, y):
    """cost_volume_common.h warp_point on float32 arrays."""
    proj = t[6] * x + t[7] * y + f32(1.0)
    return (t[0] * x + t[1] * y + t[2]) / proj, (t[3] * x + t[4] * y + t[5]) / proj


def window(t, H, W, clamp=None):
    """cvb_pass2_kernel's candidate window of every source pixel for one (view, plane) transform t (8 float32):
    -> x_lo, x_hi, y_lo, y_hi (H, W) int arrays, skip (H, W) bool, bx, by (H, W) float32.
    `clamp`: cut bx, by at that many pixels first -- the form the kernel had before the window was bounded by the image alone."""
    t = np.asarray(t, f32)
    a0, a1, a2, b0, b1, b2, c0, c1 = t
    i00, i01, i02 = b1 - b2 * c1, a2 * c1 - a1, a1 * b2 - a2 * b1
    i10, i11, i12 = b2 * c0 - b0, a0 - a2 * c0, a2 * b0 - a0 * b2
    i20, i21, i22 = b0 * c1 - b1 * c0, a1 * c0 - a0 * c1, a0 * b1 - a1 * b0
    ys, xs = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")

    def inv_map(u, w_):
        q = f32(1.0) / (i20 * u + i21 * w_ + i22)
        return (i00 * u + i01 * w_ + i02) * q, (i10 * u + i11 * w_ + i12) * q

    with np.errstate(all="ignore"):
        px, py = inv_map(xs, ys)
        pxu, pyu = inv_map(xs + f32(1.0), ys)
        pxv, pyv = inv_map(xs, ys + f32(1.0))
        bx = np.abs(pxu - px) + np.abs(pxv - px) + f32(0.5)
        by = np.abs(pyu - py) + np.abs(pyv - py) + f32(0.5)
        if clamp is not None:
            bx = np.where(bx < f32(clamp), bx, f32(clamp)).astype(f32)
            by = np.where(by < f32(clamp), by, f32(clamp)).astype(f32)
        skip = ~(np.abs(px) < f32(1e8)) | ~(np.abs(py) < f32(1e8))
        okx, oky = (bx < f32(W)) & ~skip, (by < f32(H)) & ~skip
        safe = lambda v, ok: np.where(ok, v, f32(0.0))               # the kernel forms the ints only where they are finite
        x_lo = np.where(okx, np.maximum(0, np.ceil(safe(px - bx, okx)).astype(np.int64)), 0)
        x_hi = np.where(okx, np.minimum(W - 1, np.floor(safe(px + bx, okx)).astype(np.int64)), W - 1)
        y_lo = np.where(oky, np.maximum(0, np.ceil(safe(py - by, oky)).astype(np.int64)), 0)
        y_hi = np.where(oky, np.minimum(H - 1, np.floor(safe(py + by, oky)).astype(np.int64)), H - 1)
    assert x_lo.dtype.kind == "i" and bx.dtype == f32
    return x_lo, x_hi, y_lo, y_hi, skip, bx, by


def contributors(t, H, W):
    """-> (ys, xs, yr, xr, weight): every in-image (source pixel, reference pixel) pair of one transform and its bilinear weight."""
    t = np.asarray(t, f32)
    yr, xr = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    with np.errstate(all="ignore"):
        sx, sy = warp_point(t, xr, yr)
        x0, y0 = np.floor(sx), np.floor(sy)
        out = []
        for dy in (0, 1):
            for dx in (0, 1):
                xs, ys = x0 + f32(dx), y0 + f32(dy)
                ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)         # (NaN compares false)
                wx = (sx - x0) if dx else (x0 + f32(1.0) - sx)
                wy = (sy - y0) if dy else (y0 + f32(1.0) - sy)
                out.append((ys[ok].astype(np.int64), xs[ok].astype(np.int64), yr[ok].astype(np.int64), xr[ok].astype(np.int64),
                            (wx * wy)[ok].astype(np.float64)))
    return tuple(np.concatenate(c) for c in zip(*out))


def survey(t8, H, W, clamp=None):
    """Over all (view, plane) of t8 (V, D, 8): pairs per view, missed pairs, missed weight share, the largest half-width."""
    pairs, missed, w_all, w_missed, half = [], 0, 0.0, 0.0, 0.0
    for v in range(t8.shape[0]):
        count = 0
        for d in range(t8.shape[1]):
            x_lo, x_hi, y_lo, y_hi, skip, bx, by = window(t8[v, d], H, W, clamp)
            ys, xs, yr, xr, wgt = contributors(t8[v, d], H, W)
            seen = (~skip[ys, xs] & (xr >= x_lo[ys, xs]) & (xr <= x_hi[ys, xs]) & (yr >= y_lo[ys, xs]) & (yr <= y_hi[ys, xs]))
            count += ys.size
            missed += int((~seen).sum())
            w_all += float(wgt.sum()); w_missed += float(wgt[~seen].sum())
            asked = np.maximum(bx, by)[ys, xs]                         # at source pixels that HAVE contributors
            if asked.size:
                half = max(half, float(np.nanmax(np.where(np.isfinite(asked), asked, np.nan))))
        pairs.append(count)
    return dict(pairs=pairs, missed=missed, share=w_missed / max(w_all, 1e-30), half=half)


@pytest.fixture(scope="module")
def surveys():
    return {name: survey(CF.family_transforms(name, N, H, W, D), H, W) for name in CF.FAMILIES}


def test_the_families_are_the_sixteen_the_tests_run():
    assert set(CF.FAMILIES) == {"roll30", "roll90", "roll180", "zoom0.5", "zoom0.25", "zoom2", "zoom4", "wide25", "wide45", "tilt20",
                                "random0", "random1", "random2", "random3", "zoom0.125", "zoom0.1"}
    assert len(CF.FAMILIES) == 16
    base = CF.S.make_cams(N, H, W, D)
    for name in CF.FAMILIES:
        cams = CF.make_family_cams(name, N, H, W, D)
        assert np.array_equal(cams[0], base[0]), name                  # the reference view is make_cams' own
        assert not np.array_equal(cams[1:], base[1:]), name
        R = cams[1:, 0, :3, :3].astype(np.float64)
        assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-6), name


@pytest.mark.parametrize("name", CF.FAMILIES)
def test_the_window_misses_no_contributor(surveys, name):
    s = surveys[name]
    print("\n    %-10s %6d   %8.2f   %6d" % (name, sum(s["pairs"]), s["half"], s["missed"]))
    assert min(s["pairs"]) >= MIN_PAIRS, s["pairs"]
    assert s["missed"] == 0, s


def test_twelve_random_cameras_at_another_size_miss_no_contributor():
    """4 views, 6 planes, 40 x 56 pixels: the four families' seeds and eight more -- every seed from 0 that keeps 100 pairs in
    each view at this size (a property of the cameras alone), until twelve are found."""
    found, seed = 0, 0
    while found < 12 and seed < 200:
        s = survey(CF.family_transforms("random", 4, 40, 56, 6, seed=seed), 40, 56)
        if min(s["pairs"]) >= MIN_PAIRS:
            found += 1
            assert s["missed"] == 0, (seed, s)
        seed += 1
    assert found == 12


@pytest.mark.parametrize("name,pairs", [("zoom0.125", 1536), ("zoom0.1", 16904)])
def test_the_former_clamp_at_eight_pixels_drops_pairs_beyond_8x_minification(name, pairs):
    """Why the window is bounded by the image: with bx, by cut at 8 the same restatement loses these pairs (the counts a window of
    8 pixels drops at 24 x 32 x 8 planes), and loses none in any other family -- the clamp never helped, it only hid."""
    t8 = CF.family_transforms(name, N, H, W, D)
    s = survey(t8, H, W, clamp=8.0)
    print("\n    %s with the clamp: %d of %d pairs, %.2f %% of the weight, half-width asked %.2f"
          % (name, s["missed"], sum(s["pairs"]), 100 * s["share"], survey(t8, H, W)["half"]))
    assert s["missed"] == pairs
    assert survey(t8, H, W)["half"] > 8.0
