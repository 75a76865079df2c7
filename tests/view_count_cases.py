"""Inputs the view-count tests share (tests/test_view_count_cases_host.py on the CPU, tests/test_gpu_view_counts.py on the GPU): a plain
helper module, no fixtures.  The cost-volume launchers choose a kernel from the number of source views (cost_volume.hip: the
depth sweep is instantiated for 1..7 of them, its per-plane table grows a second quad of block offsets from 5 on, 8 and more go to
the per-plane kernel), so a test of them needs inputs on which a view that is paired with another view's block, weights or
offsets CANNOT give the right volume.  What makes that so is asserted on the CPU, in the host file:

band_case    integer features and pure translations on a quarter-pixel grid (every product exact in float32, as in
             test_gpu_parity.test_cost_volume_border_bands_are_exact).  On every plane the views' shifts differ pairwise in the
             integer part AND in the fraction, no two warped images are equal, and over the planes every view puts its 2x2
             block inside the image, in each one-pixel band, in each corner, two pixels out and 300 pixels out.
camera_case  S.make_cams / S.make_features at any view count; the float32 oracle's own distance from the float64 one is held to
             the bounds the GPU test uses, with room to spare.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S

# The 24 shifts of band_case, integer parts as functions of (H, W).  Entry i carries the fraction FRACTIONS[i % 12]; view v reads
# entry (d + v) % 24 on plane d, so the (at most 9) views of a plane hold 9 consecutive entries of the cycle: 24 different integer
# parts and fractions that repeat only 12 entries apart give every plane pairwise different ones.  Only entries 0 and 12 (300
# pixels out, both signs) warp to an all-zero image, and they never share a plane; every other entry leaves at least one pixel
# whose block touches the image.
FRACTIONS = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.25, 0.75), (0.75, 0.25), (0.5, 0.5), (0.25, 0.0), (0.0, 0.25), (0.75, 0.75),
             (0.25, 0.25), (0.5, 0.75), (0.75, 0.5)]
BAND_PERIOD = 24
MAX_BAND_SRC = 9


def band_integer_parts(H, W):
    return [(300, -300), (-1, 0), (0, -1), (-1, -1), (-2, 0), (0, -2), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W - 1, -1), (-1, H - 1),
            (1, 2), (-300, 300), (W - 2, H - 2), (-2, -2), (2, 1), (-1, 1), (1, -1), (W - 1, 1), (0, 0), (-3, H - 2), (W - 2, -2),
            (1, H - 1), (-2, 2)]


def band_shifts(H, W):
    """-> (24, 2) float64: (sx, sy) of every entry, exact multiples of 1/4."""
    return np.array([(ix + FRACTIONS[i % 12][0], iy + FRACTIONS[i % 12][1]) for i, (ix, iy) in enumerate(band_integer_parts(H, W))], np.float64)


def band_entry(d, v):
    return (d + v) % BAND_PERIOD


@functools.lru_cache(maxsize=None)
def band_case(n_src, H, W, C, D):
    """-> ref (H,W,C), src (n_src,H,W,C), T (n_src,D,8), all float32 and read-only."""
    if not 1 <= n_src <= MAX_BAND_SRC:
        raise ValueError("band_case holds 1..%d source views" % MAX_BAND_SRC)
    if H < 4 or W < 4:
        raise ValueError("band_case needs an image of at least 4 x 4")
    rs = np.random.RandomState(1000 * n_src + C)
    ref = rs.randint(-4, 5, size=(H, W, C)).astype(np.float32)
    src = rs.randint(-4, 5, size=(n_src, H, W, C)).astype(np.float32)
    sh = band_shifts(H, W)
    T = np.zeros((n_src, D, 8), np.float32)
    T[:, :, 0] = 1; T[:, :, 4] = 1
    for d in range(D):
        for v in range(n_src):
            T[v, d, 2], T[v, d, 5] = sh[band_entry(d, v)]
    for a in (ref, src, T):
        a.setflags(write=False)
    return ref, src, T


@functools.lru_cache(maxsize=None)
def band_warped(n_src, H, W, C, D):
    """-> (n_src, D, H, W, C) float64: every view's warped image on every plane (exact: quarter-pixel weights, small integers)."""
    _ref, src, T = band_case(n_src, H, W, C, D)
    out = np.stack([np.stack([O.image_projective_transform_bilinear(src[v], T[v, d].astype(np.float64), np.float64) for d in range(D)])
                    for v in range(n_src)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def band_expected(n_src, H, W, C, D, variant):
    """-> (D,H,W,C) float64 oracle volume of band_case."""
    ref, _src, _T = band_case(n_src, H, W, C, D)
    warped = band_warped(n_src, H, W, C, D)
    fn = O.variance_cost_mem if variant == "mem" else O.variance_cost_eager
    out = np.stack([fn(ref, [warped[v, d] for v in range(n_src)], n_src + 1, np.float64) for d in range(D)])
    out.setflags(write=False)
    return out


BANDS = ("inside", "left", "right", "top", "bottom", "top-left", "top-right", "bottom-left", "bottom-right", "two out", "far out")


def bands_of_shift(sx, sy, H, W):
    """The bands the top-left taps (x + floor(sx), y + floor(sy)) of the image's pixels fall into under the shift (sx, sy)."""
    ix0 = np.arange(W)[None, :] + int(np.floor(sx)) + np.zeros((H, 1), np.int64)
    iy0 = np.arange(H)[:, None] + int(np.floor(sy)) + np.zeros((1, W), np.int64)
    xin, yin = (ix0 >= 0) & (ix0 <= W - 2), (iy0 >= 0) & (iy0 <= H - 2)
    xl, xr, yt, yb = ix0 == -1, ix0 == W - 1, iy0 == -1, iy0 == H - 1
    found = {"inside": xin & yin, "left": xl & yin, "right": xr & yin, "top": yt & xin, "bottom": yb & xin,
             "top-left": xl & yt, "top-right": xr & yt, "bottom-left": xl & yb, "bottom-right": xr & yb,
             "two out": (ix0 == -2) | (ix0 == W) | (iy0 == -2) | (iy0 == H)}
    out = {k for k, m in found.items() if m.any()}
    if abs(sx) >= 300 and abs(sy) >= 300:
        out.add("far out")
    return out


# ---- cameras ------------------------------------------------------------------------------------------------------------------
CAMERA_INTERVAL = 30.0
CAMERA_VIEW_COUNTS = (2, 4, 6, 7, 8, 9, 10)
CAMERA_SHAPES = ((11, 13, 8, 12), (11, 13, 32, 12))          # (H, W, C, D) the GPU file runs, each at every view count


@functools.lru_cache(maxsize=None)
def camera_case(N, H, W, C, D):
    """-> dict(features (N,H,W,C), cams (N,2,4,4), t8 (N-1,D,8) float32, start, interval)."""
    cams = S.make_cams(N, H, W, D, interval=CAMERA_INTERVAL)
    feats = S.make_features(N, H, W, C)
    start, interval = float(cams[0, 1, 3, 0]), float(cams[0, 1, 3, 1])
    Hs = np.stack([O.get_homographies(cams[0], cams[v], D, start, interval, np.float32) for v in range(1, N)])
    t8 = O.homography_to_transform8(Hs, np.float32)
    for a in (cams, feats, t8):
        a.setflags(write=False)
    return dict(features=feats, cams=cams, t8=t8, start=start, interval=interval)


def _camera_volume(N, H, W, C, D, variant, dtype):
    c = camera_case(N, H, W, C, D)
    fn = O.variance_cost_mem if variant == "mem" else O.variance_cost_eager
    f, t8 = c["features"], c["t8"].astype(dtype)
    return np.stack([fn(f[0], [O.image_projective_transform_bilinear(f[v + 1], t8[v, d], dtype) for v in range(N - 1)], N, dtype)
                     for d in range(D)])


@functools.lru_cache(maxsize=None)
def camera_expected(N, H, W, C, D, variant="mem"):
    """-> (D,H,W,C) float64 oracle volume on the case's float32 transforms."""
    out = _camera_volume(N, H, W, C, D, variant, np.float64)
    out.setflags(write=False)
    return out


def camera_volume_f32(N, H, W, C, D, variant="mem"):
    return _camera_volume(N, H, W, C, D, variant, np.float32)


def camera_coverage(N, H, W, C, D):
    """-> (N-1,) per view: the share of (plane, pixel) whose 2x2 block touches the source image (-1 < sx < W and -1 < sy < H), that
    is, whose warped feature is not zero by construction."""
    t8 = camera_case(N, H, W, C, D)["t8"].astype(np.float64)
    xs, ys = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    out = []
    for v in range(N - 1):
        t = t8[v][:, :, None, None]
        proj = t[:, 6] * xs + t[:, 7] * ys + 1.0
        sx = (t[:, 0] * xs + t[:, 1] * ys + t[:, 2]) / proj
        sy = (t[:, 3] * xs + t[:, 4] * ys + t[:, 5]) / proj
        out.append(float(((sx > -1) & (sx < W) & (sy > -1) & (sy < H)).mean()))
    return np.array(out)
