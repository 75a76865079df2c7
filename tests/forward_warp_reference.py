"""Float64 reference, per-voxel error unit and case table for the forward geometry path: mvs_homography_transforms_f32,
mvs_warp_f32 (zero fill) and mvs_cost_volume_f32.  A plain helper module (no fixtures, no GPU), in the manner of
tests/sweep_reference.py: tests/test_forward_warp_reference_host.py proves on the CPU that the float32 oracle stays inside the
rule on every case and that planted faults do not, tests/test_gpu_forward_cameras.py holds the device to it.

The rule.  For transforms T (float32 as given, evaluated in float64), per voxel and channel

    |got - ref64| <= BOUND * unit,            non-finite exactly where ref64 is non-finite (a 0 / 0 sample point), no voxel excluded.

Zero-filled bilinear sampling is continuous across tap boundaries, so a float32 sample point that lands in the neighbouring
block moves the value by (gradient x coordinate error) and no more; nothing needs an allowance for "tap flips".  With N views,
reference feature r, view v's float64 sample w_v, m_v the largest |tap| of its 2 x 2 block, mean = (r + sum w_v) / N:

    unit =  eps32 (r^2 + sum m_v^2) / N + eps32 (|r| + sum m_v)^2 / N^2                  rounding of blend and single-pass variance
          + sum_v 2 (|w_v - mean| + eps32 m_v) / N * (g_x,v d_x,v + g_y,v d_y,v + eps32 m_v)      sensitivity to the sample point
    d_x  =  eps32 ((|t0| x + |t1| y + |t2|) / |p| + |sx| (|t6| x + |t7| y + 1) / |p| + |sx|)      (d_y: t3, t4, t5 and sy)

g_x, g_y: the largest |difference| of horizontally / vertically adjacent taps over the block AND its neighbouring blocks (the
derivative jumps at a tap boundary).  mvs_warp_f32 has the one-view form eps32 m + g_x d_x + g_y d_y.  Both variance variants
share the unit (they are the same function in exact arithmetic).

BOUND is 3 x (MARGIN of tests/test_gpu_towers_backward.py) the worst ratio the float32 CPU oracle reaches over the whole case
table, rounded up; it is never taken from the device.  Measured (tests/test_forward_warp_reference_host.py prints them), worst
|f32 - f64| / unit over every voxel of every case of all_cases():

    float32 CPU oracle   cost volume, mem variant 0.93   eager variant 1.06 (zoom2-i26.5-N9)   warp, every plane of every view 0.48
    numpy copy of the sweep's block-and-weights scheme (reciprocal and multiply, clamped block, tap cache)   mem 1.04, eager 1.16
    (the prototype of the unit measured 1.33 on the families at C = 8; this table's worst is 1.06; 3 x either rounds up to 4.0)

Votes of the sweep kernel's wave tile (rows log2; `vote` restates the kernel's) at 3 views, 24 x 32, 8 planes, C = 32, the same
at both depth intervals:
    0   roll90 tilt20 random0 random1 random3        1   roll60        2   roll30
    3   roll180 zoom0.5 zoom0.25 zoom2 zoom4 wide25 wide45 random2 zoom0.125 zoom0.1
Samples travel at most 3.0 px over the 8 planes at interval 2.65 and up to 24.9 px at 26.5.

Far worlds on random0 (largest |T32 - T64| of the float32 oracle chain over the 8-vectors): 2.3e-6 at home, 4.4e-6 with the
world moved by 1e3 mm and 30 degrees, 1.9e-5 by 1e4 mm; the float64 8-vectors move by 8.9e-7 and 2.9e-5 (rounding of the moved
float32 cameras).

Measured on an MI355X (tests/test_gpu_forward_cameras.py), worst ratio per family over its cases:
    family            cost volume   warp    homographies (share of the entry's bound)
    roll30            0.82          0.33    0.53
    roll90            0.83          0.29    0.56
    roll180           0.66          0.21    0.34
    zoom0.5           0.42          0.31    0.58
    zoom0.25          0.33          0.28    0.33
    zoom2             1.06          0.32    0.65
    zoom4             0.87          0.15    0.62
    wide25            0.71          0.33    0.36
    wide45            0.87          0.26    0.52
    tilt20            0.79          0.35    0.55
    random0           0.30          0.27    0.76
    random1           0.42          0.26    0.43
    random2           0.86          0.23    0.46
    random3           0.83          0.25    0.49
    zoom0.125         0.30          0.31    0.33
    zoom0.1           0.47          0.29    0.33
    roll60            0.83          0.26    0.36
    hand-horizon      0.18          0.13    -
    hand-far_out      0.00          0.00    -
    hand-near_zero    0.14          0.09    -
    hand-exact_zero   0.11          0.06    -
    random0-far1000   -             -       0.42
    random0-far10000  -             -       0.42
    roll60-far10000   -             -       0.56
    worst: cost volume 1.06, warp 0.35 units (BOUND 4); homographies 0.76 of the bound; between the sweep and the per-plane kernel 0.88 units (2 BOUND = 8)
    features to depth roll90 one call: abs-rel 1.53e-07, prob share off by more than 1e-3: 0
    features to depth roll90 set_cameras + run_3dcnn: abs-rel 1.53e-07, prob share off by more than 1e-3: 0
    features to depth tilt20 one call: abs-rel 2.15e-07, prob share off by more than 1e-3: 0
    features to depth tilt20 set_cameras + run_3dcnn: abs-rel 2.15e-07, prob share off by more than 1e-3: 0
    features to depth random3 one call: abs-rel 2.36e-07, prob share off by more than 1e-3: 0
    features to depth random3 set_cameras + run_3dcnn: abs-rel 2.36e-07, prob share off by more than 1e-3: 0
    recurrent sweep roll90 fused: E = 1.03e-05  regret 0.000 E  prob 0.604 E  (16 x 27 x 41)
    recurrent sweep roll90 scalar: E = 1.03e-05  regret 0.000 E  prob 0.612 E  (16 x 27 x 41)
    recurrent sweep random3 fused: E = 1.04e-05  regret 0.000 E  prob 0.741 E  (16 x 27 x 41)
    recurrent sweep random3 scalar: E = 1.04e-05  regret 0.000 E  prob 0.722 E  (16 x 27 x 41)
"""
from __future__ import annotations

import collections
import functools

import numpy as np

from mvsnet_amd import synthetic as S
from oracle import mvsnet_oracle as O
from tests import camera_families as CF

EPS32 = float(np.finfo(np.float32).eps)        # 2^-23
MARGIN = 3.0
ORACLE_WORST = 1.06                            # the float32 CPU oracle's worst ratio over the case table (docstring)
BOUND = 4.0                                    # MARGIN x ORACLE_WORST, rounded up; also sweep_reference.BOUND

FAMILIES = CF.FAMILIES + ("roll60",)           # roll60 is the one family whose vote is 1; the backward tests keep CF.FAMILIES
INTERVALS = (2.65, 26.5)                       # samples travel up to 5 px / 27 px over the 8 planes
N, H, W, D, C = 3, 24, 32, 8, 32
f32 = np.float32


# ---- cameras ----------------------------------------------------------------------------------------------------------------
def family_cams(name, view_num=N, height=H, width=W, depth_num=D, interval=2.65):
    """CF.make_family_cams with another depth interval (make_cams' poses do not depend on it)."""
    cams = CF.make_family_cams(name, view_num, height, width, depth_num)
    cams[:, 1, 3, 1] = interval
    cams[:, 1, 3, 3] = cams[:, 1, 3, 0] + f32(interval) * depth_num
    return cams


def far_world(cams, shift, degrees):
    """Every camera's world frame moved by one rigid motion X' = G X: a rotation by `degrees` about each of x and y and a
    translation of `shift` mm along (0.6, -0.48, 0.64).  The homographies are unchanged in exact arithmetic; the float32 chain
    c = -R^T t, c_r - c_l now cancels numbers of the size of `shift`."""
    Rg = CF.rot("y", degrees) @ CF.rot("x", degrees)
    s = shift * np.array([0.6, -0.48, 0.64])
    out = np.asarray(cams, np.float64).copy()
    for v in range(out.shape[0]):
        R, t = out[v, 0, :3, :3].copy(), out[v, 0, :3, 3].copy()
        out[v, 0, :3, :3] = R @ Rg.T
        out[v, 0, :3, 3] = t - out[v, 0, :3, :3] @ s
    return out.astype(f32)


def cams_transforms(cams, depth_num, dtype=f32):
    """-> t8 (N - 1, D, 8) as tests/camera_families.family_transforms forms them (the float32 oracle chain)."""
    start, interval = float(cams[0, 1, 3, 0]), float(cams[0, 1, 3, 1])
    Hs = np.stack([O.get_homographies(cams[0], cams[v], depth_num, start, interval, dtype) for v in range(1, cams.shape[0])])
    return O.homography_to_transform8(Hs, dtype)


# ---- the float64 reference and the unit -------------------------------------------------------------------------------------
def sample_points(t8, height, width):
    """t8 (8,) -> proj, sx, sy, d_x, d_y (H, W) float64 (non-finite where proj is 0)."""
    t = np.asarray(t8, f32).astype(np.float64)
    x = np.arange(width, dtype=np.float64)[None, :]
    y = np.arange(height, dtype=np.float64)[:, None]
    a = np.abs(t)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = t[6] * x + t[7] * y + 1.0
        sx = (t[0] * x + t[1] * y + t[2]) / p
        sy = (t[3] * x + t[4] * y + t[5]) / p
        q = (a[6] * x + a[7] * y + 1.0) / np.abs(p)
        dx = EPS32 * ((a[0] * x + a[1] * y + a[2]) / np.abs(p) + np.abs(sx) * q + np.abs(sx))
        dy = EPS32 * ((a[3] * x + a[4] * y + a[5]) / np.abs(p) + np.abs(sy) * q + np.abs(sy))
    return p, sx, sy, dx, dy


def in_image(t8, height, width):
    """Number of pixels whose sample point has at least one tap inside the image."""
    _p, sx, sy, _dx, _dy = sample_points(t8, height, width)
    with np.errstate(invalid="ignore"):
        return int(((sx > -1) & (sx < width) & (sy > -1) & (sy < height)).sum())


PAD = 4


def warp64(image, t8):
    """image (H, W, C), t8 (8,) -> value, m, sens (H, W, C) float64: the zero-filled bilinear sample, the largest |tap| of its
    block, and g_x d_x + g_y d_y.  value is NaN where a coordinate is NaN (0 / 0) and 0 where one is +-inf."""
    img = np.asarray(image, np.float64)
    height, width, _ = img.shape
    _p, sx, sy, dx, dy = sample_points(t8, height, width)
    bad = np.isnan(sx) | np.isnan(sy)                           # 0 / 0: the voxel is NaN
    out = ~bad & (np.isinf(sx) | np.isinf(sy))                  # +-inf: outside the image like any other sample (include/mvsnet_hip.h)
    sxs, sys_ = np.where(bad | out, 0.0, sx), np.where(bad | out, 0.0, sy)
    x0, y0 = np.floor(sxs), np.floor(sys_)
    fx, fy = (sxs - x0)[..., None], (sys_ - y0)[..., None]
    # beyond these every tap of the 4 x 4 neighbourhood is outside the image
    xi = np.clip(x0, -3, width + 1).astype(np.int64)
    yi = np.clip(y0, -3, height + 1).astype(np.int64)
    pad = np.zeros((height + 2 * PAD, width + 2 * PAD, img.shape[2]))
    pad[PAD:-PAD, PAD:-PAD] = img
    nb = [[pad[yi + PAD - 1 + i, xi + PAD - 1 + j] for j in range(4)] for i in range(4)]
    value = (1 - fy) * ((1 - fx) * nb[1][1] + fx * nb[1][2]) + fy * ((1 - fx) * nb[2][1] + fx * nb[2][2])
    m = np.maximum(np.maximum(np.abs(nb[1][1]), np.abs(nb[1][2])), np.maximum(np.abs(nb[2][1]), np.abs(nb[2][2])))
    gx = functools.reduce(np.maximum, [np.abs(nb[i][j + 1] - nb[i][j]) for i in range(4) for j in range(3)])
    gy = functools.reduce(np.maximum, [np.abs(nb[i + 1][j] - nb[i][j]) for i in range(3) for j in range(4)])
    with np.errstate(invalid="ignore", over="ignore"):
        sens = np.where(gx > 0, gx * dx[..., None], 0.0) + np.where(gy > 0, gy * dy[..., None], 0.0)
    value[out] = 0.0; m[out] = 0.0; sens[out] = 0.0
    value[bad] = np.nan
    sens[bad] = np.nan
    return value, m, sens


def warp_reference(image, t8):
    """-> (ref64, unit) of mvs_warp_f32 with zero fill."""
    value, m, sens = warp64(image, t8)
    return value, EPS32 * m + sens


def volume_reference(features, T, negate=False):
    """features (N, H, W, C) float32, T (N - 1, D, 8) float32 -> (ref64, unit) (D, H, W, C) of either variance variant."""
    feats = np.asarray(features, np.float64)
    n_src, depth_num = T.shape[:2]
    n = n_src + 1
    r = feats[0]
    ref = np.empty((depth_num,) + r.shape)
    unit = np.empty_like(ref)
    for d in range(depth_num):
        views = [warp64(feats[v + 1], T[v, d]) for v in range(n_src)]
        s = r + sum(w for w, _m, _s in views)
        q = r * r + sum(w * w for w, _m, _s in views)
        mean = s / n
        ref[d] = q / n - mean * mean
        u = EPS32 * (r * r + sum(m * m for _w, m, _s in views)) / n + EPS32 * (np.abs(r) + sum(m for _w, m, _s in views)) ** 2 / n ** 2
        for w, m, sens in views:
            u = u + 2 * (np.abs(w - mean) + EPS32 * m) / n * (sens + EPS32 * m)
        unit[d] = u
    return (-ref if negate else ref), unit


def ratio(got, ref, unit):
    """|got - ref| / unit per voxel, 0 where both are non-finite or bit-equal, inf where only one is finite."""
    got = np.asarray(got, np.float64)
    fin_r, fin_g = np.isfinite(ref), np.isfinite(got)
    with np.errstate(invalid="ignore", divide="ignore"):
        diff = np.abs(got - ref)
        out = np.where(diff == 0, 0.0, diff / unit)
    out[~fin_r & ~fin_g] = 0.0
    out[fin_r != fin_g] = np.inf
    return out


def check_every_voxel(got, ref, unit, tag, bound=BOUND):
    """Every voxel: non-finite exactly where the reference is, |got - ref| <= bound * unit elsewhere.  Prints and returns the
    worst ratio."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    fin_r, fin_g = np.isfinite(ref), np.isfinite(got)
    rt = ratio(got, ref, unit)
    finite = np.where(np.isfinite(rt), rt, 0.0)
    worst = float(finite.max()) if finite.size else 0.0
    print("%s: worst %.3f units (median unit %.3g, %d non-finite voxel(s) in the reference)" % (
        tag, worst, float(np.nanmedian(unit)), int((~fin_r).sum())))
    if (fin_r != fin_g).any():
        at = tuple(np.argwhere(fin_r != fin_g)[0])
        raise AssertionError("%s: %d voxel(s) finite on one side only, first at %s: got %r, reference %r" % (
            tag, int((fin_r != fin_g).sum()), at, float(got[at]), float(ref[at])))
    at = np.unravel_index(rt.argmax(), rt.shape)
    assert rt.max() <= bound, "%s: %.3f units > %g at voxel %s (got %r, reference %r, unit %.3g; %d voxel(s) over)" % (
        tag, rt.max(), bound, at, float(got[at]), float(ref[at]), float(unit[at]), int((rt > bound).sum()))
    return worst


# ---- the float32 CPU oracle ----------------------------------------------------------------------------------------------------
def oracle_volume(features, T, variant="mem", negate=False, dtype=f32):
    feats = np.asarray(features, dtype)
    fn = O.variance_cost_mem if variant == "mem" else O.variance_cost_eager
    out = np.stack([fn(feats[0], [O.image_projective_transform_bilinear(feats[v + 1], T[v, d], dtype) for v in range(T.shape[0])],
                       T.shape[0] + 1, dtype) for d in range(T.shape[1])])
    return -out if negate else out


# ---- the sweep kernel restated --------------------------------------------------------------------------------------------------
def vote(T, height, width, channels):
    """cost_volume_sweep_kernel's vote of its wave tile: rows log2, 0..3, capped by the pixels a wave holds."""
    T = np.asarray(T, f32)
    cx, cy = f32(0.5) * f32(width), f32(0.5) * f32(height)
    mx = my = f32(0)
    for v in range(T.shape[0]):
        a, b = T[v, 0], T[v, -1]
        mx = mx + np.abs((b[0] - a[0]) * cx + (b[1] - a[1]) * cy + (b[2] - a[2]))
        my = my + np.abs((b[3] - a[3]) * cx + (b[4] - a[4]) * cy + (b[5] - a[5]))
    ty = 3 if mx >= 2 * my else 0 if my >= 2 * mx else 2 if mx >= my else 1
    ppw = 64 // (channels // 4)
    while (1 << ty) > ppw:
        ty -= 1
    return ty


def _cvt_i32(x):
    """v_cvt_i32_f32: saturates, NaN -> 0."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0, np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def sweep_scheme(features, T, variant="mem", fault=None):
    """A float32 numpy copy of cost_volume_sweep_kernel's per-(plane, view) bookkeeping and its register tap cache: reciprocal
    and multiply where the oracle divides, saturating conversion, the 2 x 2 block clamped into the image with the separable
    weights moved along, taps refetched only when the block's offset changes.  `fault` plants one defect:
      weights_x / weights_corner   weights not moved with a clamped block (x axis; only where both axes are clamped)
      stale_row                    the cache key ignores the block's row
      offset                       the sample point is off by 1e-3 px in x
      rcp18                        the reciprocal is good to 2^-18 only"""
    feats = np.asarray(features, f32)
    T = np.asarray(T, f32)
    n_src, depth_num = T.shape[:2]
    n = n_src + 1
    _, height, width, channels = feats.shape
    xf = np.arange(width, dtype=f32)[None, :]
    yf = np.arange(height, dtype=f32)[:, None]
    r = feats[0]
    cur = np.full((n_src, height, width), -1, np.int64)
    taps = np.zeros((n_src, 4, height, width, channels), f32)
    inv_n, inv_nn = f32(1) / f32(n), f32(1) / (f32(n) * f32(n))
    out = np.empty((depth_num, height, width, channels), f32)
    one, zero = f32(1), f32(0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for d in range(depth_num):
            s, q = r.copy(), r * r
            for v in range(n_src):
                t = T[v, d]
                proj = t[6] * xf + t[7] * yf + one
                inv = one / proj
                if fault == "rcp18":
                    inv = inv * f32(1 + 2.0 ** -18)
                sx = (t[0] * xf + t[1] * yf + t[2]) * inv
                sy = (t[3] * xf + t[4] * yf + t[5]) * inv
                if fault == "offset":
                    sx = sx + f32(1e-3)
                x0, y0 = np.floor(sx), np.floor(sy)
                ix0, iy0 = _cvt_i32(x0), _cvt_i32(y0)
                cb, rb = np.clip(ix0, 0, width - 2), np.clip(iy0, 0, height - 2)
                dx, dy = ix0 - cb, iy0 - rb
                fx1, fx0, fy1, fy0 = (x0 + one) - sx, sx - x0, (y0 + one) - sy, sy - y0
                zx = zy = zero                                           # literal zeros: a +-inf coordinate contributes 0
                ax = np.where(dx == 0, fx1, np.where(dx == -1, fx0, zx)); bx = np.where(dx == 0, fx0, np.where(dx == 1, fx1, zx))
                ay = np.where(dy == 0, fy1, np.where(dy == -1, fy0, zy)); by = np.where(dy == 0, fy0, np.where(dy == 1, fy1, zy))
                if fault in ("weights_x", "weights_corner"):
                    moved = (np.abs(dx) == 1) if fault == "weights_x" else ((np.abs(dx) == 1) & (np.abs(dy) == 1))
                    ax, bx = np.where(moved, fx1, ax), np.where(moved, fx0, bx)
                    if fault == "weights_corner":
                        ay, by = np.where(moved, fy1, ay), np.where(moved, fy0, by)
                key = cb if fault == "stale_row" else rb * width + cb
                move = key != cur[v]
                for k, (oy, ox) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    taps[v, k][move] = feats[v + 1][rb + oy, cb + ox][move]
                cur[v] = key
                w = ((ay * ax)[..., None] * taps[v, 0] + (ay * bx)[..., None] * taps[v, 1] + (by * ax)[..., None] * taps[v, 2]
                     + (by * bx)[..., None] * taps[v, 3])
                s = s + w
                q = q + w * w
            if variant == "mem":
                out[d] = q * inv_n - (s * s) * inv_nn
            else:
                mean = s * inv_n
                out[d] = q * inv_n - mean * mean
    return out


def swap_tile(volume, channels, ty_log2):
    """The volume as a sweep kernel would store it whose wave tile counts its pixel slots columns first while the tile shape
    `ty_log2` expects rows first: a permutation of the pixels inside every TY x TX tile (whole tiles only)."""
    ppw = 64 // (channels // 4)
    ty, tx = 1 << ty_log2, ppw >> ty_log2
    out = volume.copy()
    _, height, width, _ = volume.shape
    for y0 in range(0, height - ty + 1, ty):
        for x0 in range(0, width - tx + 1, tx):
            for slot in range(ppw):
                out[:, y0 + slot // tx, x0 + slot % tx] = volume[:, y0 + (slot & (ty - 1)), x0 + (slot >> ty_log2)]
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "tag kind name interval views height width planes channels")
VOTERS = (("roll90", 2.65), ("roll60", 2.65), ("roll30", 2.65), ("zoom2", 26.5))        # votes 0, 1, 2, 3 at C = 32
ROW_FAMILIES = (("zoom2", 2.65), ("wide25", 26.5), ("zoom0.5", 2.65))                   # keep their samples on a one-row image
FAR_WORLDS = ((1e3, 30.0), (1e4, 30.0))
HAND = ("horizon", "far_out", "near_zero", "exact_zero")
HAND_H, HAND_W = 12, 24


def _camera_case(name, interval, views=N, height=H, width=W, planes=D, channels=C, note=""):
    tag = "%s-i%g%s" % (name, interval, note)
    return Case(tag, "cams", name, interval, views, height, width, planes, channels)


def camera_cases():
    out = [_camera_case(nm, iv) for nm in FAMILIES for iv in INTERVALS]
    for nm, iv in VOTERS:
        out += [_camera_case(nm, iv, channels=c, note="-C%d" % c) for c in (8, 16, 64)]
        out.append(_camera_case(nm, iv, height=11, width=13, note="-11x13"))
        out += [_camera_case(nm, iv, views=n, note="-N%d" % n) for n in (2, 5, 8)]
        out.append(_camera_case(nm, iv, views=9, note="-N9"))                         # per-plane kernel: more than 8 views
        out.append(_camera_case(nm, iv, channels=12, note="-C12"))                    # per-plane kernel: 3 lanes per pixel
    out += [_camera_case(nm, iv, height=1, note="-1x32") for nm, iv in ROW_FAMILIES]  # per-plane kernel: H < 2
    out += [Case("random0-far%g" % sh, "far", "random0", 2.65, N, H, W, D, C) for sh, _deg in FAR_WORLDS]
    return out


def hand_cases(channels=16):
    return [Case("hand-%s-C%d" % (nm, channels), "hand", nm, 0.0, 4, HAND_H, HAND_W, 4, channels) for nm in HAND]


def all_cases():
    return camera_cases() + hand_cases(16) + hand_cases(12)


def hand_transforms(name):
    """(3, 4, 8) float32 on the 12 x 24 image: source views 0 and 2 are benign shifts by quarters of a pixel (exact blends of the
    integer features), view 1 is the named hard one -- a view that has left the image must not disturb the others.

      horizon     t6 = -1 / 10.5: proj changes sign between columns 10 and 11 (|proj| >= 0.047); samples reach tens of widths
      far_out     translations of +3e9 and -3e9 (beyond int32: the conversion saturates) and of 2^24 + 1 (x0 + 1 == x0)
      near_zero   proj = 2^-20 on column 8
      exact_zero  t6 = -0.125: proj is exactly 0 on column 8, with or without fma; planes 0, 1: non-zero numerators (the sample
                  is +-inf: the view contributes 0), planes 2, 3: both numerators 0 at that column too (0 / 0: NaN)"""
    T = np.zeros((3, 4, 8), f32)
    for d in range(4):
        T[0, d] = (1, 0, 0.25 * d - 0.5, 0, 1, 0.5 * d - 0.75, 0, 0)
        T[2, d] = (1, 0, -0.75 * d + 1.25, 0, 1, 0.25 * d, 0, 0)
    if name == "horizon":
        for d in range(4):
            T[1, d] = (2 + d, 0.25, 0.5, 0.125 * d, 1, 0.25 - d, -1 / 10.5, 0)
    elif name == "far_out":
        T[1, 0] = (1, 0, 3e9, 0, 1, 0.5, 0, 0)
        T[1, 1] = (1, 0, -3e9, 0, 1, -3e9, 0, 0)
        T[1, 2] = (1, 0, 2.0 ** 24 + 1, 0, 1, 0.25, 0, 0)
        T[1, 3] = (1, 0, 0.5, 0, 1, -(2.0 ** 24 + 1), 0, 0)
    elif name == "near_zero":
        for d in range(4):
            T[1, d] = (1, 0, 0.5 + d, 0, 1, 0.25 * d, -(1 - 2.0 ** -20) / 8, 0)
    elif name == "exact_zero":
        T[1, 0] = (1, 0, 0.5, 0, 1, 0.25, -0.125, 0)
        T[1, 1] = (-1, 0, 0.5, 0, -1, -0.25, -0.125, 0)
        T[1, 2] = (1, 0, -8, 0, 0, 0, -0.125, 0)
        T[1, 3] = (0.5, 0, -4, 0, 0, 0, -0.125, 0)
    else:
        raise KeyError(name)
    return T


Problem = collections.namedtuple("Problem", "case features T cams")


@functools.lru_cache(maxsize=None)
def problem(case):
    """-> Problem(case, features (N, H, W, C), T (N - 1, D, 8), cams or None), read-only, built once."""
    if case.kind == "hand":
        rs = np.random.RandomState(17)
        feats = rs.randint(-4, 5, size=(case.views, case.height, case.width, case.channels)).astype(f32)
        T, cams = hand_transforms(case.name), None
    else:
        cams = family_cams(case.name, case.views, case.height, case.width, case.planes, case.interval)
        if case.kind == "far":
            shift, degrees = FAR_WORLDS[[("random0-far%g" % sh) for sh, _ in FAR_WORLDS].index(case.tag)]
            cams = far_world(cams, shift, degrees)
        feats = S.make_features(case.views, case.height, case.width, case.channels, seed=5)
        T = cams_transforms(cams, case.planes)
    for a in (feats, T) + (() if cams is None else (cams,)):
        a.setflags(write=False)
    return Problem(case, feats, T, cams)


@functools.lru_cache(maxsize=None)
def reference(case):
    """-> (ref64, unit) of the case's cost volume, read-only, computed once and shared."""
    p = problem(case)
    ref, unit = volume_reference(p.features, p.T)
    ref.setflags(write=False); unit.setflags(write=False)
    return ref, unit


def takes_sweep(case):
    """mvs_cost_volume_f32's route for the case: the depth sweep (True) or the per-plane kernel."""
    cq = case.channels // 4
    return case.views <= 8 and cq <= 16 and cq & (cq - 1) == 0 and case.height >= 2 and case.width >= 2


# ---- homographies --------------------------------------------------------------------------------------------------------------
T_KINDS = (0, 0, 1, 0, 0, 1, 2, 2)             # entry of the 8-vector -> linear term, translation, projective term


def homography_reference(cams, depth_num, start, interval, end, inverse):
    """-> T64 (N-1, D, 8), H64 (N-1, D, 3, 3) of the float64 oracle on the float32 cameras, and per-entry bounds of the same
    shapes: MARGIN x the float32 oracle's largest distance from float64 among the entries of the same kind (linear terms,
    translations, projective terms; each row of H) for that view over the planes, with the floor 4 eps32 |entry|."""
    def chain(dtype):
        if inverse:
            Hs = [O.get_homographies_inv_depth(cams[0], cams[v], depth_num, start, end, dtype) for v in range(1, cams.shape[0])]
        else:
            Hs = [O.get_homographies(cams[0], cams[v], depth_num, start, interval, dtype) for v in range(1, cams.shape[0])]
        Hs = np.stack(Hs)
        return O.homography_to_transform8(Hs, dtype), Hs
    T64, H64 = chain(np.float64)
    T32, H32 = chain(f32)
    eT, eH = np.abs(T32 - T64), np.abs(H32 - H64)
    bT, bH = np.empty_like(T64), np.empty_like(H64)
    kinds = np.asarray(T_KINDS)
    for v in range(T64.shape[0]):
        for k in range(3):
            bT[v][:, kinds == k] = MARGIN * eT[v][:, kinds == k].max()
            bH[v][:, k, :] = MARGIN * eH[v][:, k, :].max()
    return T64, H64, np.maximum(bT, 4 * EPS32 * np.abs(T64)), np.maximum(bH, 4 * EPS32 * np.abs(H64)), float(eT.max())
