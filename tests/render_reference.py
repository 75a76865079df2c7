"""Numpy restatement of the point-cloud rendering of mvsnet_amd/render.py (the semantics in its docstring): the float32
statement, vectorised with np.minimum.at on uint64 keys, a float64 twin that differs only in the projection's precision, the
occlusion filter, and the scenes the tests render."""
from __future__ import annotations

import functools

import numpy as np

from tests import fusion_reference as F

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def projection_tables(cams):
    """(V,3,4) float32: P_v = K_v [R_v | t_v] composed in float64, rounded once."""
    cams = np.asarray(cams, np.float64)
    return np.stack([c[1][:3, :3] @ c[0][:3, :4] for c in cams]).astype(np.float32)


def _project(P, pts, dtype):
    """(u, v, w) per point in `dtype`: r = ((P0 X + P1 Y) + P2 Z) + P3 per row, left to right, every step rounded."""
    P = np.asarray(P, np.float32).astype(dtype)
    X, Y, Z = (np.asarray(pts, np.float32)[:, k].astype(dtype) for k in range(3))
    return [((P[r, 0] * X + P[r, 1] * Y) + P[r, 2] * Z) + P[r, 3] for r in range(3)]


def render(points, cams, H, W, splat=0, min_depth=0.0, occlusion=None, dtype=np.float32):
    """-> (depth (V,H,W) float32, index (V,H,W) int32).  dtype=np.float64 is the twin: the projection, the division and the
    rounding to a pixel in float64; the key still holds float32(w), so the two differ only in which pixel a point lands on
    and in the last bit of its depth."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    P = projection_tables(cams)
    V = len(P)
    half = dtype(0.5)
    keys = np.full((V, H * W), EMPTY, np.uint64)
    idx = np.arange(n, dtype=np.uint64)
    for v in range(V):
        with np.errstate(all="ignore"):
            u, vv, w = _project(P[v], points, dtype)
            fx, fy = np.floor(u / w + half), np.floor(vv / w + half)
            w32 = w.astype(np.float32)
            cand = np.isfinite(w) & (w > dtype(np.float32(min_depth))) & np.isfinite(fx) & np.isfinite(fy)
            if dtype is not np.float32:
                cand &= np.isfinite(w32) & (w32 > 0)
        key = (w32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
        for dy in range(-splat, splat + 1):
            for dx in range(-splat, splat + 1):
                px, py = fx + dtype(dx), fy + dtype(dy)
                with np.errstate(invalid="ignore"):
                    ok = cand & (px >= 0) & (px <= dtype(W - 1)) & (py >= 0) & (py <= dtype(H - 1))
                pix = py[ok].astype(np.int64) * W + px[ok].astype(np.int64)
                np.minimum.at(keys[v], pix, key[ok])
    empty = keys == EMPTY
    depth = np.where(empty, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    index = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    depth, index = depth.reshape(V, H, W), index.reshape(V, H, W)
    if occlusion is not None:
        depth, index = occlusion_filter(depth, index, *occlusion)
    return depth, index


def occlusion_filter(raw, index, k, rel, count):
    """The hidden-point removal on a raw map (V,H,W): reads raw, writes copies."""
    raw = np.asarray(raw, np.float32)
    ratio = np.float32(1.0 - float(rel))
    V, H, W = raw.shape
    limit = raw * ratio                                                      # float32 product
    pad = np.zeros((V, H + 2 * k, W + 2 * k), np.float32)
    pad[:, k:k + H, k:k + W] = raw
    c = np.zeros((V, H, W), np.int64)
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            if dx == 0 and dy == 0:
                continue
            q = pad[:, k + dy:k + dy + H, k + dx:k + dx + W]
            c += (q > 0) & (q < limit)
    removed = (raw > 0) & (c >= count)
    return np.where(removed, np.float32(0), raw), np.where(removed, np.int32(-1), index).astype(np.int32)


# ------------------------------------------------------------------------------------------------ scenes

def backproject(cam, depth64):
    """Every pixel with depth > 0 of one view, back-projected in float64 -> (points (m,3) float64, pixel y W + x (m,))."""
    H, W = depth64.shape
    yy, xx = np.nonzero(depth64 > 0)
    return F._backproject(np.asarray(cam, np.float64), xx, yy, depth64[yy, xx].astype(np.float64)), yy * W + xx


def scale_cams(cams, H0, W0, H, W):
    """The cameras of an H0 x W0 scene for an H x W image of the same field of view: K's rows scaled."""
    out = np.array(cams, np.float64)
    out[:, 1, 0, :3] *= W / float(W0)
    out[:, 1, 1, :3] *= H / float(H0)
    return out


@functools.lru_cache(maxsize=None)
def scene(kind, V=5, H=40, W=48):
    return F.make_scene(kind, V=V, H=H, W=W)


@functools.lru_cache(maxsize=None)
def scene_cloud(kind="sphere", V=5, H=40, W=48):
    """Every valid pixel of every view of the scene, back-projected in float64 and stored as float32 -> (points, cams)."""
    sc = scene(kind, V, H, W)
    pts = [backproject(sc["cams"][v], sc["depths"][v].astype(np.float64))[0] for v in range(V)]
    return np.concatenate(pts).astype(np.float32), sc["cams"]


def identity_cam(H, W, f):
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[1, :3, :3] = [[f, 0, W / 2.0 + 0.1371], [0, f, H / 2.0 - 0.0613], [0, 0, 1.0]]
    return cam


TWO_LAYER_REMOVED = 203           # pixels the filter (1, 0.1, 2) removes from the two-layer case below


@functools.lru_cache(maxsize=None)
def two_layer(H=24, W=32, f=30.0, back=800.0, front=500.0):
    """One camera at identity.  The back layer is every pixel back-projected at depth `back`; the front layer is the pixels
    with (x + y) even and x < W/2 at depth `front`: a half-dense surface whose gaps show the layer behind it.
    -> (points float32 (back layer first), cams (1,2,4,4), front mask (H,W) bool)."""
    cam = identity_cam(H, W, f)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = ((xx + yy) % 2 == 0) & (xx < W // 2)
    b = F._backproject(cam, xx.reshape(-1), yy.reshape(-1), np.full(H * W, back))
    fr = F._backproject(cam, xx[mask], yy[mask], np.full(int(mask.sum()), front))
    return np.concatenate([b, fr]).astype(np.float32), cam[None], mask
