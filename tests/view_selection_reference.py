"""Numpy restatement of the view selection of mvsnet_amd/select_views.py (the semantics in its docstring): the float32
statement of visibility, pair scores and depth ranges, a float64 twin of the visibility, the continuous acos / exp score the
weight table discretises, and the cameras the tests use."""
from __future__ import annotations

import functools

import numpy as np

from tests import fusion_reference as F
from tests import render_reference as R

TABLE = 8192


def weight_table(theta0=5.0, sigma1=1.0, sigma2=10.0):
    """T[k] = floor(65535 g(theta_k) + 1/2), theta_k = degrees(asin((k + 1/2) / 8192)), in float64."""
    theta = np.degrees(np.arcsin((np.arange(TABLE, dtype=np.float64) + 0.5) / TABLE))
    return np.floor(65535.0 * gauss(theta, theta0, sigma1, sigma2) + 0.5).astype(np.uint16)


def gauss(theta, theta0=5.0, sigma1=1.0, sigma2=10.0):
    sigma = np.where(theta <= theta0, sigma1, sigma2)
    return np.exp(-(theta - theta0) ** 2 / (2.0 * sigma ** 2))


def camera_centres(cams):
    """(V,3) float32: c_v = -R_v^T t_v in float64, rounded once."""
    cams = np.asarray(cams, np.float64)
    return np.stack([-(c[0][:3, :3].T @ c[0][:3, 3]) for c in cams]).astype(np.float32)


def depths(points, cams):
    """(n,V) float32: w of the float32 projection."""
    P = R.projection_tables(cams)
    with np.errstate(all="ignore"):
        return np.stack([R._project(P[v], points, np.float32)[2] for v in range(len(P))], 1)


def visibility(points, cams, H, W, min_depth=0.0, zbuf=None, z_rel=0.01, dtype=np.float32):
    """(n,V) bool.  zbuf None: frustum; else (V,H,W) float32 depth maps.  dtype=np.float64 is the twin: projection, division
    and rounding to a pixel in float64 (the depth comparison stays the float32 statement's)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    P = R.projection_tables(cams)
    tol = np.float32(1.0 + float(z_rel))
    out = np.zeros((len(points), len(P)), bool)
    for v in range(len(P)):
        with np.errstate(all="ignore"):
            u, vv, w = R._project(P[v], points, dtype)
            fx, fy = np.floor(u / w + dtype(0.5)), np.floor(vv / w + dtype(0.5))
            vis = np.isfinite(w) & (w > dtype(np.float32(min_depth))) & np.isfinite(fx) & np.isfinite(fy)
            vis &= (fx >= 0) & (fx <= dtype(W - 1)) & (fy >= 0) & (fy <= dtype(H - 1))
            if zbuf is not None:
                z = np.zeros(len(points), np.float32)
                z[vis] = np.asarray(zbuf, np.float32)[v, fy[vis].astype(np.int64), fx[vis].astype(np.int64)]
                vis &= (z > 0) & (w.astype(np.float32) <= z * tol)
        out[:, v] = vis
    return out


def zbuffer(points, cams, H, W, splat=0, occlusion=None, min_depth=0.0):
    return R.render(points, cams, H, W, splat=splat, min_depth=min_depth, occlusion=occlusion)[0]


def pack_mask(vis):
    """(n,V) bool -> (n, ceil(V/64)) uint64: view p is bit p % 64 of word p / 64."""
    n, V = vis.shape
    out = np.zeros((n, (V + 63) // 64), np.uint64)
    for p in range(V):
        out[:, p // 64] |= vis[:, p].astype(np.uint64) << np.uint64(p % 64)
    return out


def pair_terms(A, B, table):
    """T[k] per row of A = c_a - p and B = c_b - p (float32 (...,3)); 0 where dot <= 0 or k is not finite."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    sum3 = lambda X, Y: (X[..., 0] * Y[..., 0] + X[..., 1] * Y[..., 1]) + X[..., 2] * Y[..., 2]
    with np.errstate(all="ignore"):
        dot, na, nb = sum3(A, B), sum3(A, A), sum3(B, B)
        r = (dot * dot) / (na * nb)
        x = np.float32(1.0) - r
        x = np.where(x < 0, np.float32(0), x)
        f = np.floor(np.sqrt(x) * np.float32(8192.0))
        ok = (dot > 0) & np.isfinite(f)
    assert f.dtype == np.float32
    k = np.minimum(TABLE - 1, np.where(ok, f, 0)).astype(np.int64)
    return np.where(ok, np.asarray(table)[k].astype(np.int64), 0)


def pair_scores(points, vis, cams, table=None):
    """-> (score_sum, shared) (V,V) int64, symmetric, zero diagonals."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    table = weight_table() if table is None else table
    c = camera_centres(cams)
    V = len(c)
    score, shared = np.zeros((V, V), np.int64), np.zeros((V, V), np.int64)
    D = c[None, :, :] - points[:, None, :]                                   # (n,V,3) float32
    for a in range(V - 1):
        both = vis[:, a:a + 1] & vis[:, a + 1:]
        t = pair_terms(D[:, a:a + 1], D[:, a + 1:], table)
        shared[a, a + 1:] = both.sum(0)
        score[a, a + 1:] = np.where(both, t, 0).sum(0)
    return score + score.T, shared + shared.T


def continuous_scores(points, vis, cams, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """The formula the table discretises, in float64: sum over the shared points of g(acos(cos theta))."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    c = camera_centres(cams).astype(np.float64)
    V = len(c)
    out = np.zeros((V, V))
    for a in range(V):
        for b in range(a + 1, V):
            both = vis[:, a] & vis[:, b]
            A, B = c[a] - p[both], c[b] - p[both]
            cos = (A * B).sum(1) / np.sqrt((A * A).sum(1) * (B * B).sum(1))
            theta = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
            out[a, b] = out[b, a] = np.where(theta < 90.0, gauss(theta, theta0, sigma1, sigma2), 0.0).sum()
    return out


def depth_range(w, lo=1, hi=99):
    """(min_depth, max_depth) float32 over the visible points' w: the sorted values at m lo // 100 and min(m - 1, m hi // 100)."""
    w = np.sort(np.asarray(w, np.float32))
    m = len(w)
    if m == 0:
        return np.float32(0), np.float32(0)
    return w[(m * int(lo)) // 100], w[min(m - 1, (m * int(hi)) // 100)]


def depth_ranges(points, vis, cams, lo=1, hi=99):
    """(V,2) float32."""
    w = depths(points, cams)
    return np.array([depth_range(w[vis[:, v], v], lo, hi) for v in range(vis.shape[1])], np.float32).reshape(-1, 2)


def radix_select(w, rank):
    """The two-pass selection of the kernels on one view's values: histogram of the high 16 bits, then of the low 16 bits
    inside the bin that holds `rank` -> the float32 of that rank."""
    bits = np.asarray(w, np.float32).view(np.uint32)
    cum = np.cumsum(np.bincount(bits >> 16, minlength=65536))
    high = int(np.searchsorted(cum, rank, side="right"))
    inside = rank - (int(cum[high - 1]) if high else 0)
    low = int(np.searchsorted(np.cumsum(np.bincount(bits[(bits >> 16) == high] & 0xFFFF, minlength=65536)), inside, side="right"))
    return np.array([(high << 16) | low], np.uint32).view(np.float32)[0]


# ------------------------------------------------------------------------------------------------ cameras

def ring_cameras(V, H=40, W=48, f=40.0, radius=4.0, centre=(0.0, 0.0, 4.0)):
    """(V,2,4,4): cameras on a full ring around `centre` in the x-z plane, each a little higher than the last, looking at it."""
    centre = np.asarray(centre, np.float64)
    cams = np.zeros((V, 2, 4, 4))
    for i in range(V):
        th = 2.0 * np.pi * i / V
        C = centre + radius * np.array([np.sin(th), 0.3 * np.sin(3.0 * th + 0.2), -np.cos(th)])
        Rm = F._look_at(C, centre)
        cams[i, 0, :3, :3], cams[i, 0, :3, 3], cams[i, 0, 3, 3] = Rm, -Rm @ C, 1.0
        cams[i, 1, :3, :3] = [[f, 0, W / 2.0 + 0.1371], [0, f, H / 2.0 - 0.0613], [0, 0, 1.0]]
    return cams


@functools.lru_cache(maxsize=None)
def scene_cams(size):
    """The five-view sphere scene's cameras at (H, W)."""
    return R.scale_cams(R.scene_cloud()[1], 40, 48, size[0], size[1])
