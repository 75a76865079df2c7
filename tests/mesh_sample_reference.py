"""Numpy restatement of mvsnet_amd/mesh_sample.py (the semantics in its docstring): surface samples of a triangle mesh, with
float64 arithmetic on whole arrays, integer quotas, np.cumsum and np.searchsorted.  It shares nothing with the kernels."""
from __future__ import annotations

import functools

import numpy as np

from tests import mesh_clean_reference as MC
from tests import mesh_simplify_reference as MS

MAX_FACES = 2 ** 26
SATURATED_AT = 2.0 ** 36
U64 = np.uint64


def _arrays(vertices, faces):
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
    return v, f


def _normals(a, b, c):
    """n = e1 x e2 and A2 = (nx nx + ny ny) + nz nz in float64; numpy rounds every array operation on its own."""
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    return n, (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]


def quota(vertices, faces, density):
    """-> (q (F,) int64, invalid (F,) bool, zero_area (F,) bool, saturated (F,) bool)."""
    v, f = _arrays(vertices, faces)
    density = np.float64(density)
    inside = ((f >= 0) & (f < len(v))).all(1)
    valid = inside.copy()
    valid[inside] = np.isfinite(v[f[inside]]).all((1, 2))
    q = np.zeros(len(f), np.int64)
    zero, saturated = np.zeros(len(f), bool), np.zeros(len(f), bool)
    idx = np.nonzero(valid)[0]
    tri = v[f[idx]].astype(np.float64)
    with np.errstate(all="ignore"):
        _, A2 = _normals(tri[:, 0], tri[:, 1], tri[:, 2])
        t = ((np.sqrt(A2) * 0.5) * density) * 65536.0
        zero[idx] = A2 == 0.0
        saturated[idx] = ~zero[idx] & ~(t < SATURATED_AT)
        ok = ~zero[idx] & ~saturated[idx]
        q[idx[ok]] = np.floor(t[ok]).astype(np.int64)
    return q, ~valid, zero, saturated


def counts(q):
    """-> (per-face sample counts (F,) int64, first sample of every face (F,) int64, N) by error diffusion."""
    I = np.cumsum(np.asarray(q, np.int64), dtype=np.int64)
    E = I - q
    first = E >> 16
    return (I >> 16) - first, first, int(I[-1] >> 16) if len(I) else 0


def mix(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, U64) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def weights(seed, n):
    """-> (w0, wu, wv) (n,) int64 in units of 2^-25 for the samples 0..n-1."""
    g = np.arange(n, dtype=U64)
    h = mix(mix(np.array([int(seed) & (2 ** 64 - 1)], U64)) ^ g)
    k1 = (h >> U64(40)).astype(np.int64)
    k2 = ((h >> U64(16)) & U64(0xFFFFFF)).astype(np.int64)
    fold = k1 + k2 >= 2 ** 24
    k1 = np.where(fold, 2 ** 24 - 1 - k1, k1)
    k2 = np.where(fold, 2 ** 24 - 1 - k2, k2)
    wu, wv = 2 * k1 + 1, 2 * k2 + 1
    return 2 ** 25 - wu - wv, wu, wv


def sample(vertices, colours, faces, density, seed=0, *, max_samples=2 ** 27):
    """-> dict(xyz (N,3) float32, face_index (N,) int32, normals (N,3) float32, colours (N,3) uint8 or None, counts (F,) int64,
    weights (w0, wu, wv), stats).  ValueError for a saturated face, more than 2^26 faces or more than max_samples samples."""
    v, f = _arrays(vertices, faces)
    if not (float(density) > 0 and np.isfinite(float(density))):
        raise ValueError("density must be positive and finite")
    if len(f) > MAX_FACES:
        raise ValueError("more than 2^26 faces")
    q, invalid, zero, saturated = quota(v, f, density)
    if saturated.any():
        raise ValueError("%d faces are saturated" % int(saturated.sum()))
    per_face, first, N = counts(q)
    if N > min(int(max_samples), 2 ** 31 - 1):
        raise ValueError("%d samples are more than max_samples" % N)
    I = np.cumsum(q, dtype=np.int64)
    g = np.arange(N, dtype=np.int64)
    face = np.searchsorted(I >> 16, g, side="right")                          # the first f with (I_f >> 16) > g
    assert np.array_equal(face, np.repeat(np.arange(len(f)), per_face))
    w0, wu, wv = weights(seed, N)
    tri = v[f[face]].astype(np.float64).reshape(N, 3, 3)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    u, w = (wu.astype(np.float64) * 2.0 ** -25)[:, None], (wv.astype(np.float64) * 2.0 ** -25)[:, None]
    xyz = ((a + u * (b - a)) + w * (c - a)).astype(np.float32)
    with np.errstate(all="ignore"):
        n, A2 = _normals(a, b, c)
        normals = (n / np.sqrt(A2)[:, None]).astype(np.float32)
    rgb = None
    if colours is not None:
        col = np.asarray(colours, np.uint8).reshape(-1, 3).astype(np.int64)[f[face]].reshape(N, 3, 3)
        rgb = ((w0[:, None] * col[:, 0] + wu[:, None] * col[:, 1] + wv[:, None] * col[:, 2] + 2 ** 24) >> 25).astype(np.uint8)
    total = int(q.sum())
    stats = {"faces": int(len(f)), "invalid": int(invalid.sum()), "zero_area": int(zero.sum()), "samples": N,
             "area": total / 65536.0 / float(density)}
    return {"xyz": xyz, "face_index": face.astype(np.int32), "normals": normals, "colours": rgb, "counts": per_face,
            "weights": (w0, wu, wv), "stats": stats}


def density_of(spacing):
    return 1.0 / (float(spacing) * float(spacing))


def plane_bound(vertices, faces, face_index):
    """The docstring's bound on the distance of a sample from its triangle's plane and beyond its edges, per sample."""
    v, f = _arrays(vertices, faces)
    s = np.abs(v[f[face_index]].astype(np.float64)).reshape(-1, 9).max(1)
    return np.sqrt(3.0) * s * (2.0 ** -24 + 2.0 ** -49)


# ------------------------------------------------------------------------------------------------ the project's meshes

@functools.lru_cache(maxsize=None)
def sphere_sample(spacing, seed=0, colour=False):
    v, f = MS.sphere_mesh()
    c = None
    if colour:
        c = np.random.RandomState(3).randint(0, 256, (len(v), 3)).astype(np.uint8)
    return sample(v, c, f, density_of(spacing), seed)


@functools.lru_cache(maxsize=None)
def scene_sample(kind, noisy, spacing, seed=0):
    v, c, f = MC.scene_mesh(kind, noisy)
    return sample(v, c, f, density_of(spacing), seed)
