"""Numpy restatement of mvsnet_amd/mesh_simplify.py (the semantics in its docstring): vertex clustering on a uniform grid of
cells with exact integer means, on whole arrays.  It shares nothing with the kernels: np.unique finds the clusters and the
first face of every set of duplicates, np.add.at sums.  ``twin`` is the float64 twin: the same cell assignment, the mean of
the members' float64 coordinates."""
from __future__ import annotations

import functools

import numpy as np

from tests import mesh_clean_reference as MC
from tests import mesh_reference as M

QUANTUM = 2 ** 20
CELLS = 2 ** 21


def _arrays(vertices, faces):
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
    return v, f


def default_origin(vertices, n_faces=0):
    """The per-axis minimum over the vertices whose three coordinates are finite, as float32; zeros when there is none and no
    face either."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    finite = np.isfinite(v).all(1)
    if not finite.any():
        if n_faces > 0:
            raise ValueError("no vertex is finite")
        return np.zeros(3, np.float32)
    return v[finite].min(0)


def cells(vertices, cell, origin):
    """-> (clusterable (M,) bool, k (M,3) int64, key (M,) int64, q (M,3) int64, u (M,3) float64); k, key and q are 0 where the
    vertex is not clusterable."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    o, c = np.asarray(origin, np.float32).astype(np.float64), np.float64(np.float32(cell))
    with np.errstate(all="ignore"):
        u = (v.astype(np.float64) - o) / c
        kf = np.floor(u)
        ok = np.isfinite(v).all(1) & ((kf >= 0) & (kf <= CELLS - 1)).all(1)
        qf = np.floor((u - kf) * QUANTUM)
    k = np.where(ok[:, None], kf, 0).astype(np.int64)
    q = np.where(ok[:, None], qf, 0).astype(np.int64)
    assert ((q >= 0) & (q < QUANTUM)).all()
    return ok, k, k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42), q, u


def _clusters(v, f, cell, origin):
    ok, k, key, q, _ = cells(v, cell, origin)
    inside = ((f >= 0) & (f < len(v))).all(1)
    valid = inside.copy()
    valid[inside] = ok[f[inside]].all(1)
    used = np.zeros(len(v), bool)
    used[f[valid].reshape(-1)] = True
    keys, inverse = np.unique(key[used], return_inverse=True)
    cluster = np.full(len(v), -1, np.int64)
    cluster[used] = inverse.reshape(-1)
    return ok, valid, used, keys, cluster, q


def _grid(v, n_faces, cell, origin):
    return np.float32(cell), default_origin(v, n_faces) if origin is None else np.asarray(origin, np.float32).reshape(3)


def _positions(keys, cluster, used, q, cell, origin):
    """-> (n (K,) int64, positions (K,3) float32): a = S / (n 2^20); b = k + a; c = b cell; d = o + c; float32(d)."""
    K = len(keys)
    n = np.bincount(cluster[used], minlength=K).astype(np.int64)
    S = np.zeros((K, 3), np.int64)
    np.add.at(S, cluster[used], q[used])
    k = np.stack([keys & (CELLS - 1), (keys >> 21) & (CELLS - 1), keys >> 42], 1)
    a = S.astype(np.float64) / (n * QUANTUM).astype(np.float64)[:, None]
    b = k.astype(np.float64) + a
    c = b * np.float64(cell)
    d = origin.astype(np.float64) + c
    return n, d.astype(np.float32)


def simplify(vertices, colours, faces, cell, origin=None):
    """-> (vertices, colours or None, faces, report)."""
    v, f = _arrays(vertices, faces)
    cell, origin = _grid(v, len(f), cell, origin)
    ok, valid, used, keys, cluster, q = _clusters(v, f, cell, origin)
    K = len(keys)
    n, cv = _positions(keys, cluster, used, q, cell, origin)
    cc = None
    if colours is not None:
        C = np.zeros((K, 3), np.int64)
        np.add.at(C, cluster[used], np.asarray(colours, np.uint8).reshape(-1, 3).astype(np.int64)[used])
        cc = ((2 * C + n[:, None]) // (2 * n[:, None])).astype(np.uint8)

    index = np.nonzero(valid)[0]
    g = cluster[f[index]].reshape(-1, 3)
    degenerate = (g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2])
    index, g = index[~degenerate], g[~degenerate]
    _, first = np.unique(np.sort(g, 1), axis=0, return_index=True) if len(g) else (None, np.zeros(0, np.int64))
    first = np.sort(first)
    kept = g[first]
    vk = np.zeros(K, bool)
    vk[kept.reshape(-1)] = True
    new = np.cumsum(vk) - 1
    out_f = new[kept].astype(np.int32).reshape(-1, 3)
    report = {"vertices_in": int(len(v)), "vertices_out": int(vk.sum()), "faces_in": int(len(f)), "faces_out": int(len(out_f)),
              "clusters": int(K), "invalid_faces": int((~valid).sum()), "degenerate_faces": int(degenerate.sum()),
              "duplicate_faces": int(len(g) - len(first)), "unclusterable_vertices": int((~ok).sum()), "cell": float(cell),
              "origin": [float(x) for x in origin]}
    return cv[vk], None if cc is None else np.ascontiguousarray(cc[vk]), out_f, report


def twin(vertices, faces, cell, origin=None):
    """-> (mean (K,3) float64 of the members' coordinates per cluster, members (K,), bound (K,3) float64: the module docstring's
    bound on |position - mean|), for ALL clusters in ascending key order."""
    v, f = _arrays(vertices, faces)
    cell, origin = _grid(v, len(f), cell, origin)
    ok, valid, used, keys, cluster, q = _clusters(v, f, cell, origin)
    K = len(keys)
    n = np.bincount(cluster[used], minlength=K).astype(np.float64)
    s = np.zeros((K, 3), np.float64)
    np.add.at(s, cluster[used], v[used].astype(np.float64))
    big = np.zeros((K, 3), np.float64)
    np.maximum.at(big, cluster[used], np.abs(v[used].astype(np.float64)))
    mean = s / n[:, None]
    scale = np.abs(origin.astype(np.float64)) + big + np.float64(cell)
    bound = np.float64(cell) * 2.0 ** -20 + 2.0 ** -24 * scale + (n[:, None] + 8) * 2.0 ** -52 * scale
    return mean, n.astype(np.int64), bound


def all_clusters(vertices, colours, faces, cell, origin=None):
    """The positions of ALL clusters (also those no surviving face names), for the twin."""
    v, f = _arrays(vertices, faces)
    cell, origin = _grid(v, len(f), cell, origin)
    ok, valid, used, keys, cluster, q = _clusters(v, f, cell, origin)
    return _positions(keys, cluster, used, q, cell, origin)[1]


# ------------------------------------------------------------------------------------------------ the project's meshes

@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """mesh_reference.analytic_sphere extracted -> (vertices, faces); treat as read-only."""
    m = M.extract(M.analytic_sphere())
    return m["vertices"], m["faces"]


def voxels(mult, voxel):
    """cell = float32(mult * voxel), as the command lines form it."""
    return np.float32(float(mult) * float(voxel))


@functools.lru_cache(maxsize=None)
def scene_simplify(kind, noisy, mult, colour=True):
    v, c, f = MC.scene_mesh(kind, noisy)
    return simplify(v, c if colour else None, f, voxels(mult, M.SCENE_VOXEL), np.asarray(M.SCENE_ORIGIN, np.float32))


@functools.lru_cache(maxsize=None)
def sphere_simplify(mult):
    v, f = sphere_mesh()
    return simplify(v, None, f, voxels(mult, M.SPHERE_VOXEL), np.asarray(M.SPHERE_ORIGIN, np.float32))
