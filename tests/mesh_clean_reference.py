"""Numpy restatement of mvsnet_amd/mesh_clean.py (the semantics in its docstring): connected components of the face graph with
the component minima as labels, face counts and boxes per component, selection and compaction in input order.  The labelling
is hook-and-jump on whole arrays (every edge pulls both ends' labels down to the smaller, then labels jump to their labels'
labels, until nothing changes); it shares nothing with the kernels' union-find and nothing with scipy, against which
tests/test_mesh_clean_host.py checks it."""
from __future__ import annotations

import functools

import numpy as np

from tests import mesh_reference as M


def _arrays(vertices, faces):
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
    return v, f


def valid_faces(vertices, faces):
    """(F,) bool: the three indices lie in 0..M-1 and the nine coordinates are finite."""
    v, f = _arrays(vertices, faces)
    ok = ((f >= 0) & (f < len(v))).all(1)
    finite = np.isfinite(v).all(1)
    ok[ok] = finite[f[ok]].all(1)
    return ok


def vertex_labels(vertices, faces):
    """(M,) int64: the smallest vertex index of each vertex's component; two vertices are connected when a valid face names both."""
    v, f = _arrays(vertices, faces)
    label = np.arange(len(v), dtype=np.int64)
    g = f[valid_faces(v, f)].astype(np.int64)
    ea, eb = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    while True:
        before = label.copy()
        m = np.minimum(label[ea], label[eb])
        np.minimum.at(label, label[ea], m)
        np.minimum.at(label, label[eb], m)
        np.minimum.at(label, ea, m)
        np.minimum.at(label, eb, m)
        while True:
            jumped = label[label]
            if np.array_equal(jumped, label):
                break
            label = jumped
        if np.array_equal(label, before):
            return label


def extent2(lo, hi):
    """d2 = (ex ex + ey ey) + ez ez in float32, every operation rounded on its own."""
    lo, hi = np.asarray(lo, np.float32).reshape(-1, 3), np.asarray(hi, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        e = hi - lo
        return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def components(vertices, faces):
    """-> dict(face_labels (F,) int32, vertex_labels (M,) int32, labels (K,) int32 ascending, faces (K,) int32, lo (K,3), hi (K,3)
    float32, d2 (K,) float32, unreferenced, invalid, error_word = 0)."""
    v, f = _arrays(vertices, faces)
    ok = valid_faces(v, f)
    vl = vertex_labels(v, f)
    fl = np.full(len(f), -1, np.int64)
    fl[ok] = vl[f[ok, 0]]
    labels, counts = np.unique(fl[ok], return_counts=True)
    used = np.zeros(len(v), bool)
    used[f[ok].reshape(-1)] = True
    lo = np.full((len(v), 3), np.inf, np.float32)
    hi = np.full((len(v), 3), -np.inf, np.float32)
    np.minimum.at(lo, vl[used], v[used])
    np.maximum.at(hi, vl[used], v[used])
    lo, hi = lo[labels], hi[labels]
    return dict(face_labels=fl.astype(np.int32), vertex_labels=vl.astype(np.int32), labels=labels.astype(np.int32),
                faces=counts.astype(np.int32), lo=lo, hi=hi, d2=extent2(lo, hi), unreferenced=int((~used).sum()),
                invalid=int((~ok).sum()), error_word=0)


def rank(labels, counts):
    """The order by face count descending, then label ascending."""
    return np.lexsort((labels, -counts.astype(np.int64)))


def select(comp, min_faces=0, min_extent=0.0, keep_largest=0):
    """(K,) bool over comp['labels']."""
    thr = np.float32(min_extent) * np.float32(min_extent)
    with np.errstate(invalid="ignore"):
        keep = (comp["faces"].astype(np.int64) >= int(min_faces)) & (comp["d2"] >= thr)
    if keep_largest > 0:
        passing = np.nonzero(keep)[0]
        order = passing[rank(comp["labels"][passing], comp["faces"][passing])]
        keep = np.zeros(len(keep), bool)
        keep[order[:int(keep_largest)]] = True
    return keep


def clean(vertices, colours, faces, min_faces=0, min_extent=0.0, keep_largest=0):
    """-> (vertices, colours or None, faces, report)."""
    v, f = _arrays(vertices, faces)
    comp = components(v, f)
    keep = select(comp, min_faces, min_extent, keep_largest)
    kept_labels = comp["labels"][keep]
    fk = np.isin(comp["face_labels"], kept_labels) & (comp["face_labels"] >= 0)
    vk = np.zeros(len(v), bool)
    vk[f[fk].reshape(-1)] = True
    new = np.cumsum(vk) - 1
    out_f = new[f[fk]].astype(np.int32).reshape(-1, 3)
    out_v = v[vk]
    out_c = None if colours is None else np.ascontiguousarray(np.asarray(colours, np.uint8).reshape(-1, 3)[vk])
    order = rank(comp["labels"], comp["faces"])[:16]
    report = {"components": int(len(keep)), "components_kept": int(keep.sum()), "faces_in": int(len(f)), "faces_out": int(len(out_f)),
              "vertices_in": int(len(v)), "vertices_out": int(len(out_v)), "unreferenced": comp["unreferenced"],
              "invalid_faces": comp["invalid"], "error_word": 0,
              "largest": [[int(comp["labels"][i]), int(comp["faces"][i]), float(np.sqrt(np.float64(comp["d2"][i])))] for i in order]}
    return out_v, out_c, out_f, report


# ------------------------------------------------------------------------------------------------ built meshes

@functools.lru_cache(maxsize=None)
def strip(n_faces, seed, cuts=0):
    """A strip of n_faces triangles (i, i+1, i+2) on n_faces + 2 vertices with vertex numbering and face order permuted; with
    cuts, every face whose index is a multiple of n_faces // cuts is left out twice over (it and its successor), so the
    strip falls into pieces.  Treat as read-only."""
    rs = np.random.RandomState(seed)
    i = np.arange(n_faces)
    if cuts:
        step = n_faces // cuts
        i = i[(i % step > 1) | (i < 2)]
    number = rs.permutation(n_faces + 2)
    faces = number[np.stack([i, i + 1, i + 2], 1)][rs.permutation(len(i))].astype(np.int32)
    vertices = np.zeros((n_faces + 2, 3), np.float32)
    vertices[number] = np.stack([np.arange(n_faces + 2) * 0.5, np.arange(n_faces + 2) % 2, np.zeros(n_faces + 2)], 1)
    return vertices, faces


@functools.lru_cache(maxsize=None)
def grid(n, gap=0):
    """n x n quads on (n+1)^2 vertices, two triangles each; with gap, every gap-th row of quads is left out.  Treat as
    read-only."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    if gap:
        keep = (j % gap) != gap - 1
        j, i = j[keep], i[keep]
    a = (j * (n + 1) + i).reshape(-1)
    faces = np.stack([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)], 1).reshape(-1, 3).astype(np.int32)
    y, x = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    vertices = np.stack([x.reshape(-1) * 0.25, y.reshape(-1) * 0.25, np.sin(x.reshape(-1) * 0.1)], 1).astype(np.float32)
    return vertices, faces


# ------------------------------------------------------------------------------------------------ the six scene meshes

SCENES = [(kind, noisy) for kind in ("plane", "sphere", "step") for noisy in (False, True)]


@functools.lru_cache(maxsize=None)
def scene_mesh(kind, noisy=False):
    """The scene's depth maps through the probability filter alone (no consistency masks) into the standard volume, with
    colour -> (vertices, colours, faces); treat as read-only."""
    sc = M.scene(kind, noisy=noisy)
    vol = M.new_volume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, M.SCENE_TRUNC, colour=True)
    m = M.extract(M.integrate(vol, sc["depths"], sc["probs"], sc["cams"], sc["images"]))
    return m["vertices"], m["colours"], m["faces"]


@functools.lru_cache(maxsize=None)
def scene_clean(kind, noisy, min_faces=0, min_extent=0.0, keep_largest=0):
    return clean(*scene_mesh(kind, noisy), min_faces=min_faces, min_extent=min_extent, keep_largest=keep_largest)
