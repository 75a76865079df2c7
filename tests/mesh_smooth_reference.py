"""Numpy restatement of mvsnet_amd/mesh_smooth.py (the semantics in its docstring): the six directed edge keys of every face,
their sort, the unique live keys as rows of neighbours with multiplicities, the class of every vertex, and Jacobi passes whose
float64 sums run over a vertex's neighbours in ascending order, one after the other.  Every intermediate array of the kernels
(keys, head, neighbours, row_start, vertex_class, each pass's Y) has its statement here; tests/test_mesh_smooth_host.py holds
them to facts.  It shares nothing with the kernels: the rows come from np.unique, the ordered sums from a loop over the k-th
neighbour of all vertices at once."""
from __future__ import annotations

import functools

import numpy as np

from tests.mesh_clean_reference import grid, strip  # noqa: F401  (the built meshes the smoothing tests share)

DEAD = np.int64(2 ** 63 - 1)
BOUNDARIES = ("fixed", "curve", "free")
FIXED, CURVE, INTERIOR = 0, 1, 2


def _arrays(vertices, faces):
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
    return v, f


def edge_keys(vertices, faces):
    """-> (keys (6 F,) int64 in the kernels' order a>b b>a b>c c>b c>a a>c per face, valid (F,) bool, finite (M,) bool)."""
    v, f = _arrays(vertices, faces)
    M = len(v)
    finite = np.isfinite(v).all(1)
    valid = ((f >= 0) & (f < M)).all(1)
    keys = np.full((len(f), 6), DEAD, np.int64)
    g = f[valid].astype(np.int64)
    for e, (s, t) in enumerate(((0, 1), (1, 0), (1, 2), (2, 1), (2, 0), (0, 2))):
        a, b = g[:, s], g[:, t]
        live = (a != b) & finite[a] & finite[b]
        keys[valid, e] = np.where(live, (a << 31) | b, DEAD)
    return keys.reshape(-1), valid, finite


def heads(sorted_keys):
    """head (E,) int32: 1 at the first key of each run of a live key."""
    s = np.asarray(sorted_keys, np.int64)
    return ((s != DEAD) & (np.concatenate([[-1], s[:-1]]) != s)).astype(np.int32)


def adjacency(vertices, faces, boundary="fixed"):
    """-> dict(keys, sorted_keys, head, head_rank, U, neighbours (U,) int32 with bit 31 on a boundary edge, row_start (M + 1,)
    int32, vertex_class (M,) uint8, targets, multiplicity (U,), and the counts of the report)."""
    v, f = _arrays(vertices, faces)
    M = len(v)
    keys, valid, finite = edge_keys(v, f)
    sorted_keys = np.sort(keys)
    head = heads(sorted_keys)
    unique, multiplicity = np.unique(sorted_keys[sorted_keys != DEAD], return_counts=True)
    source, target = unique >> 31, unique & (2 ** 31 - 1)
    on_boundary = multiplicity == 1
    neighbours = (target.astype(np.uint32) | (on_boundary.astype(np.uint32) << 31)).view(np.int32)
    row_start = np.searchsorted(source, np.arange(M + 1), side="left").astype(np.int32)
    degree = np.diff(row_start)
    boundary_vertex = np.zeros(M, bool)
    boundary_vertex[source[on_boundary]] = True
    cls = np.full(M, INTERIOR, np.uint8)
    if boundary == "curve":
        cls[boundary_vertex] = CURVE
    elif boundary == "fixed":
        cls[boundary_vertex] = FIXED
    else:
        assert boundary == "free", boundary
    cls[(degree == 0) | ~finite] = FIXED
    assert (degree[~finite] == 0).all()                                        # a vertex that is not finite has no live edge
    return dict(keys=keys, sorted_keys=sorted_keys, head=head, head_rank=np.cumsum(head).astype(np.int32), U=len(unique),
                neighbours=neighbours, row_start=row_start, vertex_class=cls, targets=target, multiplicity=multiplicity,
                invalid_faces=int((~valid).sum()), non_finite_vertices=int((~finite).sum()), edges=len(unique) // 2,
                boundary_edges=int((on_boundary & (source < target)).sum()),
                non_manifold_edges=int(((multiplicity >= 3) & (source < target)).sum()),
                boundary_vertices=int(boundary_vertex.sum()), fixed_vertices=int((cls == FIXED).sum()))


def one_pass(X, V0, adj, factor, r=None):
    """One Jacobi pass X -> Y with the float32 factor; r None or the float32 bound around V0."""
    X = np.asarray(X, np.float32)
    M = len(X)
    cls, row_start = adj["vertex_class"], adj["row_start"].astype(np.int64)
    target, flag = adj["targets"], adj["multiplicity"] == 1
    s = np.zeros((M, 3), np.float64)
    n = np.zeros(M, np.int64)
    degree = np.diff(row_start)
    Xd = X.astype(np.float64)
    for k in range(int(degree.max()) if M else 0):                             # the k-th neighbour of every vertex that has one
        rows = np.nonzero((degree > k) & (cls != FIXED))[0]
        e = row_start[rows] + k
        use = (cls[rows] != CURVE) | flag[e]
        rows, e = rows[use], e[use]
        s[rows] = s[rows] + Xd[target[e]]
        n[rows] += 1
    Y = X.copy()
    move = np.nonzero((cls != FIXED) & (n > 0))[0]
    with np.errstate(over="ignore", invalid="ignore"):
        m = s[move] / n[move, None].astype(np.float64)
        d = m - Xd[move]
        e = np.float64(np.float32(factor)) * d
        y = Xd[move] + e
        if r is not None:
            lo = np.asarray(V0, np.float32)[move].astype(np.float64) - np.float64(np.float32(r))
            hi = np.asarray(V0, np.float32)[move].astype(np.float64) + np.float64(np.float32(r))
            y = np.minimum(np.maximum(y, lo), hi)
        y32 = y.astype(np.float32)
    ok = np.isfinite(y32).all(1)
    Y[move[ok]] = y32[ok]
    return Y


def passes(vertices, faces, iterations, lam=0.5, mu=-0.53, boundary="fixed", max_displacement=None):
    """-> (adjacency, the list of every pass's Y)."""
    v, f = _arrays(vertices, faces)
    adj = adjacency(v, f, boundary)
    out, X = [], v
    for _ in range(int(iterations)):
        for factor in (lam, mu) if np.float32(mu) != 0 else (lam,):
            X = one_pass(X, v, adj, factor, max_displacement)
            out.append(X)
    return adj, out


def smooth(vertices, colours, faces, iterations, lam=0.5, mu=-0.53, boundary="fixed", max_displacement=None):
    """-> (vertices, colours or None, faces, report) as mesh_smooth.smooth_mesh returns them."""
    v, f = _arrays(vertices, faces)
    adj, ys = passes(v, f, iterations, lam, mu, boundary, max_displacement)
    c = None if colours is None else np.ascontiguousarray(np.asarray(colours, np.uint8).reshape(-1, 3))
    report = {"vertices": len(v), "faces": len(f)}
    report.update({k: adj[k] for k in ("invalid_faces", "non_finite_vertices", "edges", "boundary_edges", "non_manifold_edges",
                                       "boundary_vertices", "fixed_vertices")})
    report.update(iterations=int(iterations), lam=float(np.float32(lam)), mu=float(np.float32(mu)) + 0.0, boundary=boundary,
                  max_displacement=None if max_displacement is None else float(np.float32(max_displacement)))
    return ys[-1], c, f, report


# ------------------------------------------------------------------------------------------------ built meshes

@functools.lru_cache(maxsize=None)
def sphere(stacks, slices):
    """A closed UV sphere of radius 1: two poles and stacks - 1 rings of `slices` vertices, 2 slices (stacks - 1) faces, outward
    winding.  Treat as read-only."""
    theta = np.pi * np.arange(1, stacks) / stacks
    phi = 2 * np.pi * np.arange(slices) / slices
    ring = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None], np.sin(theta)[:, None] * np.sin(phi)[None],
                     np.repeat(np.cos(theta)[:, None], slices, 1)], 2).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1]], ring, [[0, 0, -1]]]).astype(np.float32)
    at = lambda i, j: 1 + i * slices + (j % slices)
    south = len(v) - 1
    f = []
    for j in range(slices):
        f.append([0, at(0, j), at(0, j + 1)])
        for i in range(stacks - 2):
            f.append([at(i, j), at(i + 1, j), at(i + 1, j + 1)])
            f.append([at(i, j), at(i + 1, j + 1), at(i, j + 1)])
        f.append([south, at(stacks - 2, j + 1), at(stacks - 2, j)])
    return v, np.asarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def fan(spokes):
    """A hub (vertex 0, lifted off the plane) and `spokes` rim vertices on the unit circle, one face per pair of rim
    neighbours: the hub's row has `spokes` neighbours, every rim vertex is a boundary vertex.  Treat as read-only."""
    phi = 2 * np.pi * np.arange(spokes) / spokes
    v = np.concatenate([[[0.1, -0.05, 0.3]], np.stack([np.cos(phi), np.sin(phi), np.zeros(spokes)], 1)]).astype(np.float32)
    j = np.arange(spokes)
    return v, np.stack([np.zeros(spokes, np.int64), 1 + j, 1 + (j + 1) % spokes], 1).astype(np.int32)


def three_on_one_edge():
    """Three faces that share the edge 0-1: one non-manifold edge, six boundary edges."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.2], [0.5, 0, 1]], np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


MESHES = ("grid", "strip63", "strip64", "strip65", "sphere", "fan200", "three", "doubled", "lone", "none")


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The meshes of the GPU tests -> (vertices, colours, faces), read-only.  grid: 12 x 12 quads with the four invalid faces
    and the three vertices that are not finite of test_gpu_arena_mesh_simplify.case("grid"); strip63 / 64 / 65: a strip of as
    many faces (a wave's edge); sphere: closed, no boundary; fan200: one row of 200 neighbours; three: three faces on one edge;
    doubled: one face twice; lone: six vertices and no face; none: nothing."""
    rs = np.random.RandomState(8)
    if name == "grid":
        v, f = (x.copy() for x in grid(12))
        f[5], f[17], f[40], f[99] = [-1, 0, 1], [0, 1, len(v)], [3, 2 ** 31 - 1, 4], [-2 ** 31, 7, 8]
        v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
    elif name.startswith("strip"):
        v, f = (x.copy() for x in strip(int(name[5:]), 1))
        v[:, 2] = np.sin(np.arange(len(v)))                                    # off the plane, so that every axis moves
    elif name == "sphere":
        v, f = sphere(6, 8)
        v = (v * (1 + 0.05 * rs.randn(len(v)))[:, None]).astype(np.float32)
    elif name == "fan200":
        v, f = fan(200)
    elif name == "three":
        v, f = three_on_one_edge()
    elif name == "doubled":
        v, f = doubled_face()
    elif name == "lone":
        v, f = rs.rand(6, 3).astype(np.float32), np.zeros((0, 3), np.int32)
    else:
        assert name == "none", name
        v, f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    for x in (v, c, f):
        x.setflags(write=False)
    return v, c, f


def near_float_max():
    """One triangle whose x coordinates are +-3e38: a pass with a negative factor leaves float32 at every vertex."""
    v = np.array([[3e38, 0, 0], [-3e38, 0, 0], [-3e38, 1, 0]], np.float32)
    return v, np.array([[0, 1, 2]], np.int32)


def doubled_face():
    """One triangle given twice, once the other way round: every edge has multiplicity 2, none is a boundary."""
    v = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0.25]], np.float32)
    return v, np.array([[0, 1, 2], [2, 1, 0]], np.int32)
