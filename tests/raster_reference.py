"""Numpy restatement of the triangle rasteriser of mvsnet_amd/render_mesh.py (the semantics in its docstring): vertices
projected in float32, snapped to 1/256 pixel, integer edge functions with the edge ownership rule, perspective-correct
depth in float64, a z-buffer of uint64 keys.  Every (face, pixel of its bounding box) pair of a view is one element of a
numpy array, so nothing loops over faces.  Besides depth and index it returns, per pixel, the number of faces that cover
it, which the kernels do not have; and it holds the meshes the tests draw."""
from __future__ import annotations

import functools

import numpy as np

from tests import render_reference as R

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
GUARD = np.float32(2.0 ** 28)
CULL = {None: 0, "back": 1, "front": -1}
PAIRS_PER_CHUNK = 1 << 21


def project_vertices(P, vertices, min_depth=0.0):
    """One view: -> (qx, qy int64 in 1/256 pixel (0 where unusable), w float32, usable bool), all (M,)."""
    X, Y, Z = (np.asarray(vertices, np.float32)[:, k] for k in range(3))
    P = np.asarray(P, np.float32)
    with np.errstate(all="ignore"):
        u, v, w = [((P[r, 0] * X + P[r, 1] * Y) + P[r, 2] * Z) + P[r, 3] for r in range(3)]
        qx = np.floor((u / w) * np.float32(256) + np.float32(0.5))
        qy = np.floor((v / w) * np.float32(256) + np.float32(0.5))
        ok = np.isfinite(w) & (w > np.float32(min_depth)) & (np.abs(qx) <= GUARD) & (np.abs(qy) <= GUARD)
    assert qx.dtype == np.float32 and w.dtype == np.float32
    return np.where(ok, qx, 0).astype(np.int64), np.where(ok, qy, 0).astype(np.int64), w, ok


def face_setup(qx, qy, w, ok, faces, H, W, cull=0):
    """Per face of one view -> dict of (F,) arrays: the snapped corners xa..yc, wa..wc, area2, sgn, the clipped bounding box
    x0..y1 and `valid` (False: the face is dropped in this view, or its box holds no pixel of the image)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    M = len(qx)
    inr = ((f >= 0) & (f < M)).all(1)
    fc = np.where(inr[:, None], f, 0)
    s = {}
    for n, k in (("a", 0), ("b", 1), ("c", 2)):
        s["x" + n], s["y" + n], s["w" + n] = qx[fc[:, k]], qy[fc[:, k]], w[fc[:, k]]
    area2 = (s["xb"] - s["xa"]) * (s["yc"] - s["ya"]) - (s["yb"] - s["ya"]) * (s["xc"] - s["xa"])
    valid = inr & ok[fc].all(1) & (area2 != 0)
    if cull > 0:
        valid &= ~(area2 > 0)
    if cull < 0:
        valid &= ~(area2 < 0)
    xs, ys = np.stack([s["xa"], s["xb"], s["xc"]]), np.stack([s["ya"], s["yb"], s["yc"]])
    s["x0"], s["x1"] = np.maximum((xs.min(0) + 255) >> 8, 0), np.minimum(xs.max(0) >> 8, W - 1)
    s["y0"], s["y1"] = np.maximum((ys.min(0) + 255) >> 8, 0), np.minimum(ys.max(0) >> 8, H - 1)
    s["dropped"] = ~valid
    s["valid"] = valid & (s["x0"] <= s["x1"]) & (s["y0"] <= s["y1"])
    s["area2"], s["sgn"] = area2, np.sign(area2)
    return s


def _edge(sgn, xs, ys, xe, ye, px, py):
    """The edge function of start -> end at p and whether p is inside or on an owned edge."""
    dx, dy = xe - xs, ye - ys
    e = sgn * (dx * (py - ys) - dy * (px - xs))
    ox, oy = sgn * dx, sgn * dy
    return e, (e > 0) | ((e == 0) & ((oy > 0) | ((oy == 0) & (ox < 0))))


def edges(s, x, y):
    """s: the setup gathered per element; pixel (x, y) int64 -> (e_a, e_b, e_c, covered)."""
    px, py = 256 * x, 256 * y
    ea, ia = _edge(s["sgn"], s["xb"], s["yb"], s["xc"], s["yc"], px, py)
    eb, ib = _edge(s["sgn"], s["xc"], s["yc"], s["xa"], s["ya"], px, py)
    ec, ic = _edge(s["sgn"], s["xa"], s["ya"], s["xb"], s["yb"], px, py)
    return ea, eb, ec, ia & ib & ic


def weights(s, ea, eb, ec):
    """-> (t_a, t_b, t_c, sum) in float64: t_k = double(e_k) (1 / double(w_k)), sum = (t_a + t_b) + t_c."""
    with np.errstate(all="ignore"):
        ta = ea.astype(np.float64) * (1.0 / s["wa"].astype(np.float64))
        tb = eb.astype(np.float64) * (1.0 / s["wb"].astype(np.float64))
        tc = ec.astype(np.float64) * (1.0 / s["wc"].astype(np.float64))
    return ta, tb, tc, (ta + tb) + tc


def _pairs(s):
    """Chunks of (face index, x, y) over every pixel of every valid face's box."""
    ids = np.nonzero(s["valid"])[0]
    bw = (s["x1"] - s["x0"] + 1)[ids]
    cnt = bw * (s["y1"] - s["y0"] + 1)[ids]
    start = 0
    while start < len(ids):
        stop = start + max(1, int(np.searchsorted(np.cumsum(cnt[start:]), PAIRS_PER_CHUNK, side="right")))
        c, i = cnt[start:stop], ids[start:stop]
        rep = np.repeat(np.arange(len(i)), c)
        t = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        f = i[rep]
        yield f, s["x0"][f] + t % bw[start:stop][rep], s["y0"][f] + t // bw[start:stop][rep]
        start = stop


def render(vertices, faces, cams, H, W, min_depth=0.0, cull=None, check=False):
    """-> (depth (V,H,W) float32, index (V,H,W) int32, count (V,H,W) int64: the faces that cover each pixel).  check=True
    also asserts e_a + e_b + e_c == |area2| on every pair."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    P = R.projection_tables(cams)
    V = len(P)
    keys = np.full((V, H * W), EMPTY, np.uint64)
    count = np.zeros((V, H * W), np.int64)
    for v in range(V):
        s = face_setup(*project_vertices(P[v], vertices, min_depth), faces, H, W, CULL[cull])
        for f, x, y in _pairs(s):
            g = {k: a[f] for k, a in s.items()}
            ea, eb, ec, cov = edges(g, x, y)
            if check:
                assert np.array_equal(ea + eb + ec, np.abs(g["area2"]))
            g = {k: a[cov] for k, a in g.items()}
            _, _, _, ssum = weights(g, ea[cov], eb[cov], ec[cov])
            z = (np.abs(g["area2"]).astype(np.float64) / ssum).astype(np.float32)
            assert np.isfinite(z).all() and (z > 0).all()
            key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | f[cov].astype(np.uint64)
            pix = y[cov] * W + x[cov]
            np.minimum.at(keys[v], pix, key)
            np.add.at(count[v], pix, 1)
    empty = keys == EMPTY
    depth = np.where(empty, np.uint32(0), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    index = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return depth.reshape(V, H, W), index.reshape(V, H, W), count.reshape(V, H, W)


def interpolate(vertices, faces, cams, H, W, index, attr, min_depth=0.0):
    """-> (V,H,W,C) float32: attr (M,C) float32 interpolated at every pixel whose index names a face that is not dropped in
    that view; 0 elsewhere."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    attr = np.asarray(attr, np.float32)
    P = R.projection_tables(cams)
    V, C = len(P), attr.shape[1]
    out = np.zeros((V, H * W, C), np.float32)
    for v in range(V):
        s = face_setup(*project_vertices(P[v], vertices, min_depth), faces, H, W, 0)
        idx = np.asarray(index[v], np.int64).reshape(-1)
        pix = np.nonzero((idx >= 0) & (idx < len(faces)))[0]
        pix = pix[~s["dropped"][idx[pix]]]
        f = idx[pix]
        g = {k: a[f] for k, a in s.items()}
        ea, eb, ec, _ = edges(g, pix % W, pix // W)
        ta, tb, tc, ssum = weights(g, ea, eb, ec)
        fc = faces[f]
        for c in range(C):
            A = [attr[fc[:, k], c].astype(np.float64) for k in range(3)]
            with np.errstate(all="ignore"):
                out[v, pix, c] = (((ta * A[0] + tb * A[1]) + tc * A[2]) / ssum).astype(np.float32)
    return out.reshape(V, H, W, C)


def colors(vertices, faces, cams, H, W, index, rgb, min_depth=0.0):
    """uint8 vertex colours interpolated as float32 attributes, floor(x + 0.5) in float32, clamped to 0..255."""
    x = interpolate(vertices, faces, cams, H, W, index, np.asarray(rgb, np.uint8).astype(np.float32), min_depth)
    return np.clip(np.floor(x + np.float32(0.5)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ meshes

def pixel_cam(H, W, f=1.0):
    """Identity pose, focal length f, principal point (0, 0): the point (x z / f, y z / f, z) lands on pixel (x, y)."""
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[1, :3, :3] = [[f, 0, 0], [0, f, 0], [0, 0, 1.0]]
    return cam[None]


def aligned_grid(n=9, step=4, z=2.0):
    """n x n vertices exactly on the pixel centres (step i, step j) of pixel_cam, two triangles per cell, diagonals
    alternating; drawn with pixel_cam(f=1) it covers the half-open square [0, step (n - 1))^2."""
    jj, ii = np.mgrid[0:n, 0:n]
    verts = np.stack([ii.reshape(-1) * step * z, jj.reshape(-1) * step * z, np.full(n * n, z)], 1).astype(np.float32)
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            faces += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return verts, np.array(faces, np.int32)


def uv_sphere(radius=0.8, centre=(0.0, 0.0, 4.0), stacks=24, slices=32):
    """A closed sphere, wound so that the normals (b - a) x (c - a) point outward."""
    c = np.asarray(centre, np.float64)
    verts = [c + [0, 0, radius]]
    for i in range(1, stacks):
        th = np.pi * i / stacks
        for j in range(slices):
            ph = 2 * np.pi * j / slices
            verts.append(c + radius * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
    verts.append(c - [0, 0, radius])
    ring = lambda i, j: 1 + (i - 1) * slices + j % slices
    faces = []
    for j in range(slices):
        faces.append([0, ring(1, j), ring(1, j + 1)])
        faces.append([len(verts) - 1, ring(stacks - 1, j + 1), ring(stacks - 1, j)])
        for i in range(1, stacks - 1):
            faces += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    return np.array(verts).astype(np.float32), np.array(faces, np.int32)


@functools.lru_cache(maxsize=None)
def scene_mesh(kind):
    """(vertices float32, colours uint8, faces int32, cams) of mesh_reference's coloured scene mesh; treat as read-only."""
    from tests import mesh_reference as MR
    m = MR.scene_mesh(kind, colour=True)
    return m["vertices"].astype(np.float32), m["colours"], m["faces"], MR.scene(kind)["cams"]


def at_pixel(x, y, z):
    """The points that pixel_cam(f=1) sees at pixel position (x, y) (fractions allowed) and depth z, (n,3) float64."""
    x, y, z = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(z, np.float64))
    return np.stack([x * z, y * z, z], -1)


def soup(corners, z):
    """Independent triangles: corners (n,3,2) in pixels of pixel_cam(f=1), z (n,) or (n,3) -> (vertices, faces)."""
    corners = np.asarray(corners, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64).reshape(len(corners), -1), corners.shape[:2])
    verts = at_pixel(corners[..., 0], corners[..., 1], z).reshape(-1, 3).astype(np.float32)
    return verts, np.arange(3 * len(corners), dtype=np.int32).reshape(-1, 3)


def join(*meshes):
    """Meshes (vertices, faces) one after the other, face indices shifted."""
    verts, faces, m = [], [], 0
    for v, f in meshes:
        verts.append(v)
        faces.append(np.asarray(f, np.int32) + m)
        m += len(v)
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32)


def subpixel_soup(n=3000, H=40, W=48, size=0.45, seed=7):
    """n triangles of about `size` pixels at random places in and just around the image, random depths and windings: most
    cover no pixel centre, some cover one."""
    rs = np.random.RandomState(seed)
    centre = np.stack([rs.uniform(-2, W + 1, n), rs.uniform(-2, H + 1, n)], 1)
    return soup(centre[:, None, :] + rs.uniform(-size, size, (n, 3, 2)), rs.uniform(1.0, 3.0, (n, 3)))


def offscreen_quad(z=2.0, far=5000.0):
    """Two triangles whose corners lie `far` pixels outside any image at the origin; together they cover every pixel once."""
    c = np.array([[-far, -far], [far + 7, -far], [far + 7, far + 3], [-far, far + 3]])
    return at_pixel(c[:, 0], c[:, 1], z).astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def mixed_mesh():
    """Both kinds of triangle for a 40 x 48 view of pixel_cam(f=1): the aligned grid (boxes of 25 pixels), a sub-pixel soup,
    and an off-screen quad at depth 2 that lies behind some of them and in front of others."""
    return join(aligned_grid(), subpixel_soup(), offscreen_quad())


def one_pixel_stack(n=4096, x=4, y=3, seed=11):
    """n triangles around the centre of pixel (x, y), depths 1 + k / 1000 shuffled, 50 of them tied at depth 1."""
    rs = np.random.RandomState(seed)
    z = np.float32(1.0) + np.arange(1, n - 49, dtype=np.float32) * np.float32(1e-3)
    z = np.concatenate([z, np.full(50, 1.0, np.float32)])[rs.permutation(n)]
    c = np.array([[x - 0.4, y - 0.3], [x + 0.4, y - 0.3], [x, y + 0.45]])
    return soup(np.broadcast_to(c, (n, 3, 2)) + rs.uniform(-0.05, 0.05, (n, 3, 2)), z.astype(np.float64)[:, None]) + (z,)
