"""Numpy restatement of mvsnet_amd/mesh_colour.py (the semantics in its docstring): the incidence keys, the area-weighted vertex
normals summed face after face in float64, the per-view visibility test and bilinear sample in float32 with the weights and sums
in float64, and the final bytes.  The depth maps come from tests/raster_reference.py.  Nothing here imports the package: the
projection tables and the camera centres are restated too.  It also holds the meshes and scenes the tests colour, built in
code, and `hazards`, which says what a (mesh, scene) pair exercises."""
from __future__ import annotations

import functools

import numpy as np

from tests import raster_reference as RR
from tests import render_reference as R

DEAD = np.int64(2 ** 63 - 1)
F32 = np.float32
DEFAULTS = dict(min_cos=0.2, angle_power=2, occlusion_rel=0.01, min_depth=0.0, view_chunk=8)
REPORT_FIELDS = ("vertices", "faces", "invalid_faces", "zero_normals", "unseen_vertices", "views", "min_cos", "angle_power",
                 "occlusion_rel", "min_depth", "view_chunk")


# ------------------------------------------------------------------------------------------------ steps 1 and 2

def incidence_keys(vertices, faces):
    """-> (keys (3 F,) int64, invalid faces)."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    M = len(v)
    inside = ((f >= 0) & (f < M)).all(1)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    g = np.where(inside[:, None], f, 0)                                        # an index outside is never dereferenced
    finite = np.isfinite(v[g].reshape(len(f), 9)).all(1) if M else np.zeros(len(f), bool)
    valid = inside & distinct & finite
    keys = np.where(valid[:, None], (g << 31) | np.arange(len(f), dtype=np.int64)[:, None], DEAD)
    return keys.reshape(-1).astype(np.int64), int((~valid).sum())


def normals(vertices, faces):
    """-> (normals (M,3) float32, dict(keys, sorted_keys, invalid_faces, zero_normals))."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    M = len(v)
    keys, invalid = incidence_keys(v, f)
    sk = np.sort(keys)
    out = np.zeros((M, 3), F32)
    zero = 0
    d = v.astype(np.float64)
    for j in range(M):
        first, last = np.searchsorted(sk, np.int64(j) << 31, "left"), np.searchsorted(sk, np.int64(j + 1) << 31, "left")
        s = [np.float64(0), np.float64(0), np.float64(0)]
        with np.errstate(all="ignore"):
            for e in range(first, last):
                a, b, c = f[int(sk[e] & 0x7fffffff)]
                u, w = d[b] - d[a], d[c] - d[a]
                s[0] = s[0] + (u[1] * w[2] - u[2] * w[1])
                s[1] = s[1] + (u[2] * w[0] - u[0] * w[2])
                s[2] = s[2] + (u[0] * w[1] - u[1] * w[0])
            length = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
            if first < last and length > 0 and np.isfinite(length):
                out[j] = [F32(s[0] / length), F32(s[1] / length), F32(s[2] / length)]
            else:
                zero += 1
    return out, dict(keys=keys, sorted_keys=sk, invalid_faces=invalid, zero_normals=zero)


# ------------------------------------------------------------------------------------------------ step 3

def camera_centres(cams):
    """(V,3) float32: -((R0i t0 + R1i t1) + R2i t2) in float64, rounded once."""
    cams = np.asarray(cams, np.float64)
    Rm, t = cams[:, 0, :3, :3], cams[:, 0, :3, 3]
    return np.stack([-((Rm[:, 0, i] * t[:, 0] + Rm[:, 1, i] * t[:, 1]) + Rm[:, 2, i] * t[:, 2]) for i in range(3)], 1).astype(F32)


def occlusion_ratio(rel):
    return F32(1.0 + float(rel))


def accumulate(vertices, nrm, cams, images, depth, acc, seen, min_cos=0.2, angle_power=2, occlusion_rel=0.01, min_depth=0.0,
               trace=None):
    """Adds the V views (one size) to acc (M,4) float64 and seen (M,) int32 in place; depth (V,H,W) float32 from the
    rasteriser.  trace, a list, receives per view a dict of the masks `hazards` reads."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    n = np.asarray(nrm, F32).reshape(-1, 3)
    P = R.projection_tables(cams).reshape(-1, 3, 4)
    C = camera_centres(cams)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    V, H, W = depth.shape
    ratio, cut, md = occlusion_ratio(occlusion_rel), np.float64(F32(min_cos)), F32(min_depth)
    wmax, hmax, half, one = F32(W - 1), F32(H - 1), F32(0.5), F32(1)
    live = np.isfinite(v).all(1) & ~(n == 0).all(1)
    for k in range(V):
        with np.errstate(all="ignore"):
            u, t, w = [((P[k, r, 0] * X + P[k, r, 1] * Y) + P[k, r, 2] * Z) + P[k, r, 3] for r in range(3)]
            front = live & np.isfinite(w) & (w > md)
            sx, sy = u / w, t / w
            usable = front & np.isfinite(sx) & np.isfinite(sy)
            px, py = np.floor(sx + half), np.floor(sy + half)
            inside = usable & (px >= 0) & (px <= wmax) & (py >= 0) & (py <= hmax)
            ix, iy = np.where(inside, px, 0).astype(np.int64), np.where(inside, py, 0).astype(np.int64)
            zb = depth[k, iy, ix]
            reach = zb * ratio
            assert reach.dtype == F32 and sx.dtype == F32
            shown = inside & (zb > 0) & (w <= reach)
            d = C[k].astype(np.float64)[None, :] - v.astype(np.float64)
            q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            nd = n.astype(np.float64)
            c = ((nd[:, 0] * d[:, 0] + nd[:, 1] * d[:, 1]) + nd[:, 2] * d[:, 2]) / np.sqrt(q)
            sees = shown & (q > 0) & (c >= cut)
            g = np.ones_like(c)
            if angle_power > 0:
                g = c.copy()
                for _ in range(angle_power - 1):
                    g = g * c
            x0, y0 = np.floor(sx), np.floor(sy)
            fx, fy = sx - x0, sy - y0
            gx, gy = one - fx, one - fy
            clampi = lambda a, top: np.where(sees, np.minimum(np.maximum(a, F32(0)), top), 0).astype(np.int64)
            xa, xb, ya, yb = clampi(x0, wmax), clampi(x0 + one, wmax), clampi(y0, hmax), clampi(y0 + one, hmax)
            im = np.asarray(images[k], np.uint8)
            for ch in range(3):
                tap = lambda yy, xx: im[yy, xx, ch].astype(F32)
                top = gx * tap(ya, xa) + fx * tap(ya, xb)
                bot = gx * tap(yb, xa) + fx * tap(yb, xb)
                s = gy * top + fy * bot
                assert s.dtype == F32
                acc[sees, ch] = acc[sees, ch] + (g * s.astype(np.float64))[sees]
            acc[sees, 3] = acc[sees, 3] + g[sees]
            seen[sees] += 1
            if trace is not None:
                trace.append(dict(behind=live & ~front, outside=usable & ~inside, hidden=inside & ~shown, back=shown & (c < 0),
                                  sees=sees, left=sees & (x0 < 0), right=sees & (x0 + one > wmax), top=sees & (y0 < 0),
                                  bottom=sees & (y0 + one > hmax)))


# ------------------------------------------------------------------------------------------------ step 4 and the whole

def finish(colours, acc, seen):
    """-> (colours (M,3) uint8, unseen vertices)."""
    M = len(acc)
    took = (seen > 0) & (acc[:, 3] > 0)
    old = np.zeros((M, 3), np.uint8) if colours is None else np.asarray(colours, np.uint8).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x = np.floor(acc[:, :3] / acc[:, 3:4] + 0.5)
    new = np.clip(np.where(np.isnan(x), 0, x), 0, 255).astype(np.uint8)
    return np.where(took[:, None], new, old).astype(np.uint8), int((~took).sum())


def size_groups(images):
    groups = {}
    for k, im in enumerate(images):
        groups.setdefault(tuple(im.shape[:2]), []).append(k)
    return list(groups.items())


def colour(vertices, colours, faces, cams, images, min_cos=0.2, angle_power=2, occlusion_rel=0.01, min_depth=0.0, view_chunk=8,
           views=None, state=None, trace=None):
    """-> (vertices, colours (M,3) uint8, faces, report, state): state = dict(normals, acc, seen, keys, sorted_keys).  views
    picks views (positions, each group ascending); state continues an earlier call's acc and seen."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    cams = np.asarray(cams, np.float64)
    M = len(v)
    if state is None:
        nrm, info = normals(v, f)
        state = dict(info, normals=nrm, acc=np.zeros((M, 4), np.float64), seen=np.zeros(M, np.int32))
    pick = list(range(len(images))) if views is None else list(views)
    if M and len(f):
        for (H, W), members in size_groups([images[k] for k in pick]):
            members = [pick[m] for m in members]
            depth = RR.render(v, f, cams[members], H, W, min_depth=float(F32(min_depth)))[0]
            accumulate(v, state["normals"], cams[members], [images[k] for k in members], depth, state["acc"], state["seen"],
                       min_cos, angle_power, occlusion_rel, min_depth, trace)
    out, unseen = finish(colours, state["acc"], state["seen"])
    values = (M, len(f), state["invalid_faces"], state["zero_normals"], unseen, len(pick), float(F32(min_cos)), int(angle_power),
              float(occlusion_rel), float(F32(min_depth)), int(view_chunk))
    return v, out, f, dict(zip(REPORT_FIELDS, values)), state


# ------------------------------------------------------------------------------------------------ cameras, meshes, scenes

def look_at(eye, target, f, H, W):
    """cam (2,4,4): at `eye`, looking at `target`, focal length f pixels, principal point at the image centre; image y is
    world y for a camera that looks along +z."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[0, :3, :3] = np.stack([x, y, z])
    cam[0, :3, 3] = -cam[0, :3, :3] @ eye
    cam[1, :3, :3] = [[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]]
    return cam


def plane(nx, ny, x0, x1, y0, y1, z):
    """nx x ny vertices on z, two triangles per cell, wound so that (b - a) x (c - a) points to -z (at the cameras)."""
    jj, ii = np.mgrid[0:ny, 0:nx]
    v = np.stack([x0 + (x1 - x0) * ii.reshape(-1) / (nx - 1), y0 + (y1 - y0) * jj.reshape(-1) / (ny - 1), np.full(nx * ny, z)], 1)
    faces = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            faces += [[a, c, b], [a, d, c]]
    return v.astype(F32), np.array(faces, np.int32)


def strip(n):
    """n vertices zigzagging along x on z = 4, n - 2 faces of one winding (towards -z)."""
    k = np.arange(n)
    v = np.stack([-1.0 + 2.0 * k / (n - 1), np.where(k % 2 == 0, -0.2, 0.2), np.full(n, 4.0)], 1).astype(F32)
    f = np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i, i + 2, i + 1] for i in range(n - 2)], np.int32)
    return v, f


ONE_F, ONE_H, ONE_W = 40.0, 20, 24                  # the camera of scene "one": identity pose


def tabs():
    """Four triangles at depth 3, each with one corner within half a pixel of a border of scene "one"'s image: the pixel
    positions (-0.3, 10), (23.3, 10), (12, -0.3), (12, 19.3)."""
    pix = np.array([[[-0.3, 10], [3, 12], [3, 8]], [[23.3, 10], [20, 8], [20, 12]], [[12, -0.3], [10, 3], [14, 3]],
                    [[12, 19.3], [14, 16], [10, 16]]])
    z = 3.0
    xyz = np.stack([(pix[..., 0] - (ONE_W - 1) / 2.0) * z / ONE_F, (pix[..., 1] - (ONE_H - 1) / 2.0) * z / ONE_F, np.full(pix.shape[:2], z)], -1)
    return xyz.reshape(-1, 3).astype(F32), np.arange(12, dtype=np.int32).reshape(4, 3)


MESHES = ("grid", "strip63", "strip65", "strip257", "tetra", "none")


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices float32, colours uint8, faces int32), read-only.
    grid: a 9 x 7 front plane on z = 4, a 5 x 5 rear plane on z = 5 behind it, the four border tabs, and the hazards: a
    face with an index outside 0..M-1 (two of them), a face with a repeated index, a vertex that is not finite (in a face), an
    unreferenced vertex.  strip<n>: n vertices.  tetra: a closed tetrahedron around (0, 0, 4), wound outward.  none: nothing."""
    rs = np.random.RandomState(21)
    if name == "grid":
        v, f = RR.join(plane(9, 7, -1.0, 1.0, -0.75, 0.75, 4.0), plane(5, 5, 0.2, 0.8, -0.4, 0.4, 5.0), tabs())
        M = len(v)
        v = np.concatenate([v, np.array([[0.1, np.nan, 4.0], [0.3, 0.2, 3.5]], F32)])                # not finite; unreferenced
        f = np.concatenate([f, np.array([[0, 1, M + 2], [-1, 2, 3], [4, 4, 5], [10, 11, M]], np.int32)])
    elif name.startswith("strip"):
        v, f = strip(int(name[5:]))
    elif name == "tetra":
        v = (np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * 0.5 + [0, 0, 4.0]).astype(F32)
        f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    else:
        v, f = np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    for x in (v, c, f):
        x.setflags(write=False)
    return v, c, f


SCENES = ("one", "three", "five", "mixed", "nine")
TARGET = (0.0, 0.0, 4.5)
SMALL, LARGE = (20, 24), (29, 37)
SIDE_EYE, SIDE_TARGET = (4.0, 0.0, 1.0), (0.5, 0.0, 5.0)      # from here the rear plane shows past the front plane's edge


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(cams (V,2,4,4) float64, images [V of (H,W,3) uint8]), read-only.
    one: the identity camera of the tabs, 20 x 24.  three: 29 x 37, two front views in which the front plane hides the rear
    one, and a side view from (4, 0, 1) that sees the rear plane past the front one.  five: 20 x 24, two front views, a view
    from behind (it sees the back of the surface), a view from between the planes (the front plane is behind it) and a narrow
    view (projections outside the image).  mixed: four views, 20 x 24 and 29 x 37 alternating.  nine: nine front views on an
    arc, 20 x 24, more than the default view_chunk."""
    rs = np.random.RandomState(34)
    cam = lambda eye, size, f, target=TARGET: look_at(eye, target, f, size[0], size[1])
    if name == "one":
        views = [(cam((0, 0, 0), SMALL, ONE_F, (0, 0, 1)), SMALL)]
    elif name == "three":
        views = [(cam((-1.5, 0.2, 0), LARGE, 60.0), LARGE), (cam((1.5, 0.5, 0), LARGE, 60.0), LARGE), (cam(SIDE_EYE, LARGE, 90.0, SIDE_TARGET), LARGE)]
    elif name == "five":
        views = [(cam((-0.8, 0, 0), SMALL, 40.0), SMALL), (cam((0, 0, 9.5), SMALL, 40.0, (0, 0, 4)), SMALL),
                 (cam((0.1, 0, 4.5), SMALL, 20.0, (0.1, 0, 6)), SMALL), (cam((0.9, -0.4, 0.5), SMALL, 40.0), SMALL),
                 (cam((0, 0, 0), SMALL, 160.0, (0, 0, 1)), SMALL)]
    elif name == "mixed":
        views = [(cam((-1, 0, 0), SMALL, 40.0), SMALL), (cam((1, 0.3, 0), LARGE, 60.0), LARGE), (cam(SIDE_EYE, SMALL, 60.0, SIDE_TARGET), SMALL),
                 (cam((0, -1, 0.5), LARGE, 60.0), LARGE)]
    else:
        views = [(cam((2.0 * np.sin(a), 0.6 * np.cos(3 * a), 4.5 - 4.5 * np.cos(a)), SMALL, 40.0), SMALL) for a in np.linspace(-0.5, 0.5, 9)]
    cams = np.stack([c for c, _ in views])
    images = [rs.randint(0, 256, size + (3,)).astype(np.uint8) for _, size in views]
    cams.setflags(write=False)
    for im in images:
        im.setflags(write=False)
    return dict(cams=cams, images=images)


@functools.lru_cache(maxsize=None)
def case(mesh_name, scene_name, with_colours=True):
    """The reference's answer for one (mesh, scene) under the default options, computed once and shared: (vertices, colours,
    faces, report, state, trace)."""
    v, c, f = mesh(mesh_name)
    s = scene(scene_name)
    trace = []
    out = colour(v, c if with_colours else None, f, s["cams"], s["images"], trace=trace)
    for x in (out[1], out[4]["normals"], out[4]["acc"], out[4]["seen"]):
        x.setflags(write=False)
    return out + (trace,)


HAZARDS = ("invalid index", "repeated index", "not finite", "unreferenced", "hidden", "hidden then seen", "behind", "outside",
           "left", "right", "top", "bottom", "back", "seen by none")


def hazards(mesh_name, scene_name):
    """The names of HAZARDS that this pair exercises."""
    v, c, f = mesh(mesh_name)
    found = set()
    if not len(v):
        return found
    M = len(v)
    f64 = f.astype(np.int64)
    inside = ((f64 >= 0) & (f64 < M)).all(1)
    if (~inside).any():
        found.add("invalid index")
    if (inside & ((f64[:, 0] == f64[:, 1]) | (f64[:, 1] == f64[:, 2]) | (f64[:, 2] == f64[:, 0]))).any():
        found.add("repeated index")
    if (~np.isfinite(v).all(1)).any():
        found.add("not finite")
    if len(np.setdiff1d(np.arange(M), f64[inside].reshape(-1))):
        found.add("unreferenced")
    _, _, _, _, state, trace = case(mesh_name, scene_name)
    hidden = np.stack([t["hidden"] for t in trace]).any(0)
    sees = np.stack([t["sees"] for t in trace]).any(0)
    for key in ("behind", "outside", "left", "right", "top", "bottom", "back", "hidden"):
        if np.stack([t[key] for t in trace]).any():
            found.add(key)
    if (hidden & sees).any():
        found.add("hidden then seen")
    referenced = np.zeros(M, bool)
    referenced[f64[inside].reshape(-1)] = True
    if (referenced & np.isfinite(v).all(1) & (state["seen"] == 0)).any():
        found.add("seen by none")
    return found
