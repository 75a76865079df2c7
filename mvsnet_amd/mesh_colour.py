"""Vertex normals and per-vertex colour from the full-resolution images on the MI355X: the last stage of a mesh, after the
removal of small pieces (mvsnet_amd.mesh_clean), the smoothing (mvsnet_amd.mesh_smooth) and the simplification
(mvsnet_amd.mesh_simplify), and the way to give a scanner's mesh the colours of a session.  Every vertex takes the weighted mean
of what the views that see it show at its projection; occlusion is resolved against the project's own rasteriser
(mvsnet_amd.render_mesh) and a view weighs by how squarely it sees the surface.

    python -m mvsnet_amd.mesh_colour --mesh IN.ply --out OUT.ply (--session DIR | --dense_folder DIR) [--mesh_scale S]
        [--transform T.txt] [--min_cos 0.2] [--angle_power 2] [--occlusion_rel 0.01] [--min_depth D] [--view_chunk 8]
        [--write_normals] [--force]

The kernels are csrc/mesh_colour.hip (mvs_mesh_normals_keys_i64, mvs_mesh_normals_f32, mvs_mesh_colour_accumulate_f32,
mvs_mesh_colour_finish_u8); torch owns the device memory, the sort of the incidence keys and the one read-back of the counts, and
the depth maps come from render_mesh.RasterPlan at the images' own size, a chunk of views at a time.

Semantics (shared by the kernels, tests/mesh_colour_reference.py and the tests).  Conventions are render_mesh.py's: cams
(V,2,4,4); pixel (x, y) is column x, row y, its centre at integer coordinates; P_v = K_v [R_v | t_v] comes from
render.projection_tables.  float32 arithmetic has every product, sum and quotient rounded on its own (no fused multiply-add,
correctly rounded divisions), and float64 arithmetic has no contraction either.
  * Input: vertices (M,3) float32, colours (M,3) uint8 or None, faces (F,3) int32; M <= 2^31 - 1 and 3 F <= 2^31 - 1.  Positions
    and faces leave the call unchanged, byte for byte; only colours change.
  * 1. Incidence keys.  Face f = (a, b, c) is valid when its three indices lie in 0 .. M - 1, are pairwise different, and all
    nine coordinates are finite.  A valid face gives the three keys int64(vertex) << 31 | f, an invalid face 2^63 - 1 three
    times.  Invalid faces are counted (status word 0) and their indices are never dereferenced.  The 3 F keys are sorted
    ascending (torch).
  * 2. Vertex normals.  For vertex v a lower-bound search in the sorted keys for v << 31 and for (v + 1) << 31 bounds its run.
    Over the run, in ascending face index, the face's (b - a) x (c - a) is summed in float64: the coordinates are widened from
    float32, each difference and each product is rounded, each component is p1 - p2 (x: uy wz - uz wy, y: uz wx - ux wz,
    z: ux wy - uy wx with u = b - a, w = c - a), and the three sums grow one face after the other.  n = sum / sqrt((sx sx +
    sy sy) + sz sz), each component rounded to float32 once.  The normal is (0, 0, 0) when the run is empty, the length is 0 or
    the length is not finite; status word 1 counts those vertices.  This is the area-weighted normal; mesh.py's faces wind
    outward, so it points at the cameras.
  * 3. Accumulation.  One call covers views of one size H x W, in ascending order; a later call continues the same sums, as
    TsdfVolume.integrate does.  Inputs: depth (V,H,W) float32 as mvs_raster_mesh_f32 wrote it for this mesh and these cameras
    with cull = 0; images (V,H,W,3) uint8; centres (V,3) float32, -R^T t with each component -((R0i t0 + R1i t1) + R2i t2)
    composed in float64 and rounded once on the host (``camera_centres``); ratio = float32(1 + occlusion_rel), the sum in
    float64; min_cos float32; power, an integer 0 .. 8.  Vertex j = X is seen by view v when all of these hold: its
    coordinates are finite and its normal is not (0, 0, 0); (u, v, w) are render.py's three rows with w finite and
    w > min_depth; sx = u / w and sy = v / w are finite; px = floor(sx + 0.5) and py = floor(sy + 0.5) lie in [0, W - 1] x
    [0, H - 1], compared in float32 before any conversion to an integer; zb = depth[v, py, px] > 0 and w <= zb * ratio (a
    rounded float32 product); in float64, with d = C_v - X, q = (dx dx + dy dy) + dz dz > 0 and c = ((nx dx + ny dy) + nz dz)
    / sqrt(q) >= double(min_cos).  Its weight g is c multiplied by itself power - 1 times, left to right (1.0 for power 0).  Its
    sample, per channel in float32: x0 = floor(sx), fx = sx - x0, taps at x0 and x0 + 1, clamped to [0, W - 1], the same in y;
    top = (1 - fx) c00 + fx c10, bot likewise on the lower row, s = (1 - fy) top + fy bot, every product and sum rounded.  Then
    acc[j][k] += g * double(s_k) for the three channels, acc[j][3] += g and seen[j] += 1.  acc is (M,4) float64 and seen (M)
    int32, zeroed before the first call; a vertex is its own lane's, so there are no atomics on either.
  * 4. Finish.  With seen[j] > 0 and acc[j][3] > 0 the byte is floor(acc[j][k] / acc[j][3] + 0.5) in float64, clamped to
    0 .. 255.  Otherwise the vertex keeps its input colour, or 0 where the mesh came without colours; status word 2 counts
    these vertices.
  * Views of several sizes are taken in groups of one size (render.size_groups: by first appearance, ascending inside a group),
    each group in chunks of view_chunk views; the chunking never changes a byte.
  * Options: min_cos, a float32 in [0, 1], default 0.2; angle_power 0 .. 8, default 2; occlusion_rel, >= 0 with a finite
    float32(1 + rel), default 0.01; min_depth >= 0 and finite in float32, default 0; view_chunk, an integer >= 1, default 8.
    Anything else is a ValueError, raised before any GPU work.
  * Report: vertices, faces, invalid_faces, zero_normals, unseen_vertices, views, and the options.

The PLY with normals adds nx ny nz after x y z, as depthfusion --normals orders them for clouds (``write_mesh_ply_normals``).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

from . import mesh_common
from .mesh_common import MAX_SIZE, inputs, integer, need_gpu, number, refuse_existing, run

WHAT = "mesh colouring"
MAX_AXIS = 1 << 20              # csrc/mesh_colour.hip MC_MAX_AXIS
MAX_POWER = 8                   # MC_MAX_POWER
OPTION_NAMES = ("min_cos", "angle_power", "occlusion_rel", "min_depth", "view_chunk")
REPORT_FIELDS = ("vertices", "faces", "invalid_faces", "zero_normals", "unseen_vertices", "views") + OPTION_NAMES

NORMALS_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                      "property float nx\nproperty float ny\nproperty float nz\n"
                      "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                      "property list uchar int vertex_indices\nend_header\n")
_NORMALS_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                  ("red", "u1"), ("green", "u1"), ("blue", "u1")])


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def _integer(name, value, lo, hi):
    n = integer(value, lo, hi)
    if n is None:
        raise ValueError("%s must be an integer %d .. %s, got %r" % (name, lo, hi if hi < MAX_SIZE else "2^31-1", value))
    return n


def occlusion_ratio(rel):
    """float32(1 + rel), the sum in float64."""
    with np.errstate(over="ignore"):
        return float(np.float32(1.0 + float(rel)))


def check_options(min_cos=0.2, angle_power=2, occlusion_rel=0.01, min_depth=0.0, view_chunk=8):
    """-> (min_cos, angle_power, occlusion_rel, min_depth, view_chunk) with min_cos and min_depth exactly float32; ValueError
    otherwise."""
    with np.errstate(over="ignore"):
        c32 = float(np.float32(number("min_cos", min_cos)))
    if not 0.0 <= c32 <= 1.0:
        raise ValueError("min_cos must lie in [0, 1] as a float32, got %r" % (min_cos,))
    power = _integer("angle_power", angle_power, 0, MAX_POWER)
    rel = number("occlusion_rel", occlusion_rel)
    if not (rel >= 0.0 and math.isfinite(occlusion_ratio(rel))):
        raise ValueError("occlusion_rel must be >= 0 with a finite float32(1 + rel), got %r" % (occlusion_rel,))
    with np.errstate(over="ignore"):
        md = float(np.float32(number("min_depth", min_depth)))
    if not (md >= 0.0 and math.isfinite(md)):
        raise ValueError("min_depth must be >= 0 and finite in float32, got %r" % (min_depth,))
    chunk = _integer("view_chunk", view_chunk, 1, MAX_SIZE)
    return c32 + 0.0, power, rel, md, chunk


def camera_centres(cams):
    """(V,3) float32: C_v = -R^T t, each component -((R0i t0 + R1i t1) + R2i t2) in float64, rounded once."""
    cams = np.asarray(cams, np.float64)
    if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4):
        raise ValueError("cams must be (V,2,4,4), got %s" % (cams.shape,))
    R, t = cams[:, 0, :3, :3], cams[:, 0, :3, 3]
    with np.errstate(all="ignore"):
        c = [-((R[:, 0, i] * t[:, 0] + R[:, 1, i] * t[:, 1]) + R[:, 2, i] * t[:, 2]) for i in range(3)]
        return np.stack(c, 1).astype(np.float32).reshape(-1, 3)


def scale_cams(cams, size, to_size):
    """Cameras of images of `size` (H, W) for the same views at `to_size`: pixel centres are at integer coordinates, so
    x' = (x + 1/2) W' / W - 1/2 and the first two rows of K change accordingly (float64)."""
    cams = np.array(cams, np.float64)
    (h, w), (h2, w2) = size, to_size
    if (h, w) == (h2, w2):
        return cams
    sx, sy = float(w2) / float(w), float(h2) / float(h)
    cams[:, 1, 0, :3] = cams[:, 1, 0, :3] * sx
    cams[:, 1, 0, 2] += 0.5 * sx - 0.5
    cams[:, 1, 1, :3] = cams[:, 1, 1, :3] * sy
    cams[:, 1, 1, 2] += 0.5 * sy - 0.5
    return cams


def write_mesh_ply_normals(path, vertices, normals, colours, faces):
    """mesh.write_mesh_ply's PLY with nx ny nz (float) after x y z."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    if len(vertices) != len(colours) or len(vertices) != len(normals):
        raise ValueError("vertices, normals and colours differ in length")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vertices)):
        raise ValueError("faces name a vertex outside 0..%d" % (len(vertices) - 1))
    from .mesh import _FACE_DTYPE
    v = np.empty(len(vertices), _NORMALS_VERTEX_DTYPE)
    for k, name in enumerate(("x", "y", "z")):
        v[name], v["n" + name] = vertices[:, k], normals[:, k]
    v["red"], v["green"], v["blue"] = colours[:, 0], colours[:, 1], colours[:, 2]
    f = np.empty(len(faces), _FACE_DTYPE)
    f["n"], f["v"] = 3, faces
    with open(path, "wb") as out:
        out.write((NORMALS_PLY_HEADER % (len(v), len(f))).encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def read_mesh_ply_normals(path):
    """Reads what write_mesh_ply_normals writes -> (vertices (M,3) float32, normals (M,3) float32, colours (M,3) uint8, faces
    (F,3) int32)."""
    from .mesh import _FACE_DTYPE
    with open(path, "rb") as fh:
        data = fh.read()
    bad = ValueError("%s: not a PLY written by write_mesh_ply_normals" % path)
    try:
        end = data.index(b"end_header\n") + len(b"end_header\n")
        head = data[:end].decode("ascii")
        m = int(head.split("element vertex ")[1].split("\n")[0])
        nf = int(head.split("element face ")[1].split("\n")[0])
    except (IndexError, ValueError):
        raise bad
    if head != NORMALS_PLY_HEADER % (m, nf) or len(data) != end + m * _NORMALS_VERTEX_DTYPE.itemsize + nf * _FACE_DTYPE.itemsize:
        raise bad
    v = np.frombuffer(data, _NORMALS_VERTEX_DTYPE, count=m, offset=end)
    f = np.frombuffer(data, _FACE_DTYPE, count=nf, offset=end + m * _NORMALS_VERTEX_DTYPE.itemsize)
    if nf and (f["n"] != 3).any():
        raise ValueError("%s: a face is not a triangle" % path)
    return (np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32), np.stack([v["nx"], v["ny"], v["nz"]], 1).astype(np.float32),
            np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.uint8), np.ascontiguousarray(f["v"]).astype(np.int32).reshape(-1, 3))


def _shapes(vertices, colours, faces):
    M, F = mesh_common.shapes(vertices, colours, faces)
    if 3 * F > MAX_SIZE:
        raise ValueError("a mesh of %d faces has more than 2^31 - 1 corners" % F)
    return M, F


def _view_list(cams, images):
    """cams (V,2,4,4) and images, one (V,H,W,3) uint8 array or tensor or V of (H,W,3) -> (cams float64, [image], views as
    render.size_groups takes them)."""
    cams = np.asarray(cams.cpu().numpy() if hasattr(cams, "cpu") else cams, np.float64)
    if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4) or cams.shape[0] < 1:
        raise ValueError("cams must be (V,2,4,4) with V >= 1, got %s" % (cams.shape,))
    images = list(images) if isinstance(images, (list, tuple)) else [images[k] for k in range(len(images))]
    if len(images) != len(cams):
        raise ValueError("%d images for %d cameras" % (len(images), len(cams)))
    views = []
    for k, im in enumerate(images):
        s = tuple(im.shape)
        if len(s) != 3 or s[2] != 3 or s[0] < 1 or s[1] < 1 or "uint8" not in str(im.dtype):
            raise ValueError("image %d must be (H,W,3) uint8, got %s %s" % (k, s, im.dtype))
        if s[0] > MAX_AXIS or s[1] > MAX_AXIS:
            raise ValueError("image %d: %d x %d is beyond 2^20 per axis" % (k, s[0], s[1]))
        views.append((k, cams[k], (s[0], s[1])))
    return cams, images, views


# ------------------------------------------------------------------------------------------------ device side

class _Workspace:
    """The status words of one mesh on the device."""

    def __init__(self, M, F, dev):
        import torch
        from . import _lib
        self.bytes = _lib.load().mvs_mesh_colour_workspace_bytes(M, F)
        if self.bytes == 0:
            raise ValueError("a mesh of %d vertices and %d faces is beyond the kernels' index range" % (M, F))
        self.t = torch.empty(self.bytes, dtype=torch.uint8, device=dev)


def normals_device(vertices, faces, dev, ws=None):
    """vertex_normals on contiguous device tensors -> (normals (M,3) float32 tensor, the workspace whose words 0 and 1 hold the
    invalid faces and the zero normals).  Enqueues only."""
    import torch
    from . import _lib
    M, F = _shapes(vertices, None, faces)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = ws or _Workspace(M, F, dev)
        st = _lib.stream_ptr
        keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        _lib.check(lib.mvs_mesh_normals_keys_i64(_lib.ptr(vertices), M, _lib.ptr(faces), F, _lib.ptr(keys), _lib.ptr(ws.t), ws.bytes, st()),
                   "mvs_mesh_normals_keys_i64")
        sorted_keys = torch.sort(keys)[0]
        normals = torch.empty((M, 3), dtype=torch.float32, device=dev)
        _lib.check(lib.mvs_mesh_normals_f32(_lib.ptr(vertices), M, _lib.ptr(faces), F, _lib.ptr(sorted_keys), _lib.ptr(normals),
                                            _lib.ptr(ws.t), ws.bytes, st()), "mvs_mesh_normals_f32")
    return normals, ws


def vertex_normals(vertices, faces, device=None):
    """Area-weighted vertex normals (step 2 of the module docstring) -> (M,3) float32: a numpy array, or a tensor on the device
    when the vertices came as a tensor."""
    import torch
    _shapes(vertices, None, faces)                                             # first, so that what has no shape is an AttributeError
    dev, v, _, f = inputs(vertices, None, faces, device, WHAT, _shapes)
    normals = normals_device(v, f, dev)[0]
    return normals if isinstance(vertices, torch.Tensor) else normals.cpu().numpy()


def accumulate_device(vertices, normals, faces, dev, cams, images, acc, seen, options, members=None):
    """Step 3 for views of ONE size: rasterises the mesh into the views, a chunk at a time, and adds them to acc and seen.
    cams (V,2,4,4) float64, images a list of V (H,W,3) uint8 arrays or tensors; `members` picks the views, ascending."""
    import torch
    from . import _lib
    from .render import projection_tables
    from .render_mesh import RasterPlan
    min_cos, power, rel, min_depth, chunk = options
    members = list(range(len(images))) if members is None else list(members)
    M = int(vertices.shape[0])
    h, w = (int(s) for s in images[members[0]].shape[:2])
    lib = _lib.load()
    order = "voxel"
    with torch.cuda.device(dev):
        for at in range(0, len(members), chunk):
            part = members[at:at + chunk]
            c = cams[part]
            plan = RasterPlan(vertices, faces, c, h, w, min_depth=min_depth, cull=None, order="voxel" if isinstance(order, str) else None,
                              device=dev)
            if isinstance(order, str):
                order = plan.order                                             # the first chunk's processing order serves them all
            depth = plan.run(order=order, index=False)[0]
            im = torch.stack([x.to(dev) if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x)).to(dev)
                              for x in (images[k] for k in part)]).contiguous()
            proj = torch.as_tensor(projection_tables(c)).to(dev)
            centres = torch.as_tensor(camera_centres(c)).to(dev)
            rc = lib.mvs_mesh_colour_accumulate_f32(_lib.ptr(vertices), _lib.ptr(normals), M, _lib.ptr(proj), _lib.ptr(centres), len(part),
                                                    h, w, _lib.ptr(depth), _lib.ptr(im), min_depth, occlusion_ratio(rel), min_cos, power,
                                                    _lib.ptr(acc), _lib.ptr(seen), _lib.stream_ptr())
            _lib.check(rc, "mvs_mesh_colour_accumulate_f32")
            # the chunk's tensors are freed in stream order (torch's caching allocator), so the next chunk may reuse them


def colour_device(vertices, colours, faces, dev, cams, images, min_cos=0.2, angle_power=2, occlusion_rel=0.01, min_depth=0.0,
                  view_chunk=8, state=None):
    """colour_mesh on contiguous device tensors -> (vertices, colours, faces, report): vertices and faces are the ones that came
    in, the colours a new (M,3) uint8 tensor.  Everything is enqueued on torch's current stream; the read-back of the counts
    comes last (RasterPlan synchronises once, for the processing order of the faces).  state, a dict, leaves the call holding
    the device tensors normals (M,3), acc (M,4) and seen (M); given again with further views of the same mesh, the call continues
    its sums, as TsdfVolume.integrate continues a volume: the colours are then those of all the views so far."""
    import torch
    from . import _lib
    from .render import size_groups
    options = check_options(min_cos, angle_power, occlusion_rel, min_depth, view_chunk)
    M, F = _shapes(vertices, colours, faces)
    cams, images, views = _view_list(cams, images)
    lib = _lib.load()
    with torch.cuda.device(dev):
        normals, ws = normals_device(vertices, faces, dev)
        if state is not None and "acc" in state:
            acc, seen = state["acc"], state["seen"]
            if tuple(acc.shape) != (M, 4) or acc.dtype != torch.float64 or tuple(seen.shape) != (M,) or seen.dtype != torch.int32:
                raise ValueError("state holds the sums of another mesh")
        else:
            acc = torch.zeros((M, 4), dtype=torch.float64, device=dev)
            seen = torch.zeros(M, dtype=torch.int32, device=dev)
        if state is not None:
            state.update(normals=normals, acc=acc, seen=seen)
        if M and F:
            for _, members in size_groups(views):
                accumulate_device(vertices, normals, faces, dev, cams, images, acc, seen, options, members)
        out = torch.empty((M, 3), dtype=torch.uint8, device=dev)
        _lib.check(lib.mvs_mesh_colour_finish_u8(_lib.ptr(colours), _lib.ptr(acc), _lib.ptr(seen), M, _lib.ptr(out), _lib.ptr(ws.t), ws.bytes,
                                                 _lib.stream_ptr()), "mvs_mesh_colour_finish_u8")
        invalid, zero, unseen = (int(c) for c in ws.t[:12].view(torch.int32).cpu().numpy())          # the one read-back
    report = dict(zip(REPORT_FIELDS, (M, F, invalid, zero, unseen, len(views)) + options))
    return vertices, out, faces, report


def colour_mesh(vertices, colours, faces, cams, images, device=None, **options):
    """-> (vertices (M,3) float32, colours (M,3) uint8, faces (F,3) int32, report): numpy arrays, or tensors on the device when
    the vertices came as a tensor.  cams (V,2,4,4) at the images' scale; images (V,H,W,3) uint8 or a list of (H,W,3), of any
    sizes; options as check_options takes them, and colour_device's state."""
    check_options(**{k: v for k, v in options.items() if k != "state"})        # before any GPU work
    _shapes(vertices, colours, faces)                                          # the mesh before the views; no shape: AttributeError
    _view_list(cams, images)
    return run(vertices, colours, faces, device, WHAT, lambda dev, v, c, f: colour_device(v, c, f, dev, cams, images, **options), _shapes)


# ------------------------------------------------------------------------------------------------ command line

def add_options(ap, prefix=""):
    """--recolour and its three numeric companions, as mesh.py and depthfusion.py take them (there under a prefix) -> their
    actions."""
    return [ap.add_argument("--%srecolour" % prefix, action="store_true",
                            help="take the mesh's vertex colours from the full-resolution images, as the last stage (mvsnet_amd.mesh_colour)"),
            ap.add_argument("--%srecolour_min_cos" % prefix, type=float, default=0.2, help="recolouring: a view counts from this cosine to the normal on"),
            ap.add_argument("--%srecolour_angle_power" % prefix, type=int, default=2, help="recolouring: a view weighs by the cosine to this power, 0 .. 8"),
            ap.add_argument("--%srecolour_occlusion_rel" % prefix, type=float, default=0.01,
                            help="recolouring: a vertex this much (relative) behind the rasterised surface is hidden")]


def check_arguments(a, prefix=""):
    """The options of add_options on a parsed namespace -> dict(min_cos, angle_power, occlusion_rel), or None without
    --recolour (the three are then checked all the same); ValueError naming the flags otherwise."""
    get = lambda name: getattr(a, "%srecolour%s" % (prefix, name))
    try:
        min_cos, power, rel, _, _ = check_options(get("_min_cos"), get("_angle_power"), get("_occlusion_rel"))
    except ValueError as e:
        raise ValueError("--%srecolour_min_cos, --%srecolour_angle_power, --%srecolour_occlusion_rel: %s" % ((prefix,) * 3 + (e,)))
    return dict(min_cos=min_cos, angle_power=power, occlusion_rel=rel) if get("") else None


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="input PLY: a triangle mesh, with or without colours")
    ap.add_argument("--out", required=True, help="output PLY")
    ap.add_argument("--mesh_scale", type=float, default=1.0, help="multiply the mesh's coordinates by this to meet the cameras (1000: metres -> mm)")
    ap.add_argument("--transform", default=None, help="4x4 transform file (as mvsnet_amd.register writes it), applied after the scale")
    tgt = ap.add_mutually_exclusive_group(required=True)
    tgt.add_argument("--session", default=None, help="session folder: cameras/<i>.json, images/<i>.jpg at their own size")
    tgt.add_argument("--dense_folder", default=None, help="dense folder: depths_mvsnet/<idx>.txt, <idx>_init.pfm, <idx>.jpg")
    ap.add_argument("--min_cos", type=float, default=0.2, help="a view counts from this cosine between the normal and the ray on")
    ap.add_argument("--angle_power", type=int, default=2, help="a view weighs by the cosine to this power, 0 .. %d" % MAX_POWER)
    ap.add_argument("--occlusion_rel", type=float, default=0.01, help="a vertex this much (relative) behind the rasterised surface is hidden")
    ap.add_argument("--min_depth", type=float, default=0.0, help="a view does not see a vertex at or below this depth")
    ap.add_argument("--view_chunk", type=int, default=8, help="views rasterised at a time")
    ap.add_argument("--write_normals", action="store_true", help="write the vertex normals too: x y z nx ny nz red green blue")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    try:
        a.min_cos, a.angle_power, a.occlusion_rel, a.min_depth, a.view_chunk = check_options(a.min_cos, a.angle_power, a.occlusion_rel,
                                                                                             a.min_depth, a.view_chunk)
        if not (a.mesh_scale > 0 and math.isfinite(a.mesh_scale)):
            raise ValueError("mesh_scale must be positive and finite, got %r" % (a.mesh_scale,))
    except ValueError as e:
        raise SystemExit("mvsnet_amd.mesh_colour: --%s" % e)
    return a


def prepare_output(a):
    return refuse_existing("mesh_colour", a.out, a.force)


def load_views(a):
    """-> (cams (V,2,4,4) float64 at the images' scale, [image (H,W,3) uint8]) of the session or the dense folder."""
    if a.session is not None:
        from PIL import Image
        from .render import session_views
        views = session_views(a.session)
        images = [np.asarray(Image.open(os.path.join(a.session, "images", "%d.jpg" % i)).convert("RGB")) for i, _, _ in views]
        return np.stack([np.asarray(cam, np.float64) for _, cam, _ in views]), images
    from . import fusion
    _, depths, _, cams, images = fusion.load_dense_folder(a.dense_folder)
    if images is None:
        raise ValueError("%s holds no <idx>.jpg" % os.path.join(a.dense_folder, "depths_mvsnet"))
    return scale_cams(cams, depths.shape[1:3], images.shape[1:3]), [images[k] for k in range(len(images))]


def main(argv=None):
    a = parse_args(argv)
    out = prepare_output(a)
    need_gpu("mesh_colour")
    import torch
    from . import _lib
    from .mesh import write_mesh_ply
    from .mesh_sample import read_ply_mesh
    try:
        cams, images = load_views(a)
        vertices, colours, faces = read_ply_mesh(a.mesh)
        dev = _lib.device(None, WHAT)
        with torch.cuda.device(dev):
            own = t = torch.as_tensor(np.ascontiguousarray(vertices, np.float32)).to(dev)
            if a.mesh_scale != 1.0:
                t = (t.double() * a.mesh_scale).float().contiguous()
            if a.transform:
                from .evaluate import _transform
                from .register import read_transform
                t = _transform(t, read_transform(a.transform))
            c = None if colours is None else torch.as_tensor(np.ascontiguousarray(colours, np.uint8)).to(dev)
            f = torch.as_tensor(np.ascontiguousarray(faces, np.int32)).to(dev)
            _, rgb, _, report = colour_device(t, c, f, dev, cams, images, a.min_cos, a.angle_power, a.occlusion_rel, a.min_depth, a.view_chunk)
            rgb = rgb.cpu().numpy()
            normals = normals_device(own, f, dev)[0].cpu().numpy() if a.write_normals else None     # of the positions that are written
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        if normals is not None:
            write_mesh_ply_normals(out, vertices, normals, rgb, faces)         # the positions are the input's own
        else:
            write_mesh_ply(out, vertices, rgb, faces)
    except (ValueError, OSError) as e:
        raise SystemExit("mvsnet_amd.mesh_colour: %s" % e)
    print(json.dumps(dict(report, out=out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
