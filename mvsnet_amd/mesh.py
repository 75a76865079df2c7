"""From depth maps to a surface on the MI355X: TSDF fusion of a session's depth maps into a volume and extraction of a triangle
mesh by naive surface nets, the last stage between the depth maps and a model that can be published.

    python -m mvsnet_amd.mesh --dense_folder DIR [--out mesh.ply] [--voxel S | --resolution R] [--bounds x0:y0:z0:x1:y1:z1]
        [--trunc_voxels 4] [--prob_threshold 0.8] [--num_consistent 3] [--min_count 1] [--fusion_sources all|listed] [--force]
        [--min_component_faces 0] [--min_component_extent 0] [--keep_largest 0] [--simplify_voxels S]
        [--smooth_iterations N [--smooth_lambda 0.5] [--smooth_mu -0.53] [--smooth_boundary fixed|curve|free] [--smooth_max_voxels 1]]
        [--eval_gt G.ply --eval_spacing s [--eval_max_dist 20] [--eval_thresholds 0.5,1,2]]

The kernels are csrc/tsdf.hip (mvs_tsdf_integrate_f32, mvs_surface_nets_count_f32, mvs_surface_nets_write_f32); torch owns the
device memory and the two scans between counting and writing.

Semantics (shared by the kernels, tests/mesh_reference.py and the tests).  Conventions are fusion.py's and render.py's: cam
(2,4,4) with E = cam[0] world -> camera and K = cam[1][:3,:3]; pixel (x, y) is column x, row y at integer coordinates; views
of one call share one size H x W; P_v = K_v [R_v | t_v] is composed in float64 and rounded to float32 once
(``render.projection_tables``).  All device arithmetic is float32 with every product, sum and quotient rounded on its own (no
fused multiply-add, correctly rounded divisions), so float32 numpy and the kernels agree byte for byte.
  * Volume: nx x ny x nz nodes, node (i, j, k) at linear index (k ny + j) nx + i, at most 2^31 - 1 of them.  Its position
    per axis is o + s float(i): a rounded product, then a rounded sum.  Per node the volume holds sum (float32), count
    (int32) and, with colour, rgb_sum (3 x uint32) and rgb_count (int32).
  * Integration: the views of one call in ascending order; a later call continues the same sums.  For node p and view v:
    (u, v, w) are the three rows r = ((P0 X + P1 Y) + P2 Z) + P3 of render.py.  The node is a candidate when w is finite and
    w > 0; fx = floor(u / w + 0.5) and fy likewise must be finite and inside [0, W - 1] x [0, H - 1], compared in float;
    d = df[v, fy, fx] must be > 0, where df is the filtered depth: D where D > 0, finite and prob >= prob_threshold, else 0.
    sdf = d - w; the observation is dropped when sdf < -trunc.  Otherwise t = min(sdf / trunc, 1), sum += t, count += 1.
    Colour, when images are given and sdf <= trunc: the nearest image pixel is ((2 fx + 1) W_img) // (2 W), likewise in y
    (fusion.py's rule, in integers); its three bytes are added to rgb_sum and rgb_count += 1.
  * A node is observed when count >= min_count (default 1); its value is f = sum / float(count); it is inside when it is
    observed and f < 0 (so f == 0 is outside).
  * Surface nets.  Cell (i, j, k), 0 <= i < nx - 1 and so on, has linear index (k (ny - 1) + j) (nx - 1) + i and the corners
    (i + dx, j + dy, k + dz).  A cell is valid when all 8 corners are observed, active when it is valid and its corners are
    neither all inside nor all outside.  Each active cell has one vertex; its id is the cell's rank among the active cells
    in ascending linear index.
  * Vertex position: for axis a = 0, 1, 2 with b = (a + 1) mod 3, c = (a + 2) mod 3, the four cell edges along a in the order
    (off_c, off_b) = (0,0), (0,1), (1,0), (1,1).  An edge from its lower corner A to its upper corner B crosses when
    inside(A) != inside(B); it then has tau = f_A / (f_A - f_B) and adds the local point (tau on a, off_b on b, off_c on c)
    to a float32 accumulator, in that order, and 1 to m.  local = acc / float(m); the coordinate on each axis is
    o + s (float(i) + local).
  * Vertex colour: R = sum of rgb_sum and n = sum of rgb_count over the 8 corners; the byte is (2 R + n) // (2 n), 0 when
    n = 0 (and without colour).
  * Faces: a node edge along axis a from q to q + e_a with both ends observed and inside(q) != inside(q + e_a) has the four
    cells c0 = q - e_b - e_c, c1 = q - e_c, c2 = q, c3 = q - e_b.  When all four exist and are valid, the edge gives the
    triangles (c0, c1, c2), (c0, c2, c3) if inside(q), else (c0, c2, c1), (c0, c3, c2): normals point from inside to
    outside, towards the cameras.  Faces are ordered by the node index of q ascending, then axis, then the two triangles.
  * Outputs: vertices (M,3) float32, colours (M,3) uint8, faces (F,3) int32.

The mesh of a session (``mesh_depth_maps``, the command line): the depth maps are first masked to the pixels the project's
geometric-consistency fusion keeps (``consistency_masks``: fusion.py's criteria without dedupe), which removes the outliers
the probability filter lets through; num_consistent = 0 leaves the probability filter alone.  Default bounds are the box of
the fusion's kept points, widened by trunc plus one voxel.

Small pieces: with min_component_faces, min_component_extent or keep_largest non-zero the extracted mesh goes through
mvsnet_amd.mesh_clean (its docstring has the semantics) on the device, before the copy to the host; with all three at 0
nothing of it runs and the mesh is the extraction's, byte for byte.

Less noise: with smooth_iterations = N > 0 the mesh, after the removal of its small pieces and before any simplification, goes
through mvsnet_amd.mesh_smooth (its docstring has the semantics) on the device: N Taubin iterations with smooth_lambda and
smooth_mu, boundary vertices treated as smooth_boundary says, and no coordinate farther than float32(smooth_max_voxels voxel)
from where the extraction put it.  With 0 nothing of it runs and the mesh bytes are unchanged.

Fewer faces: with simplify_voxels = S > 0 (not necessarily an integer) the mesh, after the removal of its small pieces, goes
through mvsnet_amd.mesh_simplify (its docstring has the semantics) on the device: vertex clustering in cells of
float32(S voxel), aligned to the volume's origin.  Without it nothing of it runs and the mesh bytes are unchanged.

A score: with eval_gt (a ground-truth cloud, PLY) and eval_spacing = s the mesh, as it is written (after the removal of small
pieces, the smoothing and the simplification), is evaluated by its surface samples at spacing s (mvsnet_amd.mesh_sample, then
mvsnet_amd.evaluate) and the metrics go to mesh_metrics.json beside the PLY.  Without them nothing of it runs.

Colour from the images: with recolour the mesh, as the last stage (after the removal of small pieces, the smoothing and the
simplification), takes its vertex colours from the full-resolution images through mvsnet_amd.mesh_colour (its docstring has the
semantics): a weighted mean over the views that see each vertex, occlusion resolved by the rasteriser.  Without it nothing of it
runs and the mesh bytes are unchanged.
"""
from __future__ import annotations

import argparse
import collections
import ctypes
import json
import math
import os
import sys

import numpy as np

from . import mesh_clean, mesh_colour, mesh_simplify, mesh_smooth
from .mesh_common import need_gpu, refuse_existing

MAX_NODES = 2 ** 31 - 1

MESH_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                   "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                   "property list uchar int vertex_indices\nend_header\n")
_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def check_volume(origin, voxel, dims, trunc):
    """-> (origin (3,) float32, voxel, dims (nx, ny, nz), trunc) as the kernels take them; ValueError otherwise."""
    o = np.asarray(origin, np.float64).reshape(-1)
    with np.errstate(over="ignore"):
        o32 = o.astype(np.float32)
    if o.shape != (3,) or not np.isfinite(o32).all():
        raise ValueError("origin must be three finite numbers, got %r" % (origin,))
    v32, t32 = float(np.float32(voxel)), float(np.float32(trunc))
    if not (v32 > 0 and math.isfinite(v32)):
        raise ValueError("voxel must be positive and finite, got %r" % (voxel,))
    if not (t32 > 0 and math.isfinite(t32)):
        raise ValueError("trunc must be positive and finite, got %r" % (trunc,))
    try:
        d = tuple(dims)
        if len(d) != 3 or any(isinstance(n, bool) or int(n) != n or int(n) < 1 for n in d):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("dims must be three positive integers (nx, ny, nz), got %r" % (dims,))
    d = tuple(int(n) for n in d)
    if d[0] * d[1] * d[2] > MAX_NODES:
        raise ValueError("a volume of %d x %d x %d nodes is beyond the kernels' int32 indices" % d)
    return o32, v32, d, t32


def check_min_count(min_count):
    if isinstance(min_count, bool) or int(min_count) != min_count or int(min_count) < 1:
        raise ValueError("min_count must be a positive integer, got %r" % (min_count,))
    return int(min_count)


def choose_volume(lo, hi, voxel=None, resolution=256, margin=0.0, margin_voxels=0.0):
    """A volume around the box [lo, hi] widened on every side by margin + margin_voxels * voxel, in float64
    -> (origin (3,), voxel, dims (nx, ny, nz)).  With a voxel, dims follow; without one, the voxel is chosen so that the
    longest axis has `resolution` nodes.  Every axis gets at least two nodes."""
    lo, hi = np.asarray(lo, np.float64).reshape(-1), np.asarray(hi, np.float64).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (hi < lo).any():
        raise ValueError("bounds must be finite with lo <= hi, got %r and %r" % (lo, hi))
    margin, margin_voxels = float(margin), float(margin_voxels)
    if not (margin >= 0 and margin_voxels >= 0 and math.isfinite(margin) and math.isfinite(margin_voxels)):
        raise ValueError("margins must be >= 0 and finite")
    extent = float((hi - lo).max()) + 2 * margin
    if voxel is None:
        if isinstance(resolution, bool) or int(resolution) != resolution or int(resolution) < 2:
            raise ValueError("resolution must be an integer >= 2, got %r" % (resolution,))
        steps = int(resolution) - 1 - 2 * margin_voxels
        if not (steps > 0 and extent > 0):
            raise ValueError("no voxel fits: resolution %r, margin of %r voxels, extent %r" % (resolution, margin_voxels, extent))
        voxel = extent / steps
    voxel = float(voxel)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError("voxel must be positive and finite, got %r" % (voxel,))
    pad = margin + margin_voxels * voxel
    origin = lo - pad
    dims = tuple(int(max(2, math.ceil(float(e) / voxel - 1e-9) + 1)) for e in (hi + pad - origin))
    if dims[0] * dims[1] * dims[2] > MAX_NODES:
        raise ValueError("a volume of %d x %d x %d nodes is beyond the kernels' int32 indices" % dims)
    return origin, voxel, dims


def write_mesh_ply(path, vertices, colours, faces):
    """Binary little-endian PLY: vertex x y z float, red green blue uchar; face list uchar int vertex_indices."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    if len(vertices) != len(colours):
        raise ValueError("vertices and colours differ in length")
    if len(faces) and (faces.min() < 0 or faces.max() >= len(vertices)):
        raise ValueError("faces name a vertex outside 0..%d" % (len(vertices) - 1))
    v = np.empty(len(vertices), _VERTEX_DTYPE)
    v["x"], v["y"], v["z"] = vertices[:, 0], vertices[:, 1], vertices[:, 2]
    v["red"], v["green"], v["blue"] = colours[:, 0], colours[:, 1], colours[:, 2]
    f = np.empty(len(faces), _FACE_DTYPE)
    f["n"], f["v"] = 3, faces
    with open(path, "wb") as out:
        out.write((MESH_PLY_HEADER % (len(v), len(f))).encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def read_mesh_ply(path):
    """Reads what write_mesh_ply writes -> (vertices (M,3) float32, colours (M,3) uint8, faces (F,3) int32)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii")
    try:
        m = int(head.split("element vertex ")[1].split("\n")[0])
        nf = int(head.split("element face ")[1].split("\n")[0])
    except (IndexError, ValueError):
        raise ValueError("%s: not a PLY written by write_mesh_ply" % path)
    if head != MESH_PLY_HEADER % (m, nf) or len(data) != end + m * _VERTEX_DTYPE.itemsize + nf * _FACE_DTYPE.itemsize:
        raise ValueError("%s: not a PLY written by write_mesh_ply" % path)
    v = np.frombuffer(data, _VERTEX_DTYPE, count=m, offset=end)
    f = np.frombuffer(data, _FACE_DTYPE, count=nf, offset=end + m * _VERTEX_DTYPE.itemsize)
    if nf and (f["n"] != 3).any():
        raise ValueError("%s: a face is not a triangle" % path)
    return (np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32), np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.uint8),
            np.ascontiguousarray(f["v"]).astype(np.int32).reshape(-1, 3))


def parse_bounds(text):
    """"x0:y0:z0:x1:y1:z1" -> (lo (3,), hi (3,)) float64."""
    tok = str(text).split(":")
    try:
        if len(tok) != 6:
            raise ValueError
        b = np.array([float(t) for t in tok])
    except ValueError:
        raise ValueError("bounds %r: x0:y0:z0:x1:y1:z1 expected" % (text,))
    if not np.isfinite(b).all() or (b[3:] <= b[:3]).any():
        raise ValueError("bounds %r: finite numbers with x0 < x1, y0 < y1, z0 < z1 expected" % (text,))
    return b[:3], b[3:]


def _check_views(depths, probs, cams, images):
    """The shapes of one integrate call -> (V, H, W); ValueError otherwise.  Works on numpy arrays and tensors alike."""
    ds, ps = tuple(depths.shape), tuple(probs.shape)
    if len(ds) != 3 or ps != ds or 0 in ds:
        raise ValueError("depths and probs must be (V,H,W) of one size, got %s and %s" % (ds, ps))
    if tuple(cams.shape) != (ds[0], 2, 4, 4):
        raise ValueError("cams must be (%d,2,4,4), got %s" % (ds[0], tuple(cams.shape)))
    if images is not None:
        s = tuple(images.shape)
        if len(s) != 4 or s[0] != ds[0] or s[3] != 3 or 0 in s:
            raise ValueError("images must be (%d,H,W,3) uint8, got %s" % (ds[0], s))
    return ds


# ------------------------------------------------------------------------------------------------ the stages after the extraction

# One row per stage, in the order in which the stages run.  Everything else that knows the chain is a loop over this table:
# TsdfVolume.extract, _mesh_depth_maps, the parser and parse_args below, and depthfusion.py's --mesh_* flags.  A stage's module
# has add_options(ap, prefix) -> its actions, check_arguments(namespace, prefix) -> its options in the units the flags carry
# (voxels) or None when it is off, check_options and a device function (vertices, colours, faces, dev, *arguments) ->
# (vertices, colours, faces, report); the row adds what only this file knows, the volume:
#   key        where the stage's report goes in the merged report (None: its fields at top level)
#   since      the stages by age, which is the order of their flags in --help and of their checks (FLAG_ORDER)
#   keywords   check_arguments' options -> the keywords of mesh_depth_maps and mesh_dense_folder that ask for the same
#   options    those keywords (popped from a dict, absent ones at their defaults), and the images -> the options, checked, or None
#   world      (volume, options, (cams, images, depth size)) -> what extract takes under the stage's name, in world units
#   arguments  (volume, that value) -> the checked arguments of the device function
Stage = collections.namedtuple("Stage", "name module device key since keywords options world arguments")


def _clean_options(kw, images):
    o = mesh_clean.check_options(kw.pop("min_component_faces", 0), kw.pop("min_component_extent", 0.0), kw.pop("keep_largest", 0))
    return dict(zip(mesh_clean.OPTION_NAMES, o)) if mesh_clean.wanted(*o) else None


def _smooth_options(kw, images):
    iterations = mesh_smooth.check_iterations(kw.pop("smooth_iterations", 0), least=0)
    lam, mu, boundary, max_voxels = (kw.pop("smooth_" + name, default) for name, default in
                                     (("lambda", 0.5), ("mu", -0.53), ("boundary", "fixed"), ("max_voxels", 1.0)))
    if not iterations:
        return None
    max_voxels = mesh_smooth.check_voxels(max_voxels)
    mesh_smooth.check_options(iterations, lam, mu, boundary)
    return dict(iterations=iterations, lam=lam, mu=mu, boundary=boundary, max_voxels=max_voxels)


def _simplify_options(kw, images):
    voxels = mesh_simplify.check_voxels(kw.pop("simplify_voxels", None))
    return None if voxels is None else dict(voxels=voxels)


def _recolour_options(kw, images):
    o = kw.pop("recolour", None)
    if o is None or o is False:
        return None
    o = {} if o is True else dict(o)
    mesh_colour.check_options(**o)
    if images is None:
        raise ValueError("recolour needs the images")
    return o


def _recolour_world(vol, o, views):
    """The cameras brought to each image's own size."""
    cams, images, size = views
    at = [tuple(int(n) for n in im.shape[:2]) for im in images]
    scaled = np.stack([mesh_colour.scale_cams(np.asarray(cams, np.float64)[k:k + 1], size, at[k])[0] for k in range(len(at))])
    return dict(o, cams=scaled, images=images)


def _recolour_arguments(vol, o):
    o = dict(o)
    cams, images, _ = mesh_colour._view_list(o.pop("cams"), o.pop("images"))
    return (cams, images) + mesh_colour.check_options(**o)


STAGES = (
    Stage("clean", mesh_clean, mesh_clean.clean_device, None, 1,
          lambda o: dict(min_component_faces=o["min_faces"], min_component_extent=o["min_extent"], keep_largest=o["keep_largest"]),
          _clean_options, lambda vol, o, views: o, lambda vol, o: mesh_clean.check_options(**o)),
    Stage("smooth", mesh_smooth, mesh_smooth.smooth_device, "smooth", 3,
          lambda o: dict(smooth_iterations=o["iterations"], smooth_lambda=o["lam"], smooth_mu=o["mu"], smooth_boundary=o["boundary"],
                         smooth_max_voxels=o["max_voxels"]),
          _smooth_options,
          lambda vol, o, views: dict(iterations=o["iterations"], lam=o["lam"], mu=o["mu"], boundary=o["boundary"],
                                     max_displacement=float(np.float32(o["max_voxels"] * vol.voxel))),
          lambda vol, o: mesh_smooth.check_options(**o)),
    Stage("simplify", mesh_simplify, mesh_simplify.simplify_device, "simplify", 2,
          lambda o: dict(simplify_voxels=o["voxels"]), _simplify_options,
          lambda vol, o, views: float(np.float32(o["voxels"] * vol.voxel)),    # the cell; extract aligns it to the volume's origin
          lambda vol, cell: mesh_simplify.check_options(cell, vol.origin)),
    Stage("recolour", mesh_colour, mesh_colour.colour_device, "recolour", 4,
          lambda o: dict(recolour=o), _recolour_options, _recolour_world, _recolour_arguments),
)
FLAG_ORDER = tuple(sorted(STAGES, key=lambda stage: stage.since))


def stage_keywords(options):
    """{stage name: check_arguments' options or None} -> the keywords of mesh_depth_maps and mesh_dense_folder that ask for it."""
    out = {}
    for stage in STAGES:
        if options.get(stage.name) is not None:
            out.update(stage.keywords(options[stage.name]))
    return out


# ------------------------------------------------------------------------------------------------ device side

class TsdfVolume:
    """A volume on the device.  ``integrate`` may be called repeatedly (a session can be fed in groups of views) and only
    enqueues on torch's current stream; ``extract`` synchronises once, to size its outputs."""

    def __init__(self, origin, voxel, dims, trunc, colour=False, device=None):
        import torch
        from . import _lib
        self.origin, self.voxel, self.dims, self.trunc = check_volume(origin, voxel, dims, trunc)      # before any GPU work
        self.colour = bool(colour)
        self.dev = _lib.device(device, "TSDF fusion")
        nx, ny, nz = self.dims
        self._origin_c = (ctypes.c_float * 3)(*[float(v) for v in self.origin])
        with torch.cuda.device(self.dev):
            self.sum = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.dev)
            self.count = torch.zeros((nz, ny, nx), dtype=torch.int32, device=self.dev)
            self.rgb_sum = self.rgb_count = None
            if self.colour:
                # torch has no uint32 arithmetic to speak of: the kernel's uint32 sums live in an int32 tensor
                self.rgb_sum = torch.zeros((nz, ny, nx, 3), dtype=torch.int32, device=self.dev)
                self.rgb_count = torch.zeros((nz, ny, nx), dtype=torch.int32, device=self.dev)
        self._workspace = None

    def _views(self, x, name, dtype):
        import torch
        if isinstance(x, torch.Tensor):
            if x.dtype != dtype:
                raise ValueError("%s must be %s, got %s" % (name, dtype, x.dtype))
            return x.to(self.dev).contiguous()
        return torch.as_tensor(x).to(self.dev)

    def integrate(self, depths, probs, cams, images=None, prob_threshold=0.8):
        """Adds V views, in ascending order, to the volume.  depths, probs: (V,H,W) float32 arrays, tensors or lists of
        (H,W); cams (V,2,4,4); images None or (V,Hi,Wi,3) uint8, used only by a volume made with colour."""
        import torch
        from . import _lib
        from .fusion import FusionPlan
        from .render import projection_tables
        pt = float(prob_threshold)
        if math.isnan(pt):
            raise ValueError("prob_threshold must not be NaN")
        depths, probs = FusionPlan._host(depths, "depth maps", np.float32), FusionPlan._host(probs, "probability maps", np.float32)
        images = None if images is None or not self.colour else FusionPlan._host(images, "images", np.uint8)
        cams = np.asarray(cams.cpu().numpy() if hasattr(cams, "cpu") else cams, np.float64)
        V, H, W = _check_views(depths, probs, cams, images)
        lib = _lib.load()
        nx, ny, nz = self.dims
        with torch.cuda.device(self.dev):
            d, p = self._views(depths, "depth maps", torch.float32), self._views(probs, "probability maps", torch.float32)
            im = None if images is None else self._views(images, "images", torch.uint8)
            proj = torch.as_tensor(projection_tables(cams)).to(self.dev)
            wsb = lib.mvs_tsdf_integrate_workspace_bytes(V, H, W)
            if wsb == 0:
                raise ValueError("integrate: %d views of %d x %d are beyond the kernel's index range" % (V, H, W))
            if self._workspace is None or self._workspace.numel() < wsb:
                self._workspace = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
            rc = lib.mvs_tsdf_integrate_f32(
                _lib.ptr(d), _lib.ptr(p), V, H, W, _lib.ptr(proj), _lib.ptr(im), im.shape[1] if im is not None else 0,
                im.shape[2] if im is not None else 0, self._origin_c, self.voxel, nx, ny, nz, self.trunc, pt, 0,
                _lib.ptr(self.sum), _lib.ptr(self.count), _lib.ptr(self.rgb_sum) if im is not None else None,
                _lib.ptr(self.rgb_count) if im is not None else None, _lib.ptr(self._workspace), self._workspace.numel(),
                _lib.stream_ptr())
            _lib.check(rc, "mvs_tsdf_integrate_f32")
        return self

    def extract(self, min_count=1, clean=None, simplify=None, smooth=None, recolour=None):
        """-> (vertices (M,3) float32, colours (M,3) uint8, faces (F,3) int32) as numpy; one synchronisation.  The keywords
        clean, smooth, simplify and recolour (the names of STAGES; a new stage adds its own here) send the mesh through those stages on the device, in the
        table's order, before the copy to the host; the result is then (vertices, colours, faces, report), the report merged as
        the table says.  Every stage's value is checked before any GPU work.
          clean = dict(min_faces=, min_extent=, keep_largest=): mesh_clean.clean_device.
          smooth = dict(iterations=, lam=, mu=, boundary=, max_displacement=) (mesh_smooth.check_options): mesh_smooth.smooth_device.
          simplify = cell (world units): mesh_simplify.simplify_device with cells aligned to the volume's origin.
          recolour = dict(cams=, images=, and mesh_colour.check_options' options), cams at the images' scale:
          mesh_colour.colour_device."""
        import torch
        from . import _lib
        min_count = check_min_count(min_count)
        given = dict(clean=clean, simplify=simplify, smooth=smooth, recolour=recolour)
        checked = {stage.name: stage.arguments(self, given[stage.name]) for stage in FLAG_ORDER         # before any GPU work
                   if given[stage.name] is not None}
        lib = _lib.load()
        nx, ny, nz = self.dims
        nodes = nx * ny * nz
        cells = max(nx - 1, 0) * max(ny - 1, 0) * max(nz - 1, 0)
        with torch.cuda.device(self.dev):
            wsb = lib.mvs_surface_nets_workspace_bytes(nx, ny, nz)
            ws = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
            totals = torch.empty(2, dtype=torch.int32, device=self.dev)
            rc = lib.mvs_surface_nets_count_f32(_lib.ptr(self.sum), _lib.ptr(self.count), nx, ny, nz, min_count, _lib.ptr(totals),
                                                _lib.ptr(ws), wsb, _lib.stream_ptr())
            _lib.check(rc, "mvs_surface_nets_count_f32")
            words = ws.view(torch.int32)
            face_at = ((max(cells, 1) * 4 + 255) // 256 * 256) // 4
            cell_rank = torch.cumsum(words[:max(cells, 1)] >> 1, 0, dtype=torch.int32)
            face_end = torch.cumsum(words[face_at:face_at + nodes], 0, dtype=torch.int32)
            M, F = (int(v) for v in totals.cpu().numpy())                       # the one synchronisation
            if M < 0 or F < 0:
                raise ValueError("the mesh is beyond int32 indices")
            vertices = torch.empty((M, 3), dtype=torch.float32, device=self.dev)
            colours = torch.empty((M, 3), dtype=torch.uint8, device=self.dev)
            faces = torch.empty((F, 3), dtype=torch.int32, device=self.dev)
            if M:
                rc = lib.mvs_surface_nets_write_f32(
                    _lib.ptr(self.sum), _lib.ptr(self.count), _lib.ptr(self.rgb_sum), _lib.ptr(self.rgb_count), self._origin_c,
                    self.voxel, nx, ny, nz, min_count, _lib.ptr(cell_rank), _lib.ptr(face_end), M, F, _lib.ptr(vertices),
                    _lib.ptr(colours), _lib.ptr(faces) if F else None, _lib.ptr(ws), wsb, _lib.stream_ptr())
                _lib.check(rc, "mvs_surface_nets_write_f32")
            report = None
            for stage in STAGES:
                if stage.name in checked:
                    vertices, colours, faces, r = stage.device(vertices, colours, faces, self.dev, *checked[stage.name])
                    report = dict(report or {}, **(r if stage.key is None else {stage.key: r}))
            mesh = (vertices.cpu().numpy(), colours.cpu().numpy(), faces.cpu().numpy())
            return mesh if report is None else mesh + (report,)

    def tsdf(self):
        """For inspection -> (f (nz,ny,nx) float32 = sum / count, NaN where count is 0, count (nz,ny,nx) int32) as numpy."""
        s, c = self.sum.cpu().numpy(), self.count.cpu().numpy()
        with np.errstate(all="ignore"):
            return np.where(c > 0, s / c.astype(np.float32), np.float32(np.nan)), c

    def state(self):
        """The raw sums as numpy: dict(sum, count, rgb_sum (uint32) or None, rgb_count or None)."""
        return dict(sum=self.sum.cpu().numpy(), count=self.count.cpu().numpy(),
                    rgb_sum=None if self.rgb_sum is None else self.rgb_sum.cpu().numpy().view(np.uint32),
                    rgb_count=None if self.rgb_count is None else self.rgb_count.cpu().numpy())


def _consistency(depths, probs, cams, *, prob_threshold=0.8, reproj_threshold=1.0, depth_rel_threshold=0.01, num_consistent=3,
                 sources=None, device=None):
    from .fusion import FusionPlan
    plan = FusionPlan(depths, probs, cams, None, prob_threshold=prob_threshold, reproj_threshold=reproj_threshold,
                      depth_rel_threshold=depth_rel_threshold, num_consistent=num_consistent, sources=sources, dedupe=False,
                      device=device)
    plan.enqueue()
    xyz, _, view, pixel = plan.result(with_pixels=True)
    masks = np.zeros((plan.V, plan.H * plan.W), bool)
    masks[view, pixel] = True
    return masks.reshape(plan.V, plan.H, plan.W), xyz


def consistency_masks(depths, probs, cams, **options):
    """(V,H,W) bool: the pixels the project's geometric-consistency fusion keeps, every view on its own (dedupe off).
    Options: prob_threshold, reproj_threshold, depth_rel_threshold, num_consistent, sources, device (fusion.FusionPlan's)."""
    return _consistency(depths, probs, cams, **options)[0]


def mesh_depth_maps(depths, probs, cams, images=None, **options):
    """V depth maps -> (vertices (M,3) float32, colours (M,3) uint8, faces (F,3) int32).  Give a voxel or a resolution (nodes
    along the longest axis, 256 when neither is given); bounds (lo, hi) default to the box of the consistent points.  Options:
    voxel, resolution, bounds, trunc_voxels, num_consistent, prob_threshold, reproj_threshold, depth_rel_threshold, sources,
    min_count, device, min_component_faces, min_component_extent, keep_largest (all 0: no cleaning runs), and simplify_voxels
    (None or 0: no simplification runs; S > 0: vertex clustering in cells of float32(S voxel)), and smooth_iterations (0: no
    smoothing runs) with smooth_lambda, smooth_mu, smooth_boundary and smooth_max_voxels (the bound is float32(R voxel)), and
    recolour (None or False: nothing of it runs; True or a dict of mesh_colour.check_options' options: the colours come from
    `images` at their own size, as the last stage, the cameras brought to the images' scale)."""
    return _mesh_depth_maps(depths, probs, cams, images, **options)[:3]


def _mesh_depth_maps(depths, probs, cams, images=None, *, voxel=None, resolution=None, bounds=None, trunc_voxels=4,
                     num_consistent=3, prob_threshold=0.8, reproj_threshold=1.0, depth_rel_threshold=0.01, sources=None,
                     min_count=1, device=None, **stage_options):
    """mesh_depth_maps -> (vertices, colours, faces, the merged report of the stages that ran or None).  stage_options: the
    keywords that STAGES' rows take (`options`)."""
    # before any GPU work; the cleaning's keywords are looked at last here, as they have been since they were the only ones
    options = [(stage, stage.options(stage_options, images)) for stage in FLAG_ORDER[1:] + FLAG_ORDER[:1]]
    if stage_options:
        raise TypeError("mesh_depth_maps() got an unexpected keyword argument %r" % sorted(stage_options)[0])
    from .fusion import FusionPlan
    if voxel is not None and resolution is not None:
        raise ValueError("give a voxel or a resolution, not both")
    tv = float(trunc_voxels)
    if not (tv > 0 and math.isfinite(tv)):
        raise ValueError("trunc_voxels must be positive and finite, got %r" % (trunc_voxels,))
    min_count = check_min_count(min_count)
    if voxel is None and resolution is None:
        resolution = 256
    depths, probs = FusionPlan._host(depths, "depth maps", np.float32), FusionPlan._host(probs, "probability maps", np.float32)
    to_numpy = lambda x: x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    depths, probs = to_numpy(depths), to_numpy(probs)
    xyz = None
    if num_consistent > 0 or bounds is None:
        masks, xyz = _consistency(depths, probs, cams, prob_threshold=prob_threshold, reproj_threshold=reproj_threshold,
                                  depth_rel_threshold=depth_rel_threshold, num_consistent=num_consistent, sources=sources,
                                  device=device)
        if num_consistent > 0:
            depths = np.where(masks, depths, np.float32(0))
    if bounds is None:
        if len(xyz) == 0:
            raise ValueError("no pixel is consistent in %g views: nothing to bound the volume with" % num_consistent)
        lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
        origin, voxel, dims = choose_volume(lo, hi, voxel, resolution, margin_voxels=tv + 1)
    else:
        origin, voxel, dims = choose_volume(bounds[0], bounds[1], voxel, resolution)
    vol = TsdfVolume(origin, voxel, dims, tv * voxel, colour=images is not None, device=device)
    vol.integrate(depths, probs, cams, images, prob_threshold=prob_threshold)
    views = (cams, images, depths.shape[1:3])
    requested = {stage.name: stage.world(vol, o, views) for stage, o in options if o is not None}
    return vol.extract(min_count, **requested) + (() if requested else (None,))


# ------------------------------------------------------------------------------------------------ command line

def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dense_folder", required=True, help="dense folder: depths_mvsnet/<idx>_init.pfm, _prob.pfm, .txt[, .jpg]")
    ap.add_argument("--out", default=None, help="output PLY (default <dense_folder>/points_mvsnet/mesh.ply)")
    size = ap.add_mutually_exclusive_group()
    size.add_argument("--voxel", type=float, default=None, help="node spacing in world units")
    size.add_argument("--resolution", type=int, default=None, help="nodes along the longest axis (256 when no --voxel is given)")
    ap.add_argument("--bounds", default=None, help="x0:y0:z0:x1:y1:z1 (default: the box of the consistent points, widened)")
    ap.add_argument("--trunc_voxels", type=float, default=4.0, help="truncation distance in voxels")
    ap.add_argument("--prob_threshold", type=float, default=0.8)
    ap.add_argument("--num_consistent", type=float, default=3, help="views that must agree on a pixel (0: probability filter alone)")
    ap.add_argument("--min_count", type=int, default=1, help="observations a node needs")
    ap.add_argument("--fusion_sources", choices=("all", "listed"), default="all",
                    help="consistency against every other view, or the neighbours of pair.txt / covisibility.json")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    for stage in FLAG_ORDER:
        stage.module.add_options(ap)
    ap.add_argument("--eval_gt", default=None, help="ground-truth cloud (PLY): evaluate the mesh's surface samples against it "
                    "(mesh_metrics.json beside the output; needs --eval_spacing)")
    from .mesh_sample import add_options as add_sampling
    add_sampling(ap, "eval_")
    ap.add_argument("--eval_max_dist", type=float, default=20.0, help="--eval_gt: distance cap (outliers at or beyond it)")
    ap.add_argument("--eval_thresholds", default="", help="--eval_gt: comma-separated tau for precision / recall / F-score")
    return ap


def parse_args(argv=None):
    """-> the namespace with .bounds parsed and the options checked (SystemExit otherwise)."""
    a = build_parser().parse_args(argv)
    try:
        a.bounds = parse_bounds(a.bounds) if a.bounds is not None else None
        a.min_count = check_min_count(a.min_count)
        if not (a.trunc_voxels > 0 and math.isfinite(a.trunc_voxels)):
            raise ValueError("--trunc_voxels must be positive and finite, got %r" % (a.trunc_voxels,))
        if a.voxel is not None and not (a.voxel > 0 and math.isfinite(a.voxel)):
            raise ValueError("--voxel must be positive and finite, got %r" % (a.voxel,))
        if a.resolution is not None and a.resolution < 2:
            raise ValueError("--resolution must be at least 2, got %r" % (a.resolution,))
        if math.isnan(a.prob_threshold) or not a.num_consistent >= 0:
            raise ValueError("--prob_threshold must be a number and --num_consistent >= 0")
        a.stages = {stage.name: stage.module.check_arguments(a) for stage in FLAG_ORDER}  # None: off, nothing of that stage runs
        if (a.eval_gt is None) != (a.eval_spacing is None):
            raise ValueError("--eval_gt and --eval_spacing go together")
        try:
            a.eval_thresholds = [float(v) for v in a.eval_thresholds.split(",") if v.strip()]
        except ValueError:
            raise ValueError("--eval_thresholds: comma-separated numbers expected, got %r" % (a.eval_thresholds,))
        if a.eval_gt is not None:
            from .evaluate import check_thresholds
            from .mesh_sample import check_spacing
            try:
                check_spacing(a.eval_spacing)
                check_thresholds(a.eval_thresholds, a.eval_max_dist)
            except ValueError as e:
                raise ValueError("--eval_spacing / --eval_max_dist / --eval_thresholds: %s" % e)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.mesh: %s" % e)
    if a.out is None:
        a.out = os.path.join(a.dense_folder, "points_mvsnet", "mesh.ply")
    return a


def prepare_output(a):
    return refuse_existing("mesh", a.out, a.force)


def evaluate_mesh(out, vertices, faces, eval_gt, eval_spacing, eval_max_dist=20.0, eval_thresholds=()):
    """The mesh against the ground-truth cloud eval_gt (a PLY) by its surface samples at eval_spacing -> the metrics, also
    written to mesh_metrics.json beside `out`."""
    from . import evaluate
    gt, _ = evaluate.read_ply_points(eval_gt)
    metrics = evaluate.evaluate_point_clouds(vertices, gt, max_dist=eval_max_dist, thresholds=eval_thresholds, pred_faces=faces,
                                             pred_spacing=eval_spacing)
    with open(os.path.join(os.path.dirname(os.path.abspath(out)), "mesh_metrics.json"), "w") as f:
        f.write(json.dumps(metrics) + "\n")
    return metrics


def mesh_dense_folder(dense_folder, out, *, fusion_sources="all", eval_gt=None, eval_spacing=None, eval_max_dist=20.0,
                      eval_thresholds=(), **options):
    """The dense folder's depth maps -> the PLY at `out`; returns the report the command line prints.  With eval_gt and
    eval_spacing also mesh_metrics.json beside it (evaluate_mesh); the report then names it."""
    from . import fusion
    if (eval_gt is None) != (eval_spacing is None):
        raise ValueError("eval_gt and eval_spacing go together")
    if eval_gt is not None:                                                    # before any GPU work
        from .evaluate import check_thresholds
        from .mesh_sample import check_spacing
        check_spacing(eval_spacing)
        check_thresholds(eval_thresholds, eval_max_dist)
    indices, depths, probs, cams, images = fusion.load_dense_folder(dense_folder)
    sources = fusion.listed_sources(dense_folder, indices) if fusion_sources == "listed" else None
    vertices, colours, faces, cleaned = _mesh_depth_maps(depths, probs, cams, images, sources=sources, **options)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    write_mesh_ply(out, vertices, colours, faces)
    report = {"views": len(indices), "vertices": int(len(vertices)), "faces": int(len(faces)), "out": out}
    if cleaned is not None:
        report.update(cleaned)                                                 # the cleaning's fields (mesh_clean.py, Report)
    if eval_gt is not None:
        evaluate_mesh(out, vertices, faces, eval_gt, eval_spacing, eval_max_dist, eval_thresholds)
        report["mesh_metrics"] = os.path.join(os.path.dirname(os.path.abspath(out)), "mesh_metrics.json")
    return report


def main(argv=None):
    a = parse_args(argv)
    out = prepare_output(a)
    need_gpu("mesh")
    try:
        report = mesh_dense_folder(a.dense_folder, out, fusion_sources=a.fusion_sources, voxel=a.voxel, resolution=a.resolution,
                                   bounds=a.bounds, trunc_voxels=a.trunc_voxels, num_consistent=a.num_consistent,
                                   prob_threshold=a.prob_threshold, min_count=a.min_count, **stage_keywords(a.stages),
                                   **({} if a.eval_gt is None else dict(eval_gt=a.eval_gt, eval_spacing=a.eval_spacing,
                                                                        eval_max_dist=a.eval_max_dist, eval_thresholds=a.eval_thresholds)))
    except (ValueError, OSError) as e:
        raise SystemExit("mvsnet_amd.mesh: %s" % e)
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
