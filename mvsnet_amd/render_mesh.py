"""Rasterisation of a triangle mesh into per-view depth maps on the MI355X: the way from a mesh, mesh.py's own or a
scanner's, back into the cameras.  Where render.py splats points and patches the holes, this draws faces: dense depth maps
without holes or show-through, per pixel the face it shows, and vertex attributes (colour, world position) interpolated per
pixel.

    python -m mvsnet_amd.render_mesh --mesh M.ply [--mesh_scale S] [--transform T.txt] (--session DIR | --dense_folder DIR)
        [--cull back|front] [--min_depth D] [--suffix gt] [--write_index] [--write_color] [--force]

One call is one fused HIP pass (csrc/raster.hip, mvs_raster_mesh_f32): a lane per face loops over the views and over the few
pixels of the face's bounding box, a 64-bit atomic minimum per covered pixel is the z-buffer, and the rare (face, view)
pairs whose box is large go through a queue to a second kernel of the same call, where a workgroup strides over the box.
torch owns the device memory and the sort behind the processing order.

Semantics (shared by the kernels, tests/raster_reference.py and the tests).  Conventions are render.py's: cam (2,4,4); pixel
(x, y) is column x, row y, its centre at integer coordinates; views of one call share one size H x W; P_v = K_v [R_v | t_v]
is composed in float64 and rounded to float32 once (render.projection_tables).
  * Vertex projection.  Vertex j = (X, Y, Z) (float32) in view v, all in float32, every product and sum rounded (no fused
    multiply-add): each row of P_v gives r = ((P0 X + P1 Y) + P2 Z) + P3, the three rows (u, v, w).  The vertex is usable when
    w is finite and w > min_depth (>= 0, default 0).  Screen position sx = u / w, sy = v / w (correctly rounded divisions),
    snapped to 1/256 pixel: qx = floor(sx * 256 + 0.5), qy likewise, in float32.  The vertex is usable only if
    |qx| <= 2^28 and |qy| <= 2^28 (the guard band), compared in float32 before qx, qy are converted to integers.
  * No clipping.  A face is dropped in a view as a whole, nothing of it is drawn and nothing is clipped, when one of its
    vertices is unusable there (non-finite, at or behind min_depth, beyond the guard band), when a vertex index is outside
    0..M-1, or when it has zero area.  The cameras of an MVS session look at the object from outside, so a face that crosses
    the camera plane is not worth a clipper.
  * Setup per (face, view), face (a, b, c), integers in int64: area2 = (xb - xa)(yc - ya) - (yb - ya)(xc - xa); area2 == 0
    drops the face; sgn = sign(area2).  cull: 0 keeps all faces, +1 drops faces with area2 > 0, -1 those with area2 < 0.
    With image y pointing down and positive focal lengths area2 < 0 is a face whose normal (b - a) x (c - a) points at the
    camera; mesh.py's meshes have outward normals, so cull = +1 removes their back faces.  Python spells cull None, "back"
    (+1) or "front" (-1).
  * Coverage.  A pixel (x, y) of the bounding box [ceil(min q / 256), floor(max q / 256)] per axis, intersected with the
    image, has p = (256 x, 256 y).  e_a = sgn [(xc - xb)(py - yb) - (yc - yb)(px - xb)], e_b the same on the edge c -> a and
    e_c on a -> b, so e_a + e_b + e_c = |area2| exactly.  The pixel is covered when every e_i > 0, or e_i == 0 and that edge
    owns its points: an edge of direction d = sgn (end - start) owns them when d_y > 0, or d_y == 0 and d_x < 0.  Two faces
    on the two sides of a shared edge run along it in opposite directions, so exactly one owns it: a mesh has neither cracks
    nor double hits (a grid of vertices on pixel centres k, 2k, ... covers the half-open square (0, n k]^2 once).
  * Depth, perspective-correct, in float64, every operation rounded: i_k = 1.0 / double(w_k), t_k = double(e_k) i_k,
    s = (t_a + t_b) + t_c, z = float32(double(|area2|) / s).  int64 -> double rounds to nearest even.
  * Z-buffer, as render.py's: per pixel the minimum of bits(z) << 32 | face index; the smallest depth wins and exact ties go
    to the smallest face index, whatever the order of execution.  depth (V,H,W) float32, 0 where empty; index (V,H,W)
    int32, -1 where empty.
  * Attribute interpolation.  Given index and attr (M, C) float32, 1 <= C <= 8, a pixel whose index names a face (0..F-1)
    that is not dropped in the view recomputes that face's setup and its e_k at the pixel and gets, per channel,
    float32(((t_a A_a + t_b A_b) + t_c A_c) / s) with A in float64; every other pixel gets 0.  The numerator of a constant
    attribute 1 is s itself, so 1 comes back as exactly 1.0.  ``colors(rgb)`` interpolates uint8 vertex colours this way
    and stores floor(x + 0.5) (float32) clamped to 0..255.
  * The processing order (order="voxel": faces sorted by the voxel key of their first vertex, a stable sort) and the two
    options of the large path, large_pixels and queue_capacity, only decide which lane does what; they never change a byte.

Defaults of the large path (tools/bench_raster.py, profiles/raster_bench.json): large_pixels = 256 and
queue_capacity = 2^16.  A lane's walk costs 1.5 us per step of four views, so 256 pixels bound it at 0.4 ms, a tenth of a
call on 2 M faces and 49 views, while a smaller box would leave most of a workgroup's 256 lanes idle; 2^16 entries are 512 KB.
The sweep over both on a mesh of sub-pixel faces plus a ground plane is flat to 1 %.

Depth files as render.py's: a session's depths/<i>.png holds uint16 millimetres; a dense folder's
depths_mvsnet/<idx>_<suffix>.pfm the float32 map.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

from .render import dense_folder_views, projection_tables, session_views, size_groups, write_depth_png

MAX_AXIS = 1 << 20              # csrc/raster.hip RS_MAX_AXIS
MAX_CHANNELS = 8                # RS_MAX_CHANNELS
LARGE_PIXELS = 256              # a (face, view) box of more pixels goes to the large path
QUEUE_CAPACITY = 1 << 16        # entries of 8 bytes
ORDER_CELL_PIXELS = 4.0         # side of the processing order's voxels, in pixel footprints at the mesh's median depth
CULL = {None: 0, "back": 1, "front": -1}


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def check_options(min_depth=0.0, cull=None, large_pixels=LARGE_PIXELS, queue_capacity=QUEUE_CAPACITY):
    """-> (min_depth, cull as -1 / 0 / 1, large_pixels, queue_capacity); ValueError outside the ranges of the module docstring."""
    md = float(min_depth)
    if not (md >= 0.0 and md <= float(np.finfo(np.float32).max)):               # finite as a float32; a NaN fails both
        raise ValueError("min_depth must be >= 0 and finite, got %r" % (min_depth,))
    if cull is not None and not (isinstance(cull, str) and cull in CULL):
        raise ValueError('cull must be None, "back" or "front", got %r' % (cull,))
    out = []
    for name, v in (("large_pixels", large_pixels), ("queue_capacity", queue_capacity)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 2 ** 31 - 1:
            raise ValueError("%s must be an integer in 0..2^31-1, got %r" % (name, v))
        out.append(int(v))
    return md, CULL[cull], out[0], out[1]


def _array(x, dtype, cols, name):
    """A (n, cols) array of `dtype` (numpy or tensor, left where it is) -> (x, n); ValueError otherwise."""
    import torch
    if isinstance(x, torch.Tensor):
        want = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8}[dtype]
    else:
        x, want = np.asarray(x), np.dtype(dtype)
    if x.dtype != want:
        raise ValueError("%s must be %s, got %s" % (name, np.dtype(dtype).name, x.dtype))
    shape = tuple(x.shape)
    if len(shape) != 2 or (cols is not None and shape[1] != cols) or shape[0] < 1:
        raise ValueError("%s must be (n,%s) with n >= 1, got %s" % (name, cols if cols is not None else "C", shape))
    if shape[0] > 2 ** 31 - 1:
        raise ValueError("%d rows of %s are beyond the kernel's int32 indices" % (shape[0], name))
    return x, int(shape[0])


# ------------------------------------------------------------------------------------------------ device side

class RasterPlan:
    """Mesh and projection tables on the device, outputs and workspace allocated once (the constructor synchronises when it
    computes the processing order).  ``enqueue()`` only launches on torch's current stream (no allocation, no
    synchronisation); ``run()`` enqueues and returns the (depth, index) device tensors, (V,H,W) float32 / int32;
    ``interpolate(attr)`` and ``colors(rgb)`` read ``index`` as the last run left it."""

    def __init__(self, vertices, faces, cams, height, width, *, min_depth=0.0, cull=None, large_pixels=LARGE_PIXELS,
                 queue_capacity=QUEUE_CAPACITY, order="voxel", device=None):
        import torch
        from . import _lib
        self.min_depth, self.cull, self.large_pixels, self.queue_capacity = check_options(min_depth, cull, large_pixels, queue_capacity)
        if order is not None and not (isinstance(order, str) and order == "voxel"):
            raise ValueError('order must be "voxel" or None, got %r' % (order,))
        if int(height) != height or int(width) != width or int(height) < 1 or int(width) < 1:
            raise ValueError("height and width must be positive integers, got %r x %r" % (height, width))
        self.H, self.W = int(height), int(width)
        if self.H > MAX_AXIS or self.W > MAX_AXIS:
            raise ValueError("render_mesh: %d x %d is beyond the guard band (2^20 per axis)" % (self.H, self.W))
        cams = np.asarray(cams.cpu().numpy() if hasattr(cams, "cpu") else cams, np.float64)
        if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4) or cams.shape[0] < 1:
            raise ValueError("cams must be (V,2,4,4), got %s" % (cams.shape,))
        self.V = int(cams.shape[0])
        vertices, self.M = _array(vertices, np.float32, 3, "vertices")
        faces, self.F = _array(faces, np.int32, 3, "faces")
        self.dev = _lib.device(device, "point-cloud rendering")
        lib = _lib.load()
        wsb = lib.mvs_raster_workspace_bytes(self.V, self.H, self.W, self.queue_capacity)
        if wsb == 0:
            raise ValueError("render_mesh: %d views of %d x %d are beyond the kernel's index range" % (self.V, self.H, self.W))
        self.proj_host = projection_tables(cams)
        to_dev = lambda x: (x.to(self.dev) if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x)).to(self.dev)).contiguous()
        with torch.cuda.device(self.dev):
            self.vertices, self.faces = to_dev(vertices), to_dev(faces)
            self.proj = torch.as_tensor(self.proj_host).to(self.dev)
            self.workspace = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
            self.depth = torch.empty((self.V, self.H, self.W), dtype=torch.float32, device=self.dev)
            self.index = torch.empty((self.V, self.H, self.W), dtype=torch.int32, device=self.dev)
            self.order = self._processing_order() if order == "voxel" else None

    def _processing_order(self):
        """Face indices sorted (stable) by the voxel key of the face's first vertex.  The cell is ORDER_CELL_PIXELS pixel
        footprints w / f at the median depth w of a strided sample of the vertices over all views, so the 64 faces of a wave
        fall on neighbouring pixels."""
        import torch
        from . import _lib
        first = self.vertices[self.faces[:, 0].long().clamp(0, self.M - 1)].contiguous()
        good = first[torch.isfinite(first).all(1)]
        if good.shape[0] == 0:
            return None
        lo = good.min(0).values.double().cpu().numpy()
        hi = good.max(0).values.double().cpu().numpy()
        sample = good[::max(1, good.shape[0] // 4096)].double().cpu().numpy()
        P = self.proj_host.astype(np.float64).reshape(self.V, 3, 4)
        w = np.einsum("vk,nk->vn", P[:, 2, :3], sample) + P[:, 2, 3:4]
        f = np.sqrt(np.abs(P[:, 0, 0] * P[:, 1, 1]))[:, None] + 0.0 * w
        ok = (w > self.min_depth) & np.isfinite(w) & (f > 0)
        emax = float(max((hi - lo).max(), 0.0))
        cell = ORDER_CELL_PIXELS * float(np.median(w[ok] / f[ok])) if ok.any() else emax / 1024.0
        cell = max(cell, emax / float(1 << 20))
        if not (cell > 0 and math.isfinite(cell)):
            return None                                                        # one face, or a mesh without extent
        keys = torch.empty(self.F, dtype=torch.int64, device=self.dev)
        _lib.check(_lib.load().mvs_voxel_keys_f32(_lib.ptr(first), self.F, float(lo[0]), float(lo[1]), float(lo[2]), cell,
                                                  _lib.ptr(keys), _lib.stream_ptr()), "mvs_voxel_keys_f32")
        return torch.sort(keys, stable=True)[1].int().contiguous()

    def enqueue(self, *, order="plan", index=True, large_pixels=None, queue_capacity=None):
        """Launches the rasteriser on the plan's device, on torch's current stream of that device.  order: "plan" (the plan's
        processing order), None (input order) or an int32 device tensor holding a permutation of the faces; index=False
        leaves ``self.index`` untouched; large_pixels and queue_capacity (at most the plan's) override the plan's."""
        import torch
        from . import _lib
        order = self.order if isinstance(order, str) and order == "plan" else order
        if order is not None and (not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or order.numel() != self.F):
            raise ValueError("order must be an int32 tensor of %d entries" % self.F)
        _, _, lp, qc = check_options(0.0, None, self.large_pixels if large_pixels is None else large_pixels,
                                     self.queue_capacity if queue_capacity is None else queue_capacity)
        if qc > self.queue_capacity:
            raise ValueError("queue_capacity %d exceeds the plan's %d" % (qc, self.queue_capacity))
        with torch.cuda.device(self.dev):
            rc = _lib.load().mvs_raster_mesh_f32(
                _lib.ptr(self.vertices), self.M, _lib.ptr(self.faces), self.F, _lib.ptr(order), _lib.ptr(self.proj), self.V, self.H,
                self.W, self.min_depth, self.cull, lp, qc, _lib.ptr(self.depth), _lib.ptr(self.index) if index else None,
                _lib.ptr(self.workspace), self.workspace.numel(), _lib.stream_ptr())
        _lib.check(rc, "mvs_raster_mesh_f32")

    def run(self, **kw):
        """enqueue() -> (depth (V,H,W) float32, index (V,H,W) int32): the plan's own device tensors, valid in stream order."""
        self.enqueue(**kw)
        return self.depth, self.index

    def interpolate(self, attr):
        """(V,H,W,C) float32 device tensor: attr (M,C) float32, 1 <= C <= 8, interpolated through ``index`` (of the last run)."""
        import torch
        from . import _lib
        attr, m = _array(attr, np.float32, None, "attr")
        C = int(attr.shape[1])
        if m != self.M or not 1 <= C <= MAX_CHANNELS:
            raise ValueError("attr must be (%d,C) with 1 <= C <= %d, got %s" % (self.M, MAX_CHANNELS, tuple(attr.shape)))
        with torch.cuda.device(self.dev):
            a = (attr.to(self.dev) if isinstance(attr, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(attr)).to(self.dev)).contiguous()
            out = torch.empty((self.V, self.H, self.W, C), dtype=torch.float32, device=self.dev)
            rc = _lib.load().mvs_raster_interpolate_f32(
                _lib.ptr(self.vertices), self.M, _lib.ptr(self.faces), self.F, _lib.ptr(self.proj), self.V, self.H, self.W,
                self.min_depth, _lib.ptr(self.index), _lib.ptr(a), C, _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "mvs_raster_interpolate_f32")
        return out

    def colors(self, rgb):
        """(V,H,W,3) uint8 device tensor: rgb (M,3) uint8 vertex colours interpolated through ``index``, floor(x + 0.5)
        clamped to 0..255; empty pixels are black."""
        import torch
        from . import _lib
        rgb, m = _array(rgb, np.uint8, 3, "rgb")
        if m != self.M:
            raise ValueError("rgb must be (%d,3), got %s" % (self.M, tuple(rgb.shape)))
        c = rgb if isinstance(rgb, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(rgb))
        x = self.interpolate(c.to(self.dev).float())
        return torch.floor(x + 0.5).clamp_(0, 255).to(torch.uint8)


def render_mesh_depth_maps(vertices, faces, cams, height, width, **options):
    """Rasterises the mesh (vertices (M,3) float32, faces (F,3) int32; numpy or device tensors) into the V cameras ->
    (depth (V,H,W) float32, index (V,H,W) int32) as numpy; options as RasterPlan's, semantics in the module docstring."""
    plan = RasterPlan(vertices, faces, cams, height, width, **options)
    depth, index = plan.run()
    return depth.cpu().numpy(), index.cpu().numpy()


# ------------------------------------------------------------------------------------------------ command line

def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="triangle mesh to draw (PLY as mvsnet_amd.mesh writes it)")
    ap.add_argument("--mesh_scale", type=float, default=1.0, help="multiply the mesh's coordinates by this first (1000: metres -> mm)")
    ap.add_argument("--transform", default=None, help="4x4 transform file (as mvsnet_amd.register writes it), applied after the scale")
    tgt = ap.add_mutually_exclusive_group(required=True)
    tgt.add_argument("--session", default=None, help="session folder: cameras/<i>.json, images/<i>.jpg -> depths/<i>.png (uint16 mm)")
    tgt.add_argument("--dense_folder", default=None, help="dense folder: depths_mvsnet/<idx>.txt, <idx>_init.pfm -> <idx>_<suffix>.pfm")
    ap.add_argument("--cull", choices=("back", "front"), default=None, help="drop the back (or front) faces of an outward-wound mesh")
    ap.add_argument("--min_depth", type=float, default=0.0, help="a face with a vertex at or below this depth is not drawn")
    ap.add_argument("--suffix", default="gt", help="dense folder: the maps are written as <idx>_<suffix>.pfm")
    ap.add_argument("--write_index", action="store_true", help="also write each view's face indices as <name>_index.npy")
    ap.add_argument("--write_color", action="store_true", help="also write the interpolated vertex colours as <name>_color.png")
    ap.add_argument("--force", action="store_true", help="overwrite an existing depths/ folder of the session")
    return ap


def parse_args(argv=None):
    """-> the namespace with the options checked (SystemExit otherwise)."""
    a = build_parser().parse_args(argv)
    try:
        a.min_depth = check_options(a.min_depth, a.cull)[0]
        if not (a.mesh_scale > 0 and math.isfinite(a.mesh_scale)):
            raise ValueError("--mesh_scale must be positive and finite, got %r" % (a.mesh_scale,))
        if not a.suffix or a.suffix == "init" or any(ch in a.suffix for ch in "/\\") or a.suffix.startswith("."):
            raise ValueError("--suffix must be a plain name other than 'init', got %r" % (a.suffix,))
    except ValueError as e:
        raise SystemExit("mvsnet_amd.render_mesh: %s" % e)
    return a


def prepare_output(a):
    """The folder the maps go to; a session's existing depths/ is refused without --force, before any GPU work."""
    if a.session is not None:
        out = os.path.join(a.session, "depths")
        if os.path.exists(out) and not a.force:
            raise SystemExit("mvsnet_amd.render_mesh: %s exists; pass --force to overwrite it" % out)
        return out
    return os.path.join(a.dense_folder, "depths_mvsnet")


def output_stem(a, out_dir, i):
    """The path without extension of view i's files: depths/<i> or depths_mvsnet/<idx>_<suffix>."""
    return os.path.join(out_dir, "%d" % i if a.session is not None else "%d_%s" % (i, a.suffix))


def write_view(a, stem, depth, index=None, color=None):
    """One view's files: <stem>.png (session) or <stem>.pfm (dense folder), and on request <stem>_index.npy, <stem>_color.png."""
    if a.session is not None:
        write_depth_png(stem + ".png", depth)
    else:
        from .preprocess import write_pfm
        write_pfm(stem + ".pfm", depth)
    if index is not None:
        np.save(stem + "_index.npy", index)
    if color is not None:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(color)).save(stem + "_color.png")


def main(argv=None):
    a = parse_args(argv)
    out_dir = prepare_output(a)
    from ._lib import gpu_ready
    why = gpu_ready()
    if why is not None:
        raise SystemExit("mvsnet_amd.render_mesh needs a GPU and the HIP library: %s" % why)
    import torch
    from . import _lib
    from . import evaluate as E
    from .mesh import read_mesh_ply
    try:
        views = session_views(a.session) if a.session is not None else dense_folder_views(a.dense_folder)
        verts, rgb, faces = read_mesh_ply(a.mesh)
        if len(verts) == 0 or len(faces) == 0:
            raise ValueError("%s holds no faces" % a.mesh)
        dev = _lib.device(None, "point-cloud rendering")
        with torch.cuda.device(dev):
            t = E._points(verts, "mesh", dev)
            if a.mesh_scale != 1.0:
                t = (t.double() * a.mesh_scale).float().contiguous()
            if a.transform:
                from .register import read_transform
                t = E._transform(t, read_transform(a.transform))
            os.makedirs(out_dir, exist_ok=True)
            report = {"vertices": int(t.shape[0]), "faces": int(len(faces)), "views": len(views), "groups": [], "covered_pixels": 0}
            for (h, w), members in size_groups(views):
                cams = np.stack([views[k][1] for k in members])
                plan = RasterPlan(t, faces, cams, h, w, min_depth=a.min_depth, cull=a.cull)
                depth, index = (x.cpu().numpy() for x in plan.run())
                color = plan.colors(rgb).cpu().numpy() if a.write_color else None
                report["groups"].append({"height": h, "width": w, "views": [views[k][0] for k in members]})
                report["covered_pixels"] += int((index >= 0).sum())
                for j, k in enumerate(members):
                    write_view(a, output_stem(a, out_dir, views[k][0]), depth[j], index[j] if a.write_index else None,
                               color[j] if a.write_color else None)
    except (ValueError, OSError) as e:
        raise SystemExit("mvsnet_amd.render_mesh: %s" % e)
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
