"""Rendering of a point cloud into per-view depth maps on the MI355X: the way from a cloud back into the cameras.  A scanned
ground-truth cloud and a session's cameras give the depth maps that mvsnet_amd.test, mvsnet_amd.train and
Cluster.masked_reference_depth read; a fused cloud gives its own view from any camera and, per pixel, the point it shows.

    python -m mvsnet_amd.render --cloud G.ply [--cloud_scale S] [--transform T.txt] (--session DIR | --dense_folder DIR)
        [--splat S] [--occlusion k:rel:count] [--min_depth D] [--write_index] [--force]

One call is one fused HIP pass (csrc/render.hip, mvs_render_points_f32): every point is projected into every view and a
64-bit atomic minimum per covered pixel is the z-buffer; torch owns the device memory and the sort behind the processing
order.

Semantics (shared by the kernels, tests/render_reference.py and the tests).  Conventions are fusion.py's: cam (2,4,4) with
E = cam[0] world -> camera and K = cam[1][:3,:3]; pixel (x, y) is column x, row y at integer coordinates; views of one call
share one size H x W.  P_v = K_v [R_v | t_v] is composed in float64 (fusion.projection_matrix) and rounded to float32 once
(``projection_tables``).
  * Projection of point i = (X, Y, Z) (float32) into view v, all in float32, in this order, every product and sum rounded (no
    fused multiply-add): each row of P_v gives r = ((P0 X + P1 Y) + P2 Z) + P3, the three rows (u, v, w); then
    fx = floor(u / w + 0.5) and fy = floor(v / w + 0.5) with a correctly rounded division.
  * The point is a candidate in v when w is finite, w > min_depth (>= 0, default 0) and fx, fy are finite.  With splat radius
    s >= 0 (default 0) it covers the pixels (fx + dx, fy + dy), |dx|, |dy| <= s, that lie inside 0 <= x <= W - 1,
    0 <= y <= H - 1; the comparison is made in float32, so a huge coordinate is culled and never converted.
  * Z-buffer: per pixel the winner is the minimum of key = bits(w) << 32 | i over the candidates that cover it.  w is positive
    and finite, so its float32 bits order as unsigned integers: the smallest depth wins and exact ties go to the smallest
    input index, whatever the order of execution.  Raw outputs: depth (V,H,W) float32, 0 where empty, and index (V,H,W)
    int32, -1 where empty.
  * Hidden-point removal, off by default: occlusion = (k, rel, count), k >= 1, 0 < rel < 1, count >= 1.  A sparse front surface
    lets the surface behind it show through its gaps; the filter removes those pixels.  ratio = float32(1 - rel) (the
    difference in float64).  A pixel p of raw depth z > 0 is removed when at least `count` pixels q != p of its window
    |qx - px|, |qy - py| <= k inside the image are in front of it: raw[q] > 0 and raw[q] < z * ratio (a float32 product).  A
    removed pixel gets depth 0 and index -1.  The filter reads the raw map and writes another, so it too is order-free.
  * The processing order (order="voxel": points sorted by voxel key, cells of a few pixels' footprint, a stable sort) only
    decides which lane takes which point; it never changes a byte of the output.

Depth files: a session's depths/<i>.png holds uint16 millimetres floor(d + 0.5), 0 where the pixel is empty or the value
exceeds 65535 (``depth_to_png16``); a dense folder's depths_mvsnet/<idx>_gt.pfm holds the float32 map.
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import sys

import numpy as np

from .fusion import projection_matrix

MAX_SPLAT = 32                 # csrc/render.hip RD_MAX_SPLAT
MAX_OCCLUSION_RADIUS = 16      # RD_MAX_OCCL_RADIUS
ORDER_CELL_PIXELS = 4.0        # side of the processing order's voxels, in pixel footprints at the cloud's median depth


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def projection_tables(cams):
    """float32 (V*12,): P_v = K_v [R_v | t_v] row-major at [v 12], composed in float64 and rounded once."""
    cams = np.asarray(cams, np.float64)
    if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4):
        raise ValueError("cams must be (V,2,4,4), got %s" % (cams.shape,))
    return np.stack([projection_matrix(c) for c in cams]).reshape(-1).astype(np.float32)


def occlusion_ratio(rel):
    """float32(1 - rel), the difference in float64."""
    return float(np.float32(1.0 - float(rel)))


def check_options(splat=0, min_depth=0.0, occlusion=None):
    """-> (splat, min_depth, None or (k, rel, count)); ValueError outside the ranges of the module docstring."""
    if isinstance(splat, bool) or int(splat) != splat or not 0 <= int(splat) <= MAX_SPLAT:
        raise ValueError("splat must be an integer in 0..%d, got %r" % (MAX_SPLAT, splat))
    md = float(min_depth)
    if not (md >= 0.0 and math.isfinite(md) and math.isfinite(float(np.float32(md)))):
        raise ValueError("min_depth must be >= 0 and finite, got %r" % (min_depth,))
    if occlusion is not None:
        try:
            k, rel, count = occlusion
        except (TypeError, ValueError):
            raise ValueError("occlusion must be (k, rel, count), got %r" % (occlusion,))
        if int(k) != k or not 1 <= int(k) <= MAX_OCCLUSION_RADIUS:
            raise ValueError("occlusion radius k must be an integer in 1..%d, got %r" % (MAX_OCCLUSION_RADIUS, k))
        rel = float(rel)
        if not (0.0 < rel < 1.0 and 0.0 < occlusion_ratio(rel) < 1.0):
            raise ValueError("occlusion rel must lie in (0, 1), got %r" % (rel,))
        if int(count) != count or int(count) < 1:
            raise ValueError("occlusion count must be a positive integer, got %r" % (count,))
        occlusion = (int(k), rel, int(count))
    return int(splat), md, occlusion


def parse_occlusion(text):
    """"1:0.1:2" -> (1, 0.1, 2) (k:rel:count)."""
    tok = str(text).split(":")
    try:
        if len(tok) != 3:
            raise ValueError
        occ = (int(tok[0]), float(tok[1]), int(tok[2]))
    except ValueError:
        raise ValueError("occlusion %r: k:rel:count expected" % (text,))
    return check_options(occlusion=occ)[2]


def depth_to_png16(depth):
    """uint16 millimetres floor(d + 0.5); 0 where the pixel is empty (or not finite) or the value exceeds 65535."""
    d = np.asarray(depth, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.floor(d + 0.5)
        v = np.where(np.isfinite(v) & (v > 0) & (v <= 65535), v, 0.0)
    return v.astype(np.uint16)


def write_depth_png(path, depth):
    from .preprocess import write_png16
    write_png16(path, depth_to_png16(depth))


def _view_indices(pattern, suffix):
    out = []
    for p in glob.glob(pattern):
        stem = os.path.basename(p)[:-len(suffix)]
        if stem.isdigit():
            out.append(int(stem))
    return sorted(out)


def session_views(session):
    """A session's views in ascending index: [(index, cam (2,4,4) in millimetres as Cluster.load_camera gives it, (H, W) of
    images/<index>.jpg)]."""
    from PIL import Image
    from .mvs_data_generation import Cluster
    idx = _view_indices(os.path.join(session, "cameras", "*.json"), ".json")
    if not idx:
        raise FileNotFoundError("%s holds no cameras/<i>.json" % session)
    views = []
    for i in idx:
        c = Cluster(session, i, [], 0.0, 1.0, 1, depth_num=2)
        with Image.open(c.image_path(i)) as im:
            w, h = im.size
        views.append((i, c.load_camera(i), (h, w)))
    return views


def dense_folder_views(dense_folder):
    """A dense folder's views in ascending index: [(index, cam of depths_mvsnet/<idx>.txt, (H, W) of <idx>_init.pfm)]."""
    from .preprocess import load_cam, load_pfm
    folder = os.path.join(dense_folder, "depths_mvsnet")
    idx = _view_indices(os.path.join(folder, "*_init.pfm"), "_init.pfm")
    if not idx:
        raise FileNotFoundError("%s holds no <idx>_init.pfm" % folder)
    return [(i, load_cam(os.path.join(folder, "%d.txt" % i)), load_pfm(os.path.join(folder, "%d_init.pfm" % i)).shape[:2])
            for i in idx]


def size_groups(views):
    """Views of different sizes are rendered in groups of one size -> [((H, W), [positions in views])], by first appearance."""
    groups = {}
    for k, (_, _, size) in enumerate(views):
        groups.setdefault(tuple(int(s) for s in size), []).append(k)
    return list(groups.items())


# ------------------------------------------------------------------------------------------------ device side

class RenderPlan:
    """Points and projection tables on the device, outputs and workspace allocated once (the constructor synchronises when it
    computes the processing order).  ``enqueue()`` only launches on torch's current stream (no allocation, no
    synchronisation); ``run()`` enqueues and returns the (depth, index) device tensors, (V,H,W) float32 / int32;
    ``colors(rgb)`` gathers an image per view through ``index``."""

    def __init__(self, points, cams, height, width, *, splat=0, min_depth=0.0, occlusion=None, order="voxel", device=None):
        import torch
        from . import _lib
        self.splat, self.min_depth, self.occlusion = check_options(splat, min_depth, occlusion)
        if order is not None and not (isinstance(order, str) and order == "voxel"):
            raise ValueError('order must be "voxel" or None, got %r' % (order,))
        if int(height) != height or int(width) != width or int(height) < 1 or int(width) < 1:
            raise ValueError("height and width must be positive integers, got %r x %r" % (height, width))
        self.H, self.W = int(height), int(width)
        cams = np.asarray(cams.cpu().numpy() if hasattr(cams, "cpu") else cams, np.float64)
        if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4) or cams.shape[0] < 1:
            raise ValueError("cams must be (V,2,4,4), got %s" % (cams.shape,))
        self.V = int(cams.shape[0])
        if isinstance(points, torch.Tensor):
            if points.dtype != torch.float32:
                raise ValueError("points must be float32, got %s" % points.dtype)
            shape = tuple(points.shape)
        else:
            points = np.asarray(points)
            if points.dtype != np.float32:
                raise ValueError("points must be float32, got %s" % points.dtype)
            shape = points.shape
        if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
            raise ValueError("points must be (n,3) with n >= 1, got %s" % (tuple(shape),))
        if shape[0] > 2 ** 31 - 1:
            raise ValueError("%d points are beyond the kernel's int32 indices" % shape[0])
        self.dev = _lib.device(device, "point-cloud rendering")
        self.n = int(shape[0])
        lib = _lib.load()
        wsb = lib.mvs_render_workspace_bytes(self.V, self.H, self.W, 1 if self.occlusion else 0)
        if wsb == 0:
            raise ValueError("render: %d views of %d x %d are beyond the kernel's index range" % (self.V, self.H, self.W))
        self.proj_host = projection_tables(cams)
        with torch.cuda.device(self.dev):
            if isinstance(points, torch.Tensor):
                self.points = points.to(self.dev).contiguous()
            else:
                self.points = torch.as_tensor(np.ascontiguousarray(points)).to(self.dev)
            self.proj = torch.as_tensor(self.proj_host).to(self.dev)
            self.workspace = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
            self.depth = torch.empty((self.V, self.H, self.W), dtype=torch.float32, device=self.dev)
            self.index = torch.empty((self.V, self.H, self.W), dtype=torch.int32, device=self.dev)
            self.order = self._processing_order() if order == "voxel" else None

    def _processing_order(self):
        """Point indices sorted (stable) by voxel key.  The cell is ORDER_CELL_PIXELS pixel footprints w / f at the median
        depth w of a strided sample of the points over all views, so the 64 points of a wave fall on neighbouring pixels."""
        import torch
        from . import _lib
        t = self.points
        fin = torch.isfinite(t).all(1)
        good = t[fin]
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
            return None                                                        # one point, or a cloud without extent
        keys = torch.empty(self.n, dtype=torch.int64, device=self.dev)
        _lib.check(_lib.load().mvs_voxel_keys_f32(_lib.ptr(t), self.n, float(lo[0]), float(lo[1]), float(lo[2]), cell,
                                                  _lib.ptr(keys), _lib.stream_ptr()), "mvs_voxel_keys_f32")
        return torch.sort(keys, stable=True)[1].int().contiguous()

    def enqueue(self, *, order="plan", index=True):
        """Launches the render on the plan's device, on torch's current stream of that device.  order: "plan" (the plan's
        processing order), None (input order) or an int32 device tensor holding a permutation; index=False leaves
        ``self.index`` untouched (the kernel then writes depth alone)."""
        import torch
        from . import _lib
        order = self.order if isinstance(order, str) and order == "plan" else order
        if order is not None and (not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or order.numel() != self.n):
            raise ValueError("order must be an int32 tensor of %d entries" % self.n)
        k, rel, count = self.occlusion if self.occlusion else (0, 0.0, 0)
        with torch.cuda.device(self.dev):
            rc = _lib.load().mvs_render_points_f32(
                _lib.ptr(self.points), self.n, _lib.ptr(order), _lib.ptr(self.proj), self.V, self.H, self.W, self.splat,
                self.min_depth, k, occlusion_ratio(rel) if k else 0.0, count, _lib.ptr(self.depth),
                _lib.ptr(self.index) if index else None, _lib.ptr(self.workspace), self.workspace.numel(), _lib.stream_ptr())
        _lib.check(rc, "mvs_render_points_f32")

    def run(self, **kw):
        """enqueue() -> (depth (V,H,W) float32, index (V,H,W) int32): the plan's own device tensors, valid in stream order."""
        self.enqueue(**kw)
        return self.depth, self.index

    def colors(self, rgb):
        """(V,H,W,3) uint8 device tensor: rgb (n,3) uint8 gathered through ``index`` (of the last run) with torch; empty
        pixels are black."""
        import torch
        if isinstance(rgb, torch.Tensor):
            if rgb.dtype != torch.uint8:
                raise ValueError("rgb must be uint8, got %s" % rgb.dtype)
            c = rgb.to(self.dev)
        else:
            c = torch.as_tensor(np.ascontiguousarray(np.asarray(rgb, np.uint8))).to(self.dev)
        if tuple(c.shape) != (self.n, 3):
            raise ValueError("rgb must be (%d,3), got %s" % (self.n, tuple(c.shape)))
        idx = self.index.long()
        out = c[idx.clamp(min=0)]
        out[idx < 0] = 0
        return out


def render_depth_maps(points, cams, height, width, **options):
    """Renders (n,3) float32 points (numpy or device tensor) into the V cameras -> (depth (V,H,W) float32, index (V,H,W)
    int32) as numpy; options as RenderPlan's, semantics in the module docstring."""
    plan = RenderPlan(points, cams, height, width, **options)
    depth, index = plan.run()
    return depth.cpu().numpy(), index.cpu().numpy()


# ------------------------------------------------------------------------------------------------ command line

def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cloud", required=True, help="point cloud to render (PLY)")
    ap.add_argument("--cloud_scale", type=float, default=1.0, help="multiply the cloud's coordinates by this first (1000: metres -> mm)")
    ap.add_argument("--transform", default=None, help="4x4 transform file (as mvsnet_amd.register writes it), applied after the scale")
    tgt = ap.add_mutually_exclusive_group(required=True)
    tgt.add_argument("--session", default=None, help="session folder: cameras/<i>.json, images/<i>.jpg -> depths/<i>.png (uint16 mm)")
    tgt.add_argument("--dense_folder", default=None, help="dense folder: depths_mvsnet/<idx>.txt, <idx>_init.pfm -> <idx>_gt.pfm")
    ap.add_argument("--splat", type=int, default=0, help="splat radius in pixels")
    ap.add_argument("--occlusion", default=None, help="k:rel:count hidden-point removal (off without it)")
    ap.add_argument("--min_depth", type=float, default=0.0, help="points at or below this depth are not drawn")
    ap.add_argument("--write_index", action="store_true", help="also write each view's point indices as <name>_index.npy")
    ap.add_argument("--force", action="store_true", help="overwrite an existing depths/ folder of the session")
    return ap


def parse_args(argv=None):
    """-> the namespace with .occlusion parsed to (k, rel, count) or None and the options checked (SystemExit otherwise)."""
    ap = build_parser()
    a = ap.parse_args(argv)
    try:
        a.occlusion = parse_occlusion(a.occlusion) if a.occlusion is not None else None
        a.splat, a.min_depth, a.occlusion = check_options(a.splat, a.min_depth, a.occlusion)
        if not (a.cloud_scale > 0 and math.isfinite(a.cloud_scale)):
            raise ValueError("--cloud_scale must be positive and finite, got %r" % (a.cloud_scale,))
    except ValueError as e:
        raise SystemExit("mvsnet_amd.render: %s" % e)
    return a


def prepare_output(a):
    """The folder the maps go to; a session's existing depths/ is refused without --force, before any GPU work."""
    if a.session is not None:
        out = os.path.join(a.session, "depths")
        if os.path.exists(out) and not a.force:
            raise SystemExit("mvsnet_amd.render: %s exists; pass --force to overwrite it" % out)
        return out
    return os.path.join(a.dense_folder, "depths_mvsnet")


def main(argv=None):
    a = parse_args(argv)
    out_dir = prepare_output(a)
    from ._lib import gpu_ready
    why = gpu_ready()
    if why is not None:
        raise SystemExit("mvsnet_amd.render needs a GPU and the HIP library: %s" % why)
    import torch
    from . import _lib
    from . import evaluate as E
    from .preprocess import write_pfm
    try:
        views = session_views(a.session) if a.session is not None else dense_folder_views(a.dense_folder)
        pts, _ = E.read_ply_points(a.cloud)
        dev = _lib.device(None, "point-cloud rendering")
        with torch.cuda.device(dev):
            t = E._points(pts, "cloud", dev)
            if a.cloud_scale != 1.0:
                t = (t.double() * a.cloud_scale).float().contiguous()
            if a.transform:
                from .register import read_transform
                t = E._transform(t, read_transform(a.transform))
            os.makedirs(out_dir, exist_ok=True)
            report = {"points": int(t.shape[0]), "views": len(views), "groups": [], "covered_pixels": 0}
            for (h, w), members in size_groups(views):
                cams = np.stack([views[k][1] for k in members])
                depth, index = render_depth_maps(t, cams, h, w, splat=a.splat, min_depth=a.min_depth, occlusion=a.occlusion)
                report["groups"].append({"height": h, "width": w, "views": [views[k][0] for k in members]})
                report["covered_pixels"] += int((depth > 0).sum())
                for j, k in enumerate(members):
                    i = views[k][0]
                    if a.session is not None:
                        write_depth_png(os.path.join(out_dir, "%d.png" % i), depth[j])
                        stem = os.path.join(out_dir, "%d" % i)
                    else:
                        write_pfm(os.path.join(out_dir, "%d_gt.pfm" % i), depth[j])
                        stem = os.path.join(out_dir, "%d_gt" % i)
                    if a.write_index:
                        np.save(stem + "_index.npy", index[j])
    except (ValueError, OSError) as e:
        raise SystemExit("mvsnet_amd.render: %s" % e)
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
