"""View selection on the MI355X: from cameras and a point cloud to the neighbour list and depth range of every reference
view, the covisibility.json (or pair.txt) that inference, test, train, depthfusion and render start from.  The cloud can be a
scan, a sparse structure-from-motion cloud or a cloud fused here.

    python -m mvsnet_amd.select_views --cloud C.ply [--cloud_scale S] [--transform T.txt] (--session DIR | --dense_folder DIR)
        [--visibility frustum|zbuffer --z_rel 0.01 --splat S --occlusion k:rel:count] [--min_depth D] [--num_views 10]
        [--min_shared 1] [--theta0 5 --sigma1 1 --sigma2 10] [--depth_percentiles 1:99] [--format covisibility|pair] [--force]

Three HIP passes over the cloud (csrc/view_selection.hip): the visibility of every point in every view as a bit mask, the
pair matrix of shared points and scores with the matrix in LDS, and two histogram passes for the exact depth percentiles;
torch owns the device memory, the scans of the histograms and the sort behind the processing order.

Semantics (shared by the kernels, tests/view_selection_reference.py and the tests).  Conventions are render.py's: cam (2,4,4),
P_v = K_v [R_v | t_v] composed in float64 and rounded to float32 once (``render.projection_tables``), points (n,3) float32,
the views of one visibility call share one size H x W.  The camera centre is c_v = -R_v^T t_v in float64, rounded to float32
once (``camera_centres``).
  1. Visibility of point i in view v.  (u, v, w) and the pixel (fx, fy) exactly as render.py defines them: float32, every
     product and sum rounded, no fused multiply-add, a correctly rounded division, floor(. + 0.5).  The point is a candidate
     when w is finite, w > min_depth, fx and fy are finite and 0 <= fx <= W - 1, 0 <= fy <= H - 1, compared in float32.
     Mode "frustum": visible = candidate.  Mode "zbuffer": with a depth map Z (V,H,W) float32 the point is visible when it is
     a candidate, Z[v,fy,fx] > 0 and w <= Z[v,fy,fx] * tol, tol = float32(1 + z_rel) (the sum in float64, the product in
     float32).  Z is a ``render.RenderPlan``'s map of the same points and cameras with the user's splat / occlusion options; a
     pixel the hidden-point filter removed hides every point that lands on it.  Result: mask (n, MW) 64-bit words,
     MW = ceil(V / 64), view position p is bit p % 64 of word p / 64, and visible (V) int64 counts.  Views of different sizes
     are processed per ``render.size_groups`` group; each call sets only its own views' bits of a mask zeroed before.
  2. Pair score.  For a < b and every point visible in both (shared[a][b] += 1), all in float32, rounded at every step:
     A = c_a - p, B = c_b - p; dot = (Ax Bx + Ay By) + Az Bz, na and nb the same shape of sum; r = (dot dot) / (na nb) with a
     correctly rounded division (cos^2); x = 1 - r, and x = 0 when x < 0; s = sqrt(x), correctly rounded (sin);
     k = min(8191, floor(s 8192)).  The pair contributes T[k] when dot > 0 and k is finite, else 0 (an angle of 90 degrees or
     more, a point at a camera centre).  T[k] = floor(65535 g(theta_k) + 0.5) as uint16 (``weight_table``),
     theta_k = degrees(asin((k + 1/2) / 8192)), g(theta) = exp(-(theta - theta0)^2 / (2 sigma^2)) with sigma = sigma1 for
     theta <= theta0 and sigma2 otherwise, in float64 on the host; defaults theta0 = 5, sigma1 = 1, sigma2 = 10 (upstream
     MVSNet's).  score_sum[a][b] = sum of T[k] is an exact integer (int64); the score is score_sum / 65535 in float64.  Both
     matrices are mirrored to b < a, diagonals are 0.  The table's bins are part of the definition: no transcendental runs in
     the kernel and the sum is an integer, so the result is independent of the order of execution.  A bin is at most 0.014
     degrees wide up to 60 degrees and |g'| <= 0.607 / sigma1 per degree, so a pair is within 0.015 of the continuous formula.
  3. Depth range of view v.  Over the m visible points' w (the float32 of the projection above), ascending:
     min_depth = w[m lo // 100], max_depth = w[min(m - 1, m hi // 100)], lo and hi integers (default 1:99), in integer
     arithmetic; m = 0 gives 0, 0.  Exact: positive float32 bits order as unsigned integers, so two histogram passes (the
     high 16 bits, then the low 16 bits inside the bin that holds the rank) select the value.
  4. Selection (``select_neighbours``).  For reference view r the candidates are the views b != r with score_sum[r][b] > 0
     and shared[r][b] >= min_shared (default 1), ordered by score_sum descending, ties to the smaller view position; the first
     num_views (default 10) are kept.

Files: covisibility.json is {"<index>": {"views", "min_depth", "max_depth", "scores", "shared"}} keyed by image index (the
depths are the float32 values as Python floats; ClusterGenerator.load_clusters ignores the two extra keys); pair.txt is the
view count, then per view its index and "k id score id score ..." with scores as %.4f, which PairClusterGenerator reads.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

from . import render as Rn

MAX_VIEWS = 512                # csrc/view_selection.hip VS_MAX_VIEWS
TABLE_SIZE = 8192
SCORE_UNIT = 65535


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def weight_table(theta0=5.0, sigma1=1.0, sigma2=10.0):
    """(8192,) uint16: T[k] of the module docstring."""
    theta0, sigma1, sigma2 = float(theta0), float(sigma1), float(sigma2)
    if not (0.0 < theta0 < 90.0 and sigma1 > 0.0 and sigma2 > 0.0 and math.isfinite(sigma1) and math.isfinite(sigma2)):
        raise ValueError("theta0 must lie in (0, 90) and the sigmas be positive, got %r, %r, %r" % (theta0, sigma1, sigma2))
    k = np.arange(TABLE_SIZE, dtype=np.float64)
    theta = np.degrees(np.arcsin((k + 0.5) / TABLE_SIZE))
    sigma = np.where(theta <= theta0, sigma1, sigma2)
    g = np.exp(-np.square(theta - theta0) / (2.0 * np.square(sigma)))
    return np.floor(SCORE_UNIT * g + 0.5).astype(np.uint16)


def camera_centres(cams):
    """(V,3) float32: c_v = -R_v^T t_v in float64, rounded once."""
    cams = np.asarray(cams, np.float64)
    if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4):
        raise ValueError("cams must be (V,2,4,4), got %s" % (cams.shape,))
    return np.stack([-(c[0, :3, :3].T @ c[0, :3, 3]) for c in cams]).astype(np.float32)


def z_tolerance(z_rel):
    """float32(1 + z_rel), the sum in float64."""
    return float(np.float32(1.0 + float(z_rel)))


def parse_percentiles(text):
    """"1:99" -> (1, 99): integers with 0 <= lo <= hi <= 100."""
    try:
        lo, hi = (int(t) for t in (text.split(":") if isinstance(text, str) else text))
    except (TypeError, ValueError):
        raise ValueError("depth percentiles %r: lo:hi expected" % (text,))
    if not 0 <= lo <= hi <= 100:
        raise ValueError("depth percentiles must satisfy 0 <= lo <= hi <= 100, got %d:%d" % (lo, hi))
    return lo, hi


def select_neighbours(score_sum, shared, num_views=10, min_shared=1):
    """Per view position r the positions of its neighbours, best first (the module docstring's step 4) -> list of lists."""
    score_sum, shared = np.asarray(score_sum, np.int64), np.asarray(shared, np.int64)
    V = score_sum.shape[0]
    if score_sum.shape != (V, V) or shared.shape != (V, V):
        raise ValueError("score_sum and shared must be (V,V), got %s and %s" % (score_sum.shape, shared.shape))
    if int(num_views) < 0 or int(min_shared) < 0:
        raise ValueError("num_views and min_shared must not be negative")
    out = []
    for r in range(V):
        cand = [b for b in range(V) if b != r and score_sum[r, b] > 0 and shared[r, b] >= int(min_shared)]
        cand.sort(key=lambda b: (-int(score_sum[r, b]), b))
        out.append(cand[:int(num_views)])
    return out


def covisibility(indices, neighbours, score_sum, shared, min_depth, max_depth):
    """The dictionary covisibility.json holds; `indices` are the image indices of the view positions."""
    score_sum, shared = np.asarray(score_sum, np.int64), np.asarray(shared, np.int64)
    lo, hi = np.asarray(min_depth, np.float32), np.asarray(max_depth, np.float32)
    out = {}
    for r, views in enumerate(neighbours):
        out[str(int(indices[r]))] = {"views": [int(indices[b]) for b in views], "min_depth": float(lo[r]), "max_depth": float(hi[r]),
                                     "scores": [int(score_sum[r, b]) / float(SCORE_UNIT) for b in views],
                                     "shared": [int(shared[r, b]) for b in views]}
    return out


def write_covisibility(path, indices, neighbours, score_sum, shared, min_depth, max_depth):
    with open(path, "w") as f:
        json.dump(covisibility(indices, neighbours, score_sum, shared, min_depth, max_depth), f)


def pair_text(indices, neighbours, score_sum):
    score_sum = np.asarray(score_sum, np.int64)
    lines = ["%d" % len(neighbours)]
    for r, views in enumerate(neighbours):
        lines.append("%d" % int(indices[r]))
        lines.append(" ".join(["%d" % len(views)] + ["%d %.4f" % (int(indices[b]), int(score_sum[r, b]) / float(SCORE_UNIT))
                                                     for b in views]))
    return "\n".join(lines) + "\n"


def write_pair_txt(path, indices, neighbours, score_sum):
    with open(path, "w") as f:
        f.write(pair_text(indices, neighbours, score_sum))


# ------------------------------------------------------------------------------------------------ device side

class ViewSelectionPlan:
    """Points, projection tables, camera centres and the weight table on the device, outputs and workspaces allocated once
    (the constructor synchronises when it computes the processing order).  `views` is [(index, cam, (H, W))] as
    ``render.session_views`` gives it, or pass cams (V,2,4,4) and size=(H, W).  ``run()`` enqueues everything on torch's
    current stream, synchronises once and returns a dict of device tensors: mask (n, MW) int64 (the 64-bit words),
    visible (V) int64, shared and score_sum (V,V) int64 (mirrored), min_depth and max_depth (V) float32."""

    def __init__(self, points, views=None, *, cams=None, size=None, visibility="frustum", z_rel=0.01, splat=0, occlusion=None,
                 min_depth=0.0, theta0=5.0, sigma1=1.0, sigma2=10.0, percentiles=(1, 99), order="voxel", device=None):
        import torch
        from . import _lib
        if (views is None) == (cams is None):
            raise ValueError("pass either views or cams and size")
        if views is None:
            if size is None:
                raise ValueError("cams need size=(H, W)")
            views = [(k, c, size) for k, c in enumerate(np.asarray(cams, np.float64))]
        self.views = [(int(i), np.asarray(c, np.float64), (int(s[0]), int(s[1]))) for i, c, s in views]
        self.V = len(self.views)
        if not 1 <= self.V <= MAX_VIEWS:
            raise ValueError("1 to %d views are supported, got %d" % (MAX_VIEWS, self.V))
        if visibility not in ("frustum", "zbuffer"):
            raise ValueError('visibility must be "frustum" or "zbuffer", got %r' % (visibility,))
        self.visibility = visibility
        self.splat, self.min_depth, self.occlusion = Rn.check_options(splat, min_depth, occlusion)
        z_rel = float(z_rel)
        if not (z_rel >= 0.0 and math.isfinite(z_rel)):
            raise ValueError("z_rel must be >= 0 and finite, got %r" % (z_rel,))
        self.z_tol = z_tolerance(z_rel)
        self.lo, self.hi = parse_percentiles(percentiles)
        if order is not None and not (isinstance(order, str) and order == "voxel"):
            raise ValueError('order must be "voxel" or None, got %r' % (order,))
        cams_all = np.stack([c for _, c, _ in self.views])
        if cams_all.shape[1:] != (2, 4, 4):
            raise ValueError("every cam must be (2,4,4), got %s" % (cams_all.shape[1:],))
        self.groups = Rn.size_groups(self.views)
        self.MW = (self.V + 63) // 64
        # a 1 x 1 render plan checks and uploads the points and computes the processing order, which depends on the cameras'
        # focal lengths and not on the image size; the z-buffer's plans, one per size group, share both
        base = Rn.RenderPlan(points, cams_all, 1, 1, min_depth=self.min_depth, order=order, device=device)
        self.dev, self.points, self.n, self.order = base.dev, base.points, base.n, base.order
        self.render_plans = []
        for (h, w), members in self.groups:
            if visibility == "zbuffer":
                rp = Rn.RenderPlan(self.points, cams_all[members], h, w, splat=self.splat, min_depth=self.min_depth,
                                   occlusion=self.occlusion, order=None, device=self.dev)
                rp.order = self.order
                self.render_plans.append(rp)
            elif self.V * h * w > 2 ** 31 - 1 or max(h, w) > 2 ** 24:
                raise ValueError("select_views: %d views of %d x %d are beyond the kernel's index range" % (self.V, h, w))
        lib = _lib.load()
        wsb = lib.mvs_view_scores_workspace_bytes(self.n, self.V)
        with torch.cuda.device(self.dev):
            dev = self.dev
            self.proj = torch.as_tensor(Rn.projection_tables(cams_all)).to(dev)
            self.centres = torch.as_tensor(camera_centres(cams_all).reshape(-1)).to(dev)
            self.table = torch.as_tensor(weight_table(theta0, sigma1, sigma2).view(np.int16)).to(dev)
            self.group_bits = [torch.as_tensor(np.asarray(m, np.int32)).to(dev) for _, m in self.groups]
            self.group_proj = [torch.as_tensor(Rn.projection_tables(cams_all[m])).to(dev) for _, m in self.groups]
            self.mask = torch.empty((self.n, self.MW), dtype=torch.int64, device=dev)
            self.score_sum = torch.empty((self.V, self.V), dtype=torch.int64, device=dev)
            self.shared = torch.empty((self.V, self.V), dtype=torch.int64, device=dev)
            self.workspace = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=dev)
            self.hist = torch.empty((self.V, 2, 65536), dtype=torch.int32, device=dev)
            self.prefixes = torch.empty((self.V, 2), dtype=torch.int32, device=dev)

    def enqueue_visibility(self):
        from . import _lib
        lib = _lib.load()
        self.mask.zero_()
        for g, ((h, w), members) in enumerate(self.groups):
            zbuf = self.render_plans[g].run(index=False)[0] if self.visibility == "zbuffer" else None
            _lib.check(lib.mvs_view_visibility_f32(_lib.ptr(self.points), self.n, _lib.ptr(self.group_proj[g]),
                                                   _lib.ptr(self.group_bits[g]), len(members), h, w, self.min_depth, _lib.ptr(zbuf),
                                                   self.z_tol, _lib.ptr(self.mask), self.MW, _lib.stream_ptr()),
                       "mvs_view_visibility_f32")

    def enqueue_scores(self, *, order="plan"):
        """order: "plan" (the plan's processing order), None (input order) or an int32 device permutation."""
        import torch
        from . import _lib
        order = self.order if isinstance(order, str) and order == "plan" else order
        if order is not None and (not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or order.numel() != self.n):
            raise ValueError("order must be an int32 tensor of %d entries" % self.n)
        _lib.check(_lib.load().mvs_view_scores_f32(_lib.ptr(self.points), self.n, _lib.ptr(order), _lib.ptr(self.mask), self.MW,
                                                   _lib.ptr(self.centres), self.V, _lib.ptr(self.table), _lib.ptr(self.score_sum),
                                                   _lib.ptr(self.shared), _lib.ptr(self.workspace), self.workspace.numel(),
                                                   _lib.stream_ptr()), "mvs_view_scores_f32")

    def _hist(self, which):
        from . import _lib
        _lib.check(_lib.load().mvs_view_depth_hist_f32(_lib.ptr(self.points), self.n, _lib.ptr(self.proj), self.V, _lib.ptr(self.mask),
                                                       self.MW, which, _lib.ptr(self.prefixes) if which else None,
                                                       _lib.ptr(self.hist), _lib.stream_ptr()), "mvs_view_depth_hist_f32")

    def enqueue_depth_ranges(self):
        """-> (visible (V) int64, min_depth (V) float32, max_depth (V) float32), device tensors in stream order."""
        import torch
        self._hist(0)
        cum = self.hist.view(-1)[:self.V * 65536].view(self.V, 65536).long().cumsum(1)
        m = cum[:, -1].clone()
        ranks = torch.stack([(m * self.lo) // 100, torch.minimum((m - 1).clamp(min=0), (m * self.hi) // 100)], 1)     # (V,2)
        high = torch.searchsorted(cum, ranks, right=True).clamp(max=65535)
        before = torch.where(high > 0, cum.gather(1, (high - 1).clamp(min=0)), torch.zeros_like(high))
        self.prefixes.copy_(high.int())
        self._hist(1)
        cum2 = self.hist.long().cumsum(2)                                                                             # (V,2,65536)
        low = torch.searchsorted(cum2, (ranks - before).unsqueeze(2), right=True).squeeze(2).clamp(max=65535)
        bits = torch.where(m.unsqueeze(1) > 0, (high << 16) | low, torch.zeros_like(high)).int()
        depth = bits.view(torch.float32)
        return m, depth[:, 0].contiguous(), depth[:, 1].contiguous()

    def run(self, *, order="plan"):
        import torch
        with torch.cuda.device(self.dev):
            self.enqueue_visibility()
            self.enqueue_scores(order=order)
            visible, lo, hi = self.enqueue_depth_ranges()
            score_sum, shared = self.score_sum + self.score_sum.t(), self.shared + self.shared.t()
            torch.cuda.current_stream().synchronize()
        return {"mask": self.mask, "visible": visible, "shared": shared, "score_sum": score_sum, "min_depth": lo, "max_depth": hi}


# ------------------------------------------------------------------------------------------------ command line

def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cloud", required=True, help="point cloud the views are selected from (PLY)")
    ap.add_argument("--cloud_scale", type=float, default=1.0, help="multiply the cloud's coordinates by this first (1000: metres -> mm)")
    ap.add_argument("--transform", default=None, help="4x4 transform file (as mvsnet_amd.register writes it), applied after the scale")
    tgt = ap.add_mutually_exclusive_group(required=True)
    tgt.add_argument("--session", default=None, help="session folder: cameras/<i>.json, images/<i>.jpg -> covisibility.json")
    tgt.add_argument("--dense_folder", default=None, help="dense folder: depths_mvsnet/<idx>.txt, <idx>_init.pfm -> pair.txt")
    ap.add_argument("--visibility", choices=("frustum", "zbuffer"), default="frustum")
    ap.add_argument("--z_rel", type=float, default=0.01, help="zbuffer: a point is visible up to (1 + z_rel) times the rendered depth")
    ap.add_argument("--splat", type=int, default=0, help="zbuffer: splat radius of the rendered depth maps")
    ap.add_argument("--occlusion", default=None, help="zbuffer: k:rel:count hidden-point removal of the rendered depth maps")
    ap.add_argument("--min_depth", type=float, default=0.0, help="points at or below this depth are not visible")
    ap.add_argument("--num_views", type=int, default=10, help="neighbours kept per reference view")
    ap.add_argument("--min_shared", type=int, default=1, help="a neighbour shares at least this many points")
    ap.add_argument("--theta0", type=float, default=5.0)
    ap.add_argument("--sigma1", type=float, default=1.0)
    ap.add_argument("--sigma2", type=float, default=10.0)
    ap.add_argument("--depth_percentiles", default="1:99", help="lo:hi percentiles of the visible points' depths")
    ap.add_argument("--format", choices=("covisibility", "pair"), default=None,
                    help="covisibility.json (default for a session) or pair.txt (default for a dense folder)")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    try:
        a.occlusion = Rn.parse_occlusion(a.occlusion) if a.occlusion is not None else None
        a.splat, a.min_depth, a.occlusion = Rn.check_options(a.splat, a.min_depth, a.occlusion)
        a.depth_percentiles = parse_percentiles(a.depth_percentiles)
        weight_table(a.theta0, a.sigma1, a.sigma2)
        if not (a.cloud_scale > 0 and math.isfinite(a.cloud_scale)):
            raise ValueError("--cloud_scale must be positive and finite, got %r" % (a.cloud_scale,))
        if not (a.z_rel >= 0 and math.isfinite(a.z_rel)):
            raise ValueError("--z_rel must be >= 0 and finite, got %r" % (a.z_rel,))
        if a.num_views < 0 or a.min_shared < 0:
            raise ValueError("--num_views and --min_shared must not be negative")
    except ValueError as e:
        raise SystemExit("mvsnet_amd.select_views: %s" % e)
    if a.format is None:
        a.format = "covisibility" if a.session is not None else "pair"
    return a


def prepare_output(a):
    """The file the result goes to; an existing one is refused without --force, before any GPU work."""
    out = os.path.join(a.session if a.session is not None else a.dense_folder,
                       "covisibility.json" if a.format == "covisibility" else "pair.txt")
    if os.path.exists(out) and not a.force:
        raise SystemExit("mvsnet_amd.select_views: %s exists; pass --force to overwrite it" % out)
    return out


def main(argv=None):
    a = parse_args(argv)
    out = prepare_output(a)
    from ._lib import gpu_ready
    why = gpu_ready()
    if why is not None:
        raise SystemExit("mvsnet_amd.select_views needs a GPU and the HIP library: %s" % why)
    import torch
    from . import _lib
    from . import evaluate as E
    try:
        views = Rn.session_views(a.session) if a.session is not None else Rn.dense_folder_views(a.dense_folder)
        pts, _ = E.read_ply_points(a.cloud)
        dev = _lib.device(None, "point-cloud rendering")
        with torch.cuda.device(dev):
            t = E._points(pts, "cloud", dev)
            if a.cloud_scale != 1.0:
                t = (t.double() * a.cloud_scale).float().contiguous()
            if a.transform:
                from .register import read_transform
                t = E._transform(t, read_transform(a.transform))
            plan = ViewSelectionPlan(t, views, visibility=a.visibility, z_rel=a.z_rel, splat=a.splat, occlusion=a.occlusion,
                                     min_depth=a.min_depth, theta0=a.theta0, sigma1=a.sigma1, sigma2=a.sigma2,
                                     percentiles=a.depth_percentiles)
            r = {k: v.cpu().numpy() for k, v in plan.run().items() if k != "mask"}
        indices = [v[0] for v in views]
        neighbours = select_neighbours(r["score_sum"], r["shared"], a.num_views, a.min_shared)
        if a.format == "covisibility":
            write_covisibility(out, indices, neighbours, r["score_sum"], r["shared"], r["min_depth"], r["max_depth"])
        else:
            write_pair_txt(out, indices, neighbours, r["score_sum"])
    except (ValueError, OSError) as e:
        raise SystemExit("mvsnet_amd.select_views: %s" % e)
    print(json.dumps({"points": int(t.shape[0]), "views": len(views), "output": out, "visible": [int(x) for x in r["visible"]],
                      "neighbours": [len(x) for x in neighbours]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
