"""Point-cloud evaluation on the MI355X: accuracy, completeness and F-score of a predicted cloud against a ground truth.

    python -m mvsnet_amd.evaluate --pred P.ply --gt G.ply --max_dist 20 [--thresholds 0.5,1,2]
        [--crop x0,y0,z0,x1,y1,z1] [--transform T.txt] [--voxel_pred s] [--voxel_gt s] [--out metrics.json]
        [--dump_distances DIR] [--align icp --align_stages 4:8:30,2:4:30,0:2:30 [--align_with_scale]]
        [--pred_spacing s] [--gt_spacing s]

The nearest-neighbour searches, the voxel downsampling and the statistics are HIP kernels (csrc/pointcloud.hip); torch owns
the device memory, the stable key sort of the downsampling and the transform / crop arithmetic.

Semantics (shared by the kernels, tests/pointcloud_reference.py and the tests).  P is the predicted cloud, G the ground
truth, each (n,3) float32.
  * Preprocessing, in this order, every step optional:
    1. transform: a 4x4 float64 matrix T applied to P only; its last row must be 0 0 0 1 (ValueError otherwise); per
       coordinate x'_i = T[i,0] x + T[i,1] y + T[i,2] z + T[i,3], evaluated left to right in float64 and rounded to float32 once;
    2. crop: an axis-aligned box lo <= x <= hi (inclusive, compared in float64), applied to both clouds;
    3. voxel downsampling, voxel_pred / voxel_gt per cloud (0 = off): key per axis floor((x - m) / s) in float64 with IEEE
       division, m the cloud's per-axis minimum after the crop; more than 2^21 voxels along an axis is a ValueError; the
       kept point of each occupied voxel is the FIRST point in input order (not a mean), and the output stays in input
       order (np.unique(keys, axis=0, return_index=True), sorted).
    A cloud that is empty after preprocessing is a ValueError that names it.
  * Alignment (align, optional; off by default and then nothing here changes).  Before the preprocessing, P is registered to
    G by ICP (mvsnet_amd/register.py, register_point_clouds with the options of `align`), starting from `transform` (identity
    without one) and restricted to `crop`; the refined transform then takes the place of `transform` in step 1, and the
    metrics gain "alignment": the transform, every stage's fitness / inlier_rmse / iterations and the reason the last stage
    stopped.
  * Nearest neighbour of a query cloud A in a target cloud B: d(a) = min_b |a - b| when that minimum is <= max_dist, else
    +inf ("beyond"); nn(a) is the minimiser's index in B, or -1 when beyond.  On the device d^2 is computed in float32 from
    float32 differences, and exact ties of that d^2 go to the smallest index.
  * Metrics.  Accuracy runs P -> G and completeness G -> P, as in DTU:
    accuracy = mean of d over the points of P with d < max_dist (points at or beyond max_dist are outliers and excluded),
    accuracy_inlier_fraction = their share of P, accuracy_median = the median of their d (np.median); completeness and its
    two companions the same over G; overall = (accuracy + completeness) / 2 (None when a mean has no inlier);
    for each tau of `thresholds` (0 < tau <= max_dist, ValueError otherwise): precision = #{p : d(p) < tau} / |P|,
    recall = #{g : d(g) < tau} / |G|, fscore = 2 precision recall / (precision + recall), 0 when both are 0.
  * Meshes (pred_faces / gt_faces with pred_spacing / gt_spacing, optional; off by default and then nothing here changes).
    That side is a triangle mesh: its cloud is the surface samples of mvsnet_amd.mesh_sample at density 1 / spacing^2 (seed
    0), taken before everything else, so the alignment, the transform, the crop and the voxel filter apply to the samples as
    they do to points.  The metrics gain "pred_sampling" / "gt_sampling": the spacing and the sampling's stats.
  * Sums are float64 and counts integers, reduced in a fixed order: the same inputs give bit-identical metrics and distance
    arrays on every run (no float atomics).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np

MAX_THRESHOLDS = 16                # csrc/pointcloud.hip PC_MAX_THRESHOLDS
MAX_CELLS = 1 << 24                # per-cell int32 starts: 64 MiB per array at most
VOXEL_AXIS_LIMIT = 1 << 21         # voxels per axis (21-bit key fields)
POINTS_PER_CELL = 16               # grid target: points in a target point's cell
MAX_DIST_CELLS = 16                # grid floor: cell >= max_dist / 16 bounds the rows a query far from the target visits


# ------------------------------------------------------------------------------------------------ PLY reading, no GPU needed

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_type(name, path):
    if name not in _PLY_TYPES:
        raise ValueError("%s: unknown PLY property type %r" % (path, name))
    return _PLY_TYPES[name]


def _parse_ply_header(data, path):
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    nl = data.find(b"\n", end)
    body = nl + 1 if nl >= 0 else len(data)
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("%s: property before any element" % path)
            if tok[1] == "list":
                elements[-1][2].append((tok[4], "list", _ply_type(tok[2], path), _ply_type(tok[3], path)))
            else:
                elements[-1][2].append((tok[2], _ply_type(tok[1], path)))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError("%s: unsupported PLY format %r" % (path, fmt))
    return fmt, elements, body


def read_ply_points(path):
    """Vertices of any PLY file -> (xyz (n,3) float32, rgb (n,3) uint8 or None).  ascii, binary_little_endian and
    binary_big_endian; any scalar vertex properties (x y z float or double; red green blue give the colours); elements other
    than `vertex` (faces, ...) are skipped.  A list property inside `vertex` or a missing x / y / z is a ValueError."""
    data = open(path, "rb").read()
    fmt, elements, pos = _parse_ply_header(data, path)
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError("%s: no vertex element" % path)
    _, n, props = elements[names.index("vertex")]
    if any(len(p) == 4 for p in props):
        raise ValueError("%s: list property %r inside the vertex element" % (path, [p[0] for p in props if len(p) == 4][0]))
    pnames = [p[0] for p in props]
    missing = [c for c in "xyz" if c not in pnames]
    if missing:
        raise ValueError("%s: vertex element without %s" % (path, "/".join(missing)))
    end = ">" if fmt == "binary_big_endian" else "<"
    if fmt == "ascii":
        lines = data[pos:].split(b"\n")
        row = 0
        for name, count, _ in elements:
            if name == "vertex":
                break
            row += count
        tok = b" ".join(lines[row:row + n]).split()
        if len(tok) != n * len(props):
            raise ValueError("%s: %d vertex values expected, found %d" % (path, n * len(props), len(tok)))
        vals = np.array(tok, np.float64).reshape(n, len(props))
        col = {p: vals[:, k] for k, p in enumerate(pnames)}
    else:
        for name, count, eprops in elements:
            if name == "vertex":
                break
            pos = _skip_binary_element(data, pos, count, eprops, end, path)
        dt = np.dtype([(p[0], end + p[1]) for p in props])
        if len(data) - pos < n * dt.itemsize:
            raise ValueError("%s: file ends inside the vertex element" % path)
        v = np.frombuffer(data, dt, count=n, offset=pos)
        col = {p: v[p] for p in pnames}
    xyz = np.stack([col["x"], col["y"], col["z"]], 1).astype(np.float32)
    rgb = None
    if all(c in col for c in ("red", "green", "blue")):
        rgb = np.stack([np.clip(col[c], 0, 255) for c in ("red", "green", "blue")], 1).astype(np.uint8)
    return xyz, rgb


def _skip_binary_element(data, pos, count, props, end, path):
    if all(len(p) == 2 for p in props):
        return pos + count * sum(np.dtype(p[1]).itemsize for p in props)
    for _ in range(count):
        for p in props:
            if len(p) == 2:
                pos += np.dtype(p[1]).itemsize
            else:
                ct, it = np.dtype(end + p[2]), np.dtype(p[3])
                if pos + ct.itemsize > len(data):
                    raise ValueError("%s: file ends inside a list property" % path)
                k = int(np.frombuffer(data, ct, count=1, offset=pos)[0])
                pos += ct.itemsize + k * it.itemsize
    return pos


# ------------------------------------------------------------------------------------------------ argument checks, no GPU

def check_transform(transform):
    """-> (4,4) float64; ValueError unless the shape is 4x4 and the last row is exactly 0 0 0 1."""
    T = np.asarray(transform, np.float64)
    if T.shape != (4, 4):
        raise ValueError("transform must be 4x4, got %s" % (T.shape,))
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) or not np.isfinite(T).all():
        raise ValueError("transform must be affine with last row 0 0 0 1, got %s" % T[3].tolist())
    return T


def check_crop(crop):
    c = np.asarray(crop, np.float64).reshape(-1)
    if c.shape != (6,) or not (c[:3] <= c[3:]).all():
        raise ValueError("crop must be x0,y0,z0,x1,y1,z1 with lo <= hi, got %s" % c.tolist())
    return c[:3], c[3:]


def check_thresholds(thresholds, max_dist):
    max_dist = float(max_dist)
    if not (max_dist > 0 and math.isfinite(max_dist)):
        raise ValueError("max_dist must be positive and finite, got %r" % max_dist)
    th = [float(t) for t in thresholds]
    if len(th) > MAX_THRESHOLDS:
        raise ValueError("at most %d thresholds, got %d" % (MAX_THRESHOLDS, len(th)))
    for t in th:
        if not (0 < t <= max_dist):
            raise ValueError("every threshold must satisfy 0 < tau <= max_dist = %g, got %g" % (max_dist, t))
    return max_dist, th


def metrics_from_counts(n_pred, n_gt, acc, comp, thresholds, acc_median=None, comp_median=None):
    """The metrics of the module docstring from acc / comp = (inlier sum, inlier count, [count below tau_t])."""
    def mean(s, c):
        return float(s) / int(c) if int(c) > 0 else None
    a, c = mean(acc[0], acc[1]), mean(comp[0], comp[1])
    prec = [int(k) / n_pred for k in acc[2]]
    rec = [int(k) / n_gt for k in comp[2]]
    f = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)]
    return {"accuracy": a, "accuracy_inlier_fraction": int(acc[1]) / n_pred, "accuracy_median": acc_median,
            "completeness": c, "completeness_inlier_fraction": int(comp[1]) / n_gt, "completeness_median": comp_median,
            "overall": (a + c) / 2 if a is not None and c is not None else None,
            "thresholds": list(thresholds), "precision": prec, "recall": rec, "fscore": f}


def inlier_median(d, max_dist):
    d = np.asarray(d)
    d = d[d < max_dist]
    return float(np.median(d.astype(np.float64))) if len(d) else None


# ------------------------------------------------------------------------------------------------ device side

def _points(x, name, dev):
    """numpy array or tensor (n,3) -> contiguous float32 tensor on dev; ValueError for other shapes or non-finite values."""
    import torch
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32:
            raise ValueError("%s must be float32, got %s" % (name, x.dtype))
        t = x.to(dev).contiguous()
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s must be (n,3), got %s" % (name, tuple(t.shape)))
    if t.shape[0] >= 2 ** 31 - 1:
        raise ValueError("%s: %d points are beyond the kernels' int32 indices" % (name, t.shape[0]))
    if t.shape[0] and not bool(torch.isfinite(t).all()):
        raise ValueError("%s holds non-finite coordinates" % name)
    return t


def _transform(t, T):
    """x'_i = T[i,0] x + T[i,1] y + T[i,2] z + T[i,3], left to right in float64, rounded to float32 once."""
    import torch
    p = t.double()
    cols = [((p[:, 0] * T[i, 0] + p[:, 1] * T[i, 1]) + p[:, 2] * T[i, 2]) + T[i, 3] for i in range(3)]
    return torch.stack(cols, 1).float().contiguous()


def _crop(t, lo, hi):
    p = t.double()
    keep = ((p >= p.new_tensor(lo)) & (p <= p.new_tensor(hi))).all(1)
    return t[keep].contiguous()


def _voxel(t, s, name):
    """First point in input order of each occupied voxel of side s (HIP keys, torch stable sort, HIP marks + compaction)."""
    import torch
    from . import _lib
    n = t.shape[0]
    if n == 0:
        return t
    m = t.min(0).values.double().cpu().numpy()
    top = t.max(0).values.double().cpu().numpy()
    nvox = np.floor((top - m) / s) + 1
    if (nvox > VOXEL_AXIS_LIMIT).any():
        raise ValueError("%s: voxel size %g gives %d voxels along an axis, more than 2^21" % (name, s, int(nvox.max())))
    lib = _lib.load()
    keys = torch.empty(n, dtype=torch.int64, device=t.device)
    _lib.check(lib.mvs_voxel_keys_f32(_lib.ptr(t), n, float(m[0]), float(m[1]), float(m[2]), float(s), _lib.ptr(keys),
                                      _lib.stream_ptr()), "mvs_voxel_keys_f32")
    sk, order = torch.sort(keys, stable=True)
    out = torch.empty_like(t)
    count = torch.zeros(1, dtype=torch.int32, device=t.device)
    ws = torch.empty(lib.mvs_voxel_select_workspace_bytes(n), dtype=torch.uint8, device=t.device)
    _lib.check(lib.mvs_voxel_select_f32(_lib.ptr(t), n, _lib.ptr(sk), _lib.ptr(order.contiguous()), _lib.ptr(out),
                                        _lib.ptr(count), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "mvs_voxel_select_f32")
    return out[:int(count.item())].contiguous()


def preprocess(pred, gt, *, transform=None, crop=None, voxel_pred=0.0, voxel_gt=0.0, device=None):
    """§ Preprocessing of the module docstring on the device -> (pred, gt) float32 (n,3) tensors, ValueError when empty."""
    import torch
    from . import _lib
    T = check_transform(transform) if transform is not None else None
    box = check_crop(crop) if crop is not None else None
    for name, v in (("voxel_pred", voxel_pred), ("voxel_gt", voxel_gt)):
        if not (float(v) >= 0 and math.isfinite(float(v))):
            raise ValueError("%s must be >= 0, got %r" % (name, v))
    dev = _lib.device(device, "point-cloud evaluation")
    with torch.cuda.device(dev):
        p, g = _points(pred, "pred", dev), _points(gt, "gt", dev)
        if T is not None:
            p = _transform(p, T)
        if box is not None:
            p, g = _crop(p, *box), _crop(g, *box)
        if voxel_pred:
            p = _voxel(p, float(voxel_pred), "pred")
        if voxel_gt:
            g = _voxel(g, float(voxel_gt), "gt")
    for name, t in (("pred", p), ("gt", g)):
        if t.shape[0] == 0:
            raise ValueError("the %s cloud is empty after preprocessing" % name)
    return p, g


def choose_grid(target, max_dist, cell=None):
    """Uniform grid over the target (device tensor (n,3)) -> {"origin", "cell", "dims"}.  Origin = the target's minimum.  The
    cell is sized from occupancy measured on the device so that a target point's cell holds about POINTS_PER_CELL points on
    average over the points (two refinements assuming points on surfaces), at least max_dist / MAX_DIST_CELLS, and grown until
    the grid has at most 2^24 cells.  `cell` overrides the size (still grown to the cap).  Any grid gives the same answers;
    the grid only sets the speed."""
    import torch
    lo = target.min(0).values
    hi = target.max(0).values
    lo_h, hi_h = lo.double().cpu().numpy(), hi.double().cpu().numpy()
    ext = np.maximum(hi_h - lo_h, 0.0)
    emax = float(ext.max())
    n = target.shape[0]
    if cell is None:
        if emax == 0.0:
            cell = float(max_dist)
        else:
            vol = float(np.prod(np.maximum(ext, emax * 1e-3)))
            s = (vol * POINTS_PER_CELL / n) ** (1.0 / 3.0)
            for _ in range(2):
                s = max(s, emax / (VOXEL_AXIS_LIMIT / 2))
                k = torch.floor((target - lo) / s).long()
                counts = torch.unique(k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42), return_counts=True)[1].double()
                seen = float((counts * counts).sum()) / n      # points of a point's own cell: sparse outliers weigh little
                s *= min(max(math.sqrt(POINTS_PER_CELL / seen), 0.125), 8.0)
            cell = max(s, float(max_dist) / MAX_DIST_CELLS)
    cell = float(cell)
    if not (cell > 0 and math.isfinite(cell)):
        raise ValueError("cell must be positive and finite, got %r" % cell)
    while True:
        dims = (np.floor(ext / cell) + 1).astype(np.int64)
        if int(np.prod(dims)) <= MAX_CELLS:
            break
        cell *= 1.01 * (float(np.prod(dims)) / MAX_CELLS) ** (1.0 / 3.0)
    return {"origin": [float(v) for v in lo.cpu().numpy()], "cell": float(np.float32(cell)), "dims": [int(d) for d in dims]}


def _surface(points, faces, spacing, name, device):
    """A side of the evaluation that is a mesh -> (its surface samples as a device tensor, {"spacing", stats...}); a side
    without faces and spacing -> (points, None), untouched."""
    if faces is None and spacing is None:
        return points, None
    if faces is None or spacing is None:
        raise ValueError("%s_faces and %s_spacing go together" % (name, name))
    import torch
    from . import _lib, mesh_sample
    from .mesh_common import inputs
    density = mesh_sample.check_spacing(spacing)
    if not hasattr(points, "shape") or not hasattr(faces, "shape"):
        raise ValueError("%s and %s_faces must be arrays or tensors" % (name, name))
    what = "point-cloud evaluation"
    mesh_sample._shapes(points, None, faces)
    dev, v, _, f = inputs(points, None, faces, _lib.device(device, what), what, mesh_sample._shapes)   # None: the current device
    with torch.cuda.device(dev):
        out, stats = mesh_sample.sample_device(v, None, f, dev, density)
    return out["xyz"], dict(stats, spacing=float(spacing))


class NearestPlan:
    """Capped nearest neighbours of every query point in the target (device float32 (n,3) tensors or numpy arrays).  The
    constructor uploads, picks the grid and allocates (it may synchronise); ``enqueue()`` only launches, on torch's current
    stream (capturable); ``result()`` synchronises once -> (dist (nq,) float32, inf beyond; index (nq,) int32, -1 beyond)."""

    def __init__(self, query, target, max_dist, *, cell=None, device=None):
        import torch
        from . import _lib
        self.dev = _lib.device(device, "point-cloud evaluation")
        self.max_dist = float(max_dist)
        if not (self.max_dist > 0 and math.isfinite(self.max_dist)):
            raise ValueError("max_dist must be positive and finite, got %r" % max_dist)
        with torch.cuda.device(self.dev):
            self.query, self.target = _points(query, "query", self.dev), _points(target, "target", self.dev)
            if self.query.shape[0] == 0 or self.target.shape[0] == 0:
                raise ValueError("nearest neighbours need non-empty clouds")
            self.grid = choose_grid(self.target, self.max_dist, cell)
            nq, nt = self.query.shape[0], self.target.shape[0]
            wsb = _lib.load().mvs_nn_workspace_bytes(nq, nt, *self.grid["dims"])
            if wsb == 0:
                raise ValueError("nearest neighbours: grid %s not supported" % (self.grid["dims"],))
            self.workspace = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
            self.dist = torch.empty(nq, dtype=torch.float32, device=self.dev)
            self.index = torch.empty(nq, dtype=torch.int32, device=self.dev)

    def enqueue(self):
        import torch
        with torch.cuda.device(self.dev):
            self._enqueue()

    def _enqueue(self):
        from . import _lib
        g = self.grid
        rc = _lib.load().mvs_nn_f32(_lib.ptr(self.query), self.query.shape[0], _lib.ptr(self.target), self.target.shape[0],
                                    *g["origin"], g["cell"], *g["dims"], self.max_dist, _lib.ptr(self.dist),
                                    _lib.ptr(self.index), _lib.ptr(self.workspace), self.workspace.numel(), _lib.stream_ptr())
        _lib.check(rc, "mvs_nn_f32")

    def result(self):
        import torch
        with torch.cuda.device(self.dev):
            d = torch.empty(self.dist.shape, dtype=self.dist.dtype, pin_memory=True)
            i = torch.empty(self.index.shape, dtype=self.index.dtype, pin_memory=True)
            d.copy_(self.dist, non_blocking=True)
            i.copy_(self.index, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return d.numpy(), i.numpy()


class EvaluationPlan:
    """Both directions plus the statistics.  The constructor uploads, preprocesses (output sizes are known only after it),
    picks both grids and allocates; ``enqueue()`` launches both grid builds, both queries and both statistics on torch's
    current stream (capturable); ``result()`` synchronises once and returns the metrics dict of evaluate_point_clouds."""

    def __init__(self, pred, gt, *, max_dist, thresholds=(), transform=None, crop=None, voxel_pred=0.0, voxel_gt=0.0,
                 align=None, device=None, pred_faces=None, pred_spacing=None, gt_faces=None, gt_spacing=None):
        import torch
        from . import _lib
        self.max_dist, self.thresholds = check_thresholds(thresholds, max_dist)
        pred, self.pred_sampling = _surface(pred, pred_faces, pred_spacing, "pred", device)
        gt, self.gt_sampling = _surface(gt, gt_faces, gt_spacing, "gt", device)
        self.pred_points, self.gt_points = len(pred), len(gt)
        self.alignment = None
        if align is not None:
            from . import register
            if transform is not None:
                check_transform(transform)
            reg = register.register_point_clouds(pred, gt, init=transform, crop=crop, device=device, **dict(align))
            transform = reg["transform"]
            self.alignment = {"transform": reg["transform"], "stopped": reg["stopped"],
                              "stages": [{k: st[k] for k in ("voxel", "max_corr_dist", "fitness", "inlier_rmse", "iterations",
                                                             "stopped")} for st in reg["stages"]]}
        p, g = preprocess(pred, gt, transform=transform, crop=crop, voxel_pred=voxel_pred, voxel_gt=voxel_gt, device=device)
        self.dev = p.device
        self.acc = NearestPlan(p, g, self.max_dist, device=self.dev)
        self.comp = NearestPlan(g, p, self.max_dist, device=self.dev)
        lib = _lib.load()
        nt = len(self.thresholds)
        self._thr = (ctypes.c_float * nt)(*self.thresholds) if nt else None
        with torch.cuda.device(self.dev):
            self.stats = torch.zeros((2, 2 + nt), dtype=torch.float64, device=self.dev)
            self.stats_ws = [torch.empty(lib.mvs_dist_stats_workspace_bytes(pl.query.shape[0], nt), dtype=torch.uint8,
                                         device=self.dev) for pl in (self.acc, self.comp)]
        self.distances = None

    @property
    def pred(self):
        return self.acc.query

    @property
    def gt(self):
        return self.comp.query

    def enqueue(self):
        import torch
        from . import _lib
        with torch.cuda.device(self.dev):
            lib = _lib.load()
            for k, (pl, ws) in enumerate(zip((self.acc, self.comp), self.stats_ws)):
                pl._enqueue()
                rc = lib.mvs_dist_stats_f32(_lib.ptr(pl.dist), pl.dist.numel(), self.max_dist, self._thr, len(self.thresholds),
                                            _lib.ptr(self.stats[k]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
                _lib.check(rc, "mvs_dist_stats_f32")

    def result(self):
        import torch
        with torch.cuda.device(self.dev):
            host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (self.stats, self.acc.dist, self.comp.dist)]
            for h, t in zip(host, (self.stats, self.acc.dist, self.comp.dist)):
                h.copy_(t, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        st, dp, dg = (h.numpy() for h in host)
        self.distances = (dp, dg)
        nt = len(self.thresholds)
        acc = (st[0, 0], int(st[0, 1]), [int(v) for v in st[0, 2:2 + nt]])
        comp = (st[1, 0], int(st[1, 1]), [int(v) for v in st[1, 2:2 + nt]])
        out = metrics_from_counts(len(dp), len(dg), acc, comp, self.thresholds, inlier_median(dp, self.max_dist),
                                  inlier_median(dg, self.max_dist))
        out.update({"max_dist": self.max_dist, "pred_points": self.pred_points, "gt_points": self.gt_points,
                    "pred_points_used": len(dp), "gt_points_used": len(dg),
                    "grid_pred_to_gt": self.acc.grid, "grid_gt_to_pred": self.comp.grid})
        if self.alignment is not None:
            out["alignment"] = self.alignment
        for name, sampling in (("pred_sampling", self.pred_sampling), ("gt_sampling", self.gt_sampling)):
            if sampling is not None:
                out[name] = sampling
        return out


def evaluate_point_clouds(pred, gt, *, max_dist, thresholds=(), transform=None, crop=None, voxel_pred=0.0, voxel_gt=0.0,
                          align=None, device=None, pred_faces=None, pred_spacing=None, gt_faces=None, gt_spacing=None):
    """Accuracy / completeness / precision / recall / F-score of pred against gt (numpy arrays or device tensors (n,3)) on
    the GPU; semantics in the module docstring.  Returns the metrics dict (plus the point counts before and after the
    preprocessing and the two grids that were used).  align: None, or a dict of register_point_clouds options (at least
    "stages") to refine `transform` by ICP first.  pred_faces / gt_faces (F,3) int32 with pred_spacing / gt_spacing: that side
    is a mesh with pred / gt its vertices, and its surface samples are evaluated."""
    plan = EvaluationPlan(pred, gt, max_dist=max_dist, thresholds=thresholds, transform=transform, crop=crop,
                          voxel_pred=voxel_pred, voxel_gt=voxel_gt, align=align, device=device, pred_faces=pred_faces,
                          pred_spacing=pred_spacing, gt_faces=gt_faces, gt_spacing=gt_spacing)
    plan.enqueue()
    return plan.result()


# ------------------------------------------------------------------------------------------------ command line

def _floats(text, n=None, what="values"):
    vals = [float(v) for v in text.split(",") if v.strip()]
    if n is not None and len(vals) != n:
        raise SystemExit("%s: %d comma-separated numbers expected, got %r" % (what, n, text))
    return vals


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", required=True, help="predicted cloud (PLY)")
    ap.add_argument("--gt", required=True, help="ground-truth cloud (PLY)")
    ap.add_argument("--max_dist", type=float, required=True, help="distance cap; points at or beyond it are outliers")
    ap.add_argument("--thresholds", default="", help="comma-separated tau for precision / recall / F-score")
    ap.add_argument("--crop", default=None, help="x0,y0,z0,x1,y1,z1 (inclusive box, both clouds)")
    ap.add_argument("--transform", default=None, help="text file with a 4x4 matrix applied to the prediction")
    ap.add_argument("--voxel_pred", type=float, default=0.0)
    ap.add_argument("--voxel_gt", type=float, default=0.0)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--dump_distances", default=None, help="directory for pred_to_gt.npy and gt_to_pred.npy")
    ap.add_argument("--align", default=None, choices=["icp"], help="refine --transform (or identity) by ICP before evaluating")
    ap.add_argument("--align_stages", default=None, help="voxel:max_corr_dist:max_iterations[,...] (mvsnet_amd.register)")
    ap.add_argument("--align_with_scale", action="store_true", help="let the alignment solve for a uniform scale as well")
    from .mesh_sample import add_options, check_spacing, read_ply_mesh
    add_options(ap, "pred_")
    add_options(ap, "gt_")
    a = ap.parse_args(argv)
    try:
        for s in (a.pred_spacing, a.gt_spacing):
            if s is not None:
                check_spacing(s)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.evaluate: --pred_spacing / --gt_spacing: %s" % e)
    align = None
    if a.align:
        from . import register
        if not a.align_stages:
            raise SystemExit("mvsnet_amd.evaluate: --align icp needs --align_stages")
        try:
            align = {"stages": register.parse_stages(a.align_stages), "with_scale": a.align_with_scale}
        except ValueError as e:
            raise SystemExit("mvsnet_amd.evaluate: %s" % e)
    elif a.align_stages or a.align_with_scale:
        raise SystemExit("mvsnet_amd.evaluate: --align_stages / --align_with_scale need --align icp")
    from ._lib import gpu_ready
    why = gpu_ready()
    if why is not None:
        raise SystemExit("mvsnet_amd.evaluate needs a GPU and the HIP library: %s" % why)
    thresholds = _floats(a.thresholds, what="--thresholds")
    crop = _floats(a.crop, 6, "--crop") if a.crop else None
    transform = np.loadtxt(a.transform, dtype=np.float64).reshape(4, 4) if a.transform else None
    try:
        pred_faces = gt_faces = None
        if a.pred_spacing is None:
            pred, _ = read_ply_points(a.pred)
        else:
            pred, _, pred_faces = read_ply_mesh(a.pred)
        if a.gt_spacing is None:
            gt, _ = read_ply_points(a.gt)
        else:
            gt, _, gt_faces = read_ply_mesh(a.gt)
    except ValueError as e:
        if a.pred_spacing is None and a.gt_spacing is None:
            raise
        raise SystemExit("mvsnet_amd.evaluate: %s" % e)
    try:
        plan = EvaluationPlan(pred, gt, max_dist=a.max_dist, thresholds=thresholds, transform=transform, crop=crop,
                              voxel_pred=a.voxel_pred, voxel_gt=a.voxel_gt, align=align, pred_faces=pred_faces,
                              pred_spacing=a.pred_spacing, gt_faces=gt_faces, gt_spacing=a.gt_spacing)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.evaluate: %s" % e)
    plan.enqueue()
    metrics = plan.result()
    line = json.dumps(metrics)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.dump_distances:
        os.makedirs(a.dump_distances, exist_ok=True)
        np.save(os.path.join(a.dump_distances, "pred_to_gt.npy"), plan.distances[0])
        np.save(os.path.join(a.dump_distances, "gt_to_pred.npy"), plan.distances[1])
    return metrics


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
