"""Geometric-consistency fusion of a session's depth maps into one coloured point cloud, on the MI355X.

The reference ends its pipeline by running the external CUDA program fusibile (mvsnet/depthfusion.py:194-214) on the
Gipuma hand-off.  This module is the project's own fusion, a HIP kernel (csrc/fusion.hip, mvs_fusion_f32) behind
``fuse_depth_maps``.  It is NOT bit-compatible with fusibile: fusibile's disparity test depends on camera constants this
project cannot check, so the criteria below are stated in pixels and relative depth instead.  Normals are this project's own:
the reference writes a constant fake normal and switches fusibile's normal test off; here they are estimated from the depth
maps on the device (``estimate_normals``), carried through the fusion and, optionally, used to reject pairs.

Semantics (shared by the kernel, tests/fusion_reference.py and the tests).  Views share one depth size H x W; pixel (x, y)
is column x, row y at integer coordinates.  cam (2,4,4) is the project's layout: E = cam[0] = [R | t] world -> camera,
K = cam[1][:3,:3].
  * valid pixel: depth > 0, finite, prob >= prob_threshold (the rule of depthfusion.probability_filter);
  * X_v(p, d) = R_v^T (d K_v^-1 [x, y, 1]^T - t_v);  projection (u, v, w) = K_s (R_s X + t_s), pixel (u/w, v/w), depth w;
  * for a valid pixel p of reference view r at depth d, X = X_r(p, d), and each source s of r's list in ascending order:
    w > 0; q = (floor(u/w + 1/2), floor(v/w + 1/2)) inside the image and valid in s; X_s = X_s(q, D_s[q]) projected into r
    gives (u', v', w'); s is consistent when w' > 0, |(u'/w', v'/w') - (x, y)| < reproj_threshold and
    |w' - d| / d < depth_rel_threshold;
  * p is kept when n, the number of consistent sources, satisfies n >= num_consistent (a float, as the reference's flag);
    its point is (X + sum of the consistent X_s) / (n + 1), its colour the reference image at the nearest pixel
    (floor((x + 1/2) W_img / W), floor((y + 1/2) H_img / H)), black without images;
  * source lists: every other view by default, or one list per reference view;
  * dedupe (default): reference views in ascending order; for each kept pixel the witness q of every consistent source is
    marked used, and a used pixel is never a reference pixel later (it still serves as a witness);
  * output: by view ascending, then row-major pixel order; bitwise reproducible (no float atomics).

Per-view normal map (``estimate_normals``, mvs_depth_normals_f32; shared by the kernel, tests/normals_reference.py and the
tests).  df is the filtered depth of view v: D where the pixel is valid, else 0.
  * pixel (x, y) with d = df[y, x] > 0 has a(x, y) = (x d, y d, d);  A_v = R_v^T K_v^-1 (the first three columns of B_v; the
    translation cancels in differences);
  * a horizontal neighbour q in {(x-1, y), (x+1, y)} is usable when it is inside the image, df[q] > 0 and
    |d_q - d| < jump_threshold d (default 0.05).  Both usable: tx = a(x+1, y) - a(x-1, y); one usable: the one-sided
    difference oriented towards +x (a(x+1, y) - a(x, y) or a(x, y) - a(x-1, y)); none usable: the pixel has no normal;
  * the vertical tangent ty by the same rule with (x, y-1), (x, y+1), oriented towards +y;
  * n = A_v ty x A_v tx; a zero or non-finite length means no normal, otherwise n is normalised, and negated when
    n . (X - C_v) > 0 (X the pixel's world point, C_v the camera centre; X - C_v = A_v a), so that it faces the camera;
  * "no normal" is stored as (0, 0, 0); normals are in the world frame (frame="camera": R_v n).

Fusion with normals (``FusionPlan(normals=True)``, mvs_fusion_normals_f32): the geometry is exactly as above.  Additionally
  * normal_angle_threshold (degrees, off by default).  When set, a pixel without a normal is not a valid pixel -- neither a
    reference pixel nor a witness -- and a geometrically consistent pair is consistent only if
    n_r . n_s(q) > cos(normal_angle_threshold).  When off, points, order and colours are bit-identical to the fusion above;
  * a kept pixel's fused normal is N = n_r + sum of n_s(q) over its consistent sources (missing normals contribute zero),
    the partial sums added in the same fixed slice order as the positions (bitwise reproducible); N is normalised, or stored
    as (0, 0, 0) when |N| = 0;
  * dedupe behaves as above.

The device evaluates the two projections of a pair with 3x4 tables composed on the host in float64 (``camera_tables``) and
rounded to float32 once, so decisions can differ from the float64 statement only where a quantity lies within float32 error
of its threshold or of a rounding boundary.
"""
from __future__ import annotations

import glob
import os

import numpy as np

PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
# with normals: fusibile's vertex, x y z nx ny nz red green blue (27 bytes)
PLY_HEADER_NORMALS = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                      "property float nx\nproperty float ny\nproperty float nz\n"
                      "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
_PLY_DTYPE_NORMALS = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                               ("red", "u1"), ("green", "u1"), ("blue", "u1")])


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def backprojection_matrix(cam):
    """B (3,4) float64 with X = B (x d, y d, d, 1): [R^T K^-1 | -R^T t]."""
    cam = np.asarray(cam, np.float64)
    R, t, K = cam[0][:3, :3], cam[0][:3, 3], cam[1][:3, :3]
    return np.concatenate([R.T @ np.linalg.inv(K), (-R.T @ t)[:, None]], axis=1)


def projection_matrix(cam):
    """P (3,4) float64 = K [R | t]."""
    cam = np.asarray(cam, np.float64)
    return cam[1][:3, :3] @ cam[0][:3, :4]


def camera_tables(cams):
    """float32 (V*V*12 + V*12,): M[a][b] = P_b o B_a row-major at [(a V + b) 12], then B_v, composed in float64."""
    cams = np.asarray(cams, np.float64)
    V = cams.shape[0]
    B = np.stack([backprojection_matrix(c) for c in cams])                         # (V,3,4)
    P = np.stack([projection_matrix(c) for c in cams])                             # (V,3,4)
    B4 = np.concatenate([B, np.tile(np.array([0, 0, 0, 1.0]), (V, 1, 1))], axis=1)  # (V,4,4)
    M = np.einsum("bij,ajk->abik", P, B4)                                          # (a, b, 3, 4)
    return np.concatenate([M.reshape(-1), B.reshape(-1)]).astype(np.float32)


def source_lists(V, sources=None):
    """Per reference view the ascending list of distinct source views, itself excluded (every other view by default)."""
    if sources is None:
        return [[s for s in range(V) if s != r] for r in range(V)]
    if len(sources) != V:
        raise ValueError("sources: one list per view expected (%d), got %d" % (V, len(sources)))
    out = []
    for r, lst in enumerate(sources):
        lst = sorted(set(int(s) for s in lst))
        if any(s < 0 or s >= V for s in lst):
            raise ValueError("sources of view %d name a view outside 0..%d" % (r, V - 1))
        out.append([s for s in lst if s != r])
    return out


def _stack_views(maps, name, dtype):
    arrs = [np.asarray(m) for m in maps]
    if not arrs:
        raise ValueError("%s: no views" % name)
    shapes = {a.shape for a in arrs}
    if len(shapes) != 1:
        raise ValueError("%s: every view must share one size, got %s" % (name, sorted(shapes)))
    return np.ascontiguousarray(np.stack(arrs).astype(dtype, copy=False))


def write_ply(path, xyz, rgb, normals=None):
    """Binary little-endian PLY: x y z float, red green blue uchar (15 bytes per point); with normals x y z nx ny nz float,
    red green blue uchar (27 bytes per point, fusibile's vertex layout)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    if len(xyz) != len(rgb):
        raise ValueError("xyz and rgb differ in length")
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(-1, 3)
        if len(normals) != len(xyz):
            raise ValueError("xyz and normals differ in length")
    v = np.empty(len(xyz), _PLY_DTYPE if normals is None else _PLY_DTYPE_NORMALS)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normals is not None:
        v["nx"], v["ny"], v["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with open(path, "wb") as f:
        f.write(((PLY_HEADER if normals is None else PLY_HEADER_NORMALS) % len(v)).encode("ascii"))
        f.write(v.tobytes())


def read_ply(path):
    """Reads what write_ply writes -> (xyz (P,3) float32, rgb (P,3) uint8)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int(data[:end].decode("ascii").split("element vertex ")[1].split("\n")[0])
    if data[:end].decode("ascii") != PLY_HEADER % n:
        raise ValueError("%s: not a PLY written by write_ply" % path)
    v = np.frombuffer(data[end:], _PLY_DTYPE, count=n)
    return (np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32),
            np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.uint8))


def read_ply_normals(path):
    """Reads what write_ply writes with normals -> (xyz (P,3) float32, rgb (P,3) uint8, normals (P,3) float32)."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int(data[:end].decode("ascii").split("element vertex ")[1].split("\n")[0])
    if data[:end].decode("ascii") != PLY_HEADER_NORMALS % n:
        raise ValueError("%s: not a PLY written by write_ply with normals" % path)
    v = np.frombuffer(data[end:], _PLY_DTYPE_NORMALS, count=n)
    return (np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32),
            np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.uint8),
            np.stack([v["nx"], v["ny"], v["nz"]], 1).astype(np.float32))


def normal_cos_threshold(normal_angle_threshold):
    """The cosine handed to the kernel for an angle in degrees: None -> -1 (off); ValueError outside (0, 180].  180 degrees
    (every pair of normals passes, pixels without a normal still drop out) is the float32 just above -1, since -1 means off."""
    if normal_angle_threshold is None:
        return -1.0
    a = float(normal_angle_threshold)
    if not (0.0 < a <= 180.0):
        raise ValueError("normal_angle_threshold must lie in (0, 180] degrees, got %r" % (normal_angle_threshold,))
    return float(max(np.float32(np.cos(np.radians(a))), np.nextafter(np.float32(-1), np.float32(0))))


def check_jump_threshold(jump_threshold):
    j = float(jump_threshold)
    if not j >= 0.0:
        raise ValueError("jump_threshold must be >= 0, got %r" % (jump_threshold,))
    return j


def load_dense_folder(dense_folder):
    """depths_mvsnet/<idx>_init.pfm, <idx>_prob.pfm, <idx>.txt and <idx>.jpg (predictlib.write_output_slice's names), views
    in ascending <idx> -> (indices, depths (V,H,W) float32, probs (V,H,W) float32, cams (V,2,4,4) float64, images (V,Hi,Wi,3)
    uint8 RGB or None when no view has a .jpg)."""
    from PIL import Image
    from .preprocess import load_cam, load_pfm
    folder = os.path.join(dense_folder, "depths_mvsnet")
    idx = sorted(int(os.path.basename(p)[:-len("_init.pfm")]) for p in glob.glob(os.path.join(folder, "*_init.pfm"))
                 if os.path.basename(p)[:-len("_init.pfm")].isdigit())
    if not idx:
        raise FileNotFoundError("%s holds no <idx>_init.pfm" % folder)
    f = lambda i, suffix: os.path.join(folder, "%d%s" % (i, suffix))
    depths = _stack_views([load_pfm(f(i, "_init.pfm")) for i in idx], "depth maps", np.float32)
    probs = _stack_views([load_pfm(f(i, "_prob.pfm")) for i in idx], "probability maps", np.float32)
    cams = np.stack([load_cam(f(i, ".txt")) for i in idx])
    have = [os.path.isfile(f(i, ".jpg")) for i in idx]
    images = None
    if all(have):
        images = _stack_views([np.asarray(Image.open(f(i, ".jpg")).convert("RGB")) for i in idx], "images", np.uint8)
    elif any(have):
        raise FileNotFoundError("%s: some views have a .jpg and some do not" % folder)
    return idx, depths, probs, cams, images


def listed_sources(dense_folder, indices):
    """Each view's neighbours from <dense_folder>/covisibility.json (session format) or pair.txt (upstream format), as
    positions in `indices`; neighbours without a depth map are dropped.  When both files exist, covisibility.json is used,
    as mvs_data_generation.make_generator does, so fusion takes the neighbours the depth maps were inferred with."""
    import json
    pos = {int(i): k for k, i in enumerate(indices)}
    pair = os.path.join(dense_folder, "pair.txt")
    covis = os.path.join(dense_folder, "covisibility.json")
    listed = {}
    if os.path.isfile(covis):
        with open(covis) as f:
            data = json.load(f)
        listed = {int(k): [int(v) for v in d["views"]] for k, d in data.items()}
    elif os.path.isfile(pair):
        from .mvs_data_generation import gen_pipeline_mvs_list
        for ref, paths in gen_pipeline_mvs_list(dense_folder, 1 << 30):
            listed[int(ref)] = [int(os.path.splitext(os.path.basename(p))[0]) for p in paths[2::2]]
    else:
        raise FileNotFoundError("%s holds neither covisibility.json nor pair.txt" % dense_folder)
    return [[pos[s] for s in listed.get(int(i), []) if s in pos] for i in indices]


# ------------------------------------------------------------------------------------------------ device side

class FusionPlan:
    """Inputs on the device, output and workspace buffers allocated once.  ``enqueue()`` only launches (no allocation, no
    synchronisation: it captures into a graph); ``result()`` synchronises once and returns the points."""

    def __init__(self, depths, probs, cams, images=None, *, prob_threshold=0.8, reproj_threshold=1.0,
                 depth_rel_threshold=0.01, num_consistent=3, sources=None, dedupe=True, device=None, normals=False,
                 normal_angle_threshold=None, jump_threshold=0.05):
        import torch
        from . import _lib
        # normals=True: the plan also estimates normal maps and fuses them; a normal_angle_threshold implies it
        self.cos_threshold = normal_cos_threshold(normal_angle_threshold)          # ValueError before any GPU work
        self.jump_threshold = check_jump_threshold(jump_threshold)
        self.normals = bool(normals) or normal_angle_threshold is not None
        # host arrays are stacked first: views of different sizes are a ValueError with or without a GPU
        depths, probs = self._host(depths, "depth maps", np.float32), self._host(probs, "probability maps", np.float32)
        images = None if images is None else self._host(images, "images", np.uint8)
        if not torch.cuda.is_available():
            raise _lib.MvsnetHipError("depth-map fusion runs on the GPU (HIP); no GPU is visible to this process")
        dev = torch.device(device) if device is not None else torch.device("cuda")
        if dev.type != "cuda":
            raise ValueError("fusion runs on a GPU device, got %s" % dev)
        self.dev = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
        d = self._views(depths, "depth maps", torch.float32)
        p = self._views(probs, "probability maps", torch.float32)
        if d.dim() != 3 or p.shape != d.shape:
            raise ValueError("depths and probs must be (V,H,W) of one size, got %s and %s" % (tuple(d.shape), tuple(p.shape)))
        V, H, W = d.shape
        cams = np.asarray(cams.cpu().numpy() if hasattr(cams, "cpu") else cams, np.float64)
        if cams.shape != (V, 2, 4, 4):
            raise ValueError("cams must be (%d,2,4,4), got %s" % (V, cams.shape))
        self.V, self.H, self.W = V, H, W
        self.depth, self.prob = d, p
        self.images = None
        if images is not None:
            im = self._views(images, "images", torch.uint8)
            if im.dim() != 4 or im.shape[0] != V or im.shape[3] != 3:
                raise ValueError("images must be (%d,H,W,3) uint8, got %s" % (V, tuple(im.shape)))
            self.images = im
        lists = source_lists(V, sources)
        self.max_sources = max(len(l) for l in lists)
        offs = np.zeros(V + 1, np.int32)
        offs[1:] = np.cumsum([len(l) for l in lists])
        idx = np.array([s for l in lists for s in l] or [0], np.int32)
        self.src_offsets = torch.as_tensor(offs).to(self.dev)
        self.src_index = torch.as_tensor(idx).to(self.dev)
        self.tables = torch.as_tensor(camera_tables(cams)).to(self.dev)
        self.params = (float(prob_threshold), float(reproj_threshold), float(depth_rel_threshold), float(num_consistent),
                       1 if dedupe else 0)
        lib = _lib.load()
        wsb = (lib.mvs_fusion_normals_workspace_bytes if self.normals else lib.mvs_fusion_workspace_bytes)(
            V, H, W, self.max_sources, self.params[4])
        if wsb == 0:
            raise ValueError("fusion: %d views of %d x %d are beyond the kernel's index range" % (V, H, W))
        n = V * H * W
        self.workspace = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
        self.xyz = torch.empty((n, 3), dtype=torch.float32, device=self.dev)
        self.rgb = torch.empty((n, 3), dtype=torch.uint8, device=self.dev)
        self.nrm = torch.empty((n, 3), dtype=torch.float32, device=self.dev) if self.normals else None
        self.view_index = torch.empty(n, dtype=torch.int32, device=self.dev)
        self.pixel_index = torch.empty(n, dtype=torch.int32, device=self.dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.dev)

    @staticmethod
    def _host(x, name, dtype):
        import torch
        if isinstance(x, torch.Tensor):
            return x
        if isinstance(x, (list, tuple)) and x and all(isinstance(t, torch.Tensor) for t in x):
            if len({tuple(t.shape) for t in x}) != 1:
                raise ValueError("%s: every view must share one size" % name)
            return torch.stack(list(x))
        return _stack_views(x, name, dtype)

    def _views(self, x, name, dtype):
        import torch
        if isinstance(x, torch.Tensor):
            if x.dtype != dtype:
                raise ValueError("%s must be %s, got %s" % (name, dtype, x.dtype))
            return x.to(self.dev).contiguous()
        return torch.as_tensor(x).to(self.dev)

    def enqueue(self):
        """Launches the fusion on the plan's device, on torch's current stream of that device (capturable)."""
        import torch
        with torch.cuda.device(self.dev):
            self._enqueue()

    def _enqueue(self):
        from . import _lib
        lib = _lib.load()
        pt, rt, dt, nc, dd = self.params
        im = self.images
        if self.normals:
            rc = lib.mvs_fusion_normals_f32(
                _lib.ptr(self.depth), _lib.ptr(self.prob), self.V, self.H, self.W, _lib.ptr(self.tables),
                _lib.ptr(self.src_offsets), _lib.ptr(self.src_index), self.max_sources, pt, rt, dt, nc, dd, self.jump_threshold,
                self.cos_threshold, _lib.ptr(im), im.shape[1] if im is not None else 0, im.shape[2] if im is not None else 0,
                _lib.ptr(self.xyz), _lib.ptr(self.rgb), _lib.ptr(self.nrm), _lib.ptr(self.view_index),
                _lib.ptr(self.pixel_index), _lib.ptr(self.count), _lib.ptr(self.workspace), self.workspace.numel(),
                _lib.stream_ptr())
            _lib.check(rc, "mvs_fusion_normals_f32")
            return
        rc = lib.mvs_fusion_f32(_lib.ptr(self.depth), _lib.ptr(self.prob), self.V, self.H, self.W, _lib.ptr(self.tables),
                                _lib.ptr(self.src_offsets), _lib.ptr(self.src_index), self.max_sources, pt, rt, dt, nc, dd,
                                _lib.ptr(im), im.shape[1] if im is not None else 0, im.shape[2] if im is not None else 0,
                                _lib.ptr(self.xyz), _lib.ptr(self.rgb), _lib.ptr(self.view_index),
                                _lib.ptr(self.pixel_index), _lib.ptr(self.count),
                                _lib.ptr(self.workspace), self.workspace.numel(), _lib.stream_ptr())
        _lib.check(rc, "mvs_fusion_f32")

    def result(self, with_pixels=False, with_normals=False):
        """(xyz (P,3) float32, rgb (P,3) uint8, view_index (P,) int32[, pixel_index (P,) int32 = y W + x][, normals (P,3)
        float32, last]) as numpy; one synchronisation.  with_normals needs a plan made with normals."""
        if with_normals and not self.normals:
            raise ValueError("this plan was made without normals (FusionPlan(..., normals=True))")
        n = int(self.count.item())
        out = (self.xyz[:n].cpu().numpy(), self.rgb[:n].cpu().numpy(), self.view_index[:n].cpu().numpy())
        if with_pixels:
            out += (self.pixel_index[:n].cpu().numpy(),)
        if with_normals:
            out += (self.nrm[:n].cpu().numpy(),)
        return out


def fuse_depth_maps(depths, probs, cams, images=None, *, prob_threshold=0.8, reproj_threshold=1.0, depth_rel_threshold=0.01,
                    num_consistent=3, sources=None, dedupe=True, device=None, normals=False, normal_angle_threshold=None,
                    jump_threshold=0.05):
    """Fuses V depth maps (numpy arrays or device tensors, (V,H,W) or a list of (H,W)) into one point cloud on the GPU.
    Returns (xyz (P,3) float32, rgb (P,3) uint8, view_index (P,) int32), and with normals=True (implied by a
    normal_angle_threshold) a fourth array, normals (P,3) float32; semantics in the module docstring.
    ValueError when the views differ in size or normal_angle_threshold lies outside (0, 180]."""
    plan = FusionPlan(depths, probs, cams, images, prob_threshold=prob_threshold, reproj_threshold=reproj_threshold,
                      depth_rel_threshold=depth_rel_threshold, num_consistent=num_consistent, sources=sources,
                      dedupe=dedupe, device=device, normals=normals, normal_angle_threshold=normal_angle_threshold,
                      jump_threshold=jump_threshold)
    plan.enqueue()
    return plan.result(with_normals=plan.normals)


def estimate_normals(depths, probs, cams, *, prob_threshold=0.8, jump_threshold=0.05, frame="world", device=None):
    """Per-view surface normals of V depth maps on the GPU (mvs_depth_normals_f32) -> (V,H,W,3) float32 numpy: unit length,
    facing the camera, (0, 0, 0) where a pixel has no normal; semantics in the module docstring.  frame "world" (default)
    or "camera" (R_v n, applied on the host)."""
    import torch
    from . import _lib
    if frame not in ("world", "camera"):
        raise ValueError('frame must be "world" or "camera", got %r' % (frame,))
    jump = check_jump_threshold(jump_threshold)
    depths, probs = FusionPlan._host(depths, "depth maps", np.float32), FusionPlan._host(probs, "probability maps", np.float32)
    if not torch.cuda.is_available():
        raise _lib.MvsnetHipError("normal estimation runs on the GPU (HIP); no GPU is visible to this process")
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        raise ValueError("normal estimation runs on a GPU device, got %s" % dev)
    dev = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())

    def views(x, name):
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float32:
                raise ValueError("%s must be float32, got %s" % (name, x.dtype))
            return x.to(dev).contiguous()
        return torch.as_tensor(x).to(dev)

    d, p = views(depths, "depth maps"), views(probs, "probability maps")
    if d.dim() != 3 or p.shape != d.shape:
        raise ValueError("depths and probs must be (V,H,W) of one size, got %s and %s" % (tuple(d.shape), tuple(p.shape)))
    V, H, W = d.shape
    cams = np.asarray(cams.cpu().numpy() if hasattr(cams, "cpu") else cams, np.float64)
    if cams.shape != (V, 2, 4, 4):
        raise ValueError("cams must be (%d,2,4,4), got %s" % (V, cams.shape))
    tables = torch.as_tensor(camera_tables(cams)).to(dev)
    out = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().mvs_depth_normals_f32(_lib.ptr(d), _lib.ptr(p), V, H, W, _lib.ptr(tables), float(prob_threshold), jump,
                                               _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "mvs_depth_normals_f32")
    n = out.cpu().numpy()
    if frame == "camera":
        n = np.einsum("vij,vhwj->vhwi", cams[:, 0, :3, :3], n.astype(np.float64)).astype(np.float32)
    return n
