"""Sampling of a triangle mesh's surface into a point cloud on the MI355X: the step that lets mvsnet_amd.evaluate score a
mesh (as DTU and Tanks and Temples do), since the vertices of a simplified mesh no longer cover its surface.

    python -m mvsnet_amd.mesh_sample --mesh IN.ply --out OUT.ply --spacing s [--seed n] [--normals] [--force]

The kernels are csrc/mesh_sample.hip (mvs_mesh_sample_quota_f32, mvs_mesh_sample_write_f32); torch owns the device memory, the
inclusive int64 scan between the two calls and the one read-back that sizes the outputs.

Semantics (shared by the kernels, tests/mesh_sample_reference.py and the tests).  Everything is deterministic, and integer
wherever an order of summation could matter.
  * Input: vertices (M,3) float32, colours (M,3) uint8 or None, faces (F,3) int32, M <= 2^31 - 1 and F <= 2^26 (ValueError);
    density, a float > 0 and finite, in samples per unit area (the command lines take a spacing s: density =
    1.0 / (float(s) * float(s))); seed, an integer of 64 bits, 0 by default.
  * Quota of a face.  A face is invalid when an index lies outside 0..M-1 (its vertices are then never dereferenced) or a
    vertex it names is not finite.  Otherwise, in float64 with every operation rounded on its own (no contraction) and
    a, b, c its three vertices: e1 = b - a, e2 = c - a, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
    A2 = (nx nx + ny ny) + nz nz, t = ((sqrt(A2) 0.5) density) 65536.  The face has zero area when A2 == 0 (a repeated
    index, three collinear vertices), it is saturated when not t < 2^36 (+inf included; t cannot be NaN), and otherwise
    q = int64(floor(t)): the expected number of its samples in units of 2^-16.  q = 0 for invalid, zero-area and saturated
    faces, which are counted; a saturated face is a ValueError.  With F <= 2^26 the sum of q stays below 2^62.
  * Counts by error diffusion.  I = the inclusive int64 sum of q, E = I - q.  Face f owns the samples E_f >> 16 up to
    (I_f >> 16) - 1: the floor or the ceiling of q_f / 65536 of them, and faces that expect less than one sample still
    get their share, in face order (ten faces of 0.3 give 0 0 0 1 0 0 1 0 0 0).  There are N = I_last >> 16 samples;
    N > max_samples (2^27 by default) or N > 2^31 - 1 is a ValueError, raised before any output is allocated.
  * Sample g, in the first face f with (I_f >> 16) > g.  mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) *
    0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31, in uint64.  h = mix(mix(seed) ^ g),
    k1 = h >> 40, k2 = (h >> 16) & 0xFFFFFF.  When k1 + k2 >= 2^24 both are folded, k -> 2^24 - 1 - k.  The weights are
    integers in units of 2^-25: wu = 2 k1 + 1, wv = 2 k2 + 1, w0 = 2^25 - wu - wv >= 0.
    Position: float32((a + u (b - a)) + v (c - a)) per axis with u = wu 2^-25, v = wv 2^-25, in float64, each step rounded.
    Colour byte: (w0 ca + wu cb + wv cc + 2^24) >> 25, in integers.  Normal: float32(n / sqrt(A2)) per component, the
    unit normal of the face by its winding.  Face index: f.  Samples stand in face order, g ascending.
  * Stats: faces, invalid, zero_area, samples, area = sum(q) / 65536 / density (the area the samples stand for).
The quota and the normals rest on float64 sqrt and divide being correctly rounded, on the device as in numpy.

How far a sample lies from its triangle.  With exact arithmetic the sample is a convex combination of a, b, c: inside the
triangle.  With s = the largest |coordinate| of the three vertices, per axis: b - a and c - a are rounded (|.| <= 2 s, each
2^-53 2 s), the two products are rounded and carry the differences' errors (4 of 2^-53 2 s), a + u (b - a) is at most 3 s
(3 2^-53 s), the last sum at most 5 s before it is rounded: less than 16 2^-53 s = 2^-49 s in float64, and 2^-24 s for the
rounding to float32.  The tests assert that every sample lies within sqrt(3) s (2^-24 + 2^-49) of its triangle's plane and
no further than that outside any of its edges.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

from .mesh_common import inputs, need_gpu, number, refuse_existing, shapes

WHAT = "mesh sampling"
MAX_VERTICES = 2 ** 31 - 1
MAX_FACES = 2 ** 26
MAX_SAMPLES = 2 ** 31 - 1
DEFAULT_MAX_SAMPLES = 2 ** 27
STATS_FIELDS = ("faces", "invalid", "zero_area", "samples", "area")


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def check_density(density):
    """-> the density as a float; ValueError unless it is a number, finite and > 0."""
    d = number("density", density)
    if not (d > 0 and math.isfinite(d)):
        raise ValueError("density must be positive and finite, got %r" % (density,))
    return d


def check_spacing(spacing):
    """The spacing s of the command lines -> the density 1.0 / (float(s) * float(s)); ValueError unless s and the density are
    finite and > 0."""
    s = number("spacing", spacing)
    d = 1.0 / (s * s) if s > 0 and s * s > 0 else 0.0
    if not (math.isfinite(s) and d > 0 and math.isfinite(d)):
        raise ValueError("spacing must be positive and finite, and so must 1 / spacing^2, got %r" % (spacing,))
    return d


def check_seed(seed):
    """-> the seed in 0 .. 2^64 - 1; ValueError otherwise."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an integer in 0 .. 2^64 - 1, got %r" % (seed,))
    return int(seed)


def check_max_samples(max_samples):
    if isinstance(max_samples, bool) or not isinstance(max_samples, (int, np.integer)) or int(max_samples) < 0:
        raise ValueError("max_samples must be an integer >= 0, got %r" % (max_samples,))
    return min(int(max_samples), MAX_SAMPLES)


def _shapes(vertices, colours, faces):
    M, F = shapes(vertices, colours, faces)
    if F > MAX_FACES:
        raise ValueError("%d faces are more than the 2^26 that the sampling takes" % F)
    return M, F


def read_ply_mesh(path):
    """A triangle mesh from any PLY file, ascii or binary_little_endian -> (vertices (M,3) float32, colours (M,3) uint8 or
    None, faces (F,3) int32).  The `vertex` element gives x y z (any scalar type) and, when all three are there, red green blue;
    the `face` element a list property vertex_indices or vertex_index, of any integer count and index types.  Every other
    element and property is skipped.  A face that is not a triangle, a file without faces, an index beyond int32 and a
    big-endian file are a ValueError."""
    from .evaluate import _parse_ply_header, _skip_binary_element
    with open(path, "rb") as fh:
        data = fh.read()
    fmt, elements, pos = _parse_ply_header(data, path)
    if fmt == "binary_big_endian":
        raise ValueError("%s: a big-endian PLY is not supported as a mesh" % path)
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError("%s: no vertex element" % path)
    if "face" not in names or elements[names.index("face")][1] == 0:
        raise ValueError("%s: no faces: not a mesh" % path)
    vprops = elements[names.index("vertex")][2]
    fprops = elements[names.index("face")][2]
    if any(len(p) == 4 for p in vprops):
        raise ValueError("%s: list property inside the vertex element" % path)
    vnames = [p[0] for p in vprops]
    missing = [c for c in "xyz" if c not in vnames]
    if missing:
        raise ValueError("%s: vertex element without %s" % (path, "/".join(missing)))
    lists = [p for p in fprops if len(p) == 4 and p[0] in ("vertex_indices", "vertex_index")]
    if len(lists) != 1:
        raise ValueError("%s: the face element needs one list property vertex_indices or vertex_index" % path)
    if lists[0][2][0] == "f" or lists[0][3][0] == "f":
        raise ValueError("%s: vertex_indices must have integer count and index types" % path)
    col, idx = None, None
    if fmt == "ascii":
        tok = data[pos:].split()
        at = 0
        for name, count, props in elements:
            if name == "vertex":
                need = count * len(props)
                if len(tok) - at < need:
                    raise ValueError("%s: file ends inside the vertex element" % path)
                vals = np.array(tok[at:at + need], np.float64).reshape(count, len(props))
                col = {p: vals[:, k] for k, p in enumerate(vnames)}
                at += need
                continue
            rows = [] if name == "face" else None
            for _ in range(count):
                for p in props:
                    if at >= len(tok):
                        raise ValueError("%s: file ends inside the %s element" % (path, name))
                    if len(p) == 2:
                        at += 1
                        continue
                    k = int(tok[at])
                    if rows is not None and p is lists[0]:
                        if k != 3:
                            raise ValueError("%s: a face is not a triangle" % path)
                        if at + 3 >= len(tok):
                            raise ValueError("%s: file ends inside the face element" % path)
                        rows.append(tok[at + 1:at + 4])
                    at += 1 + k
            if rows is not None:
                idx = np.array(rows, np.int64).reshape(-1, 3)
    else:
        for name, count, props in elements:
            if name == "vertex":
                dt = np.dtype([(p[0], "<" + p[1]) for p in props])
                if len(data) - pos < count * dt.itemsize:
                    raise ValueError("%s: file ends inside the vertex element" % path)
                v = np.frombuffer(data, dt, count=count, offset=pos)
                col = {p: v[p] for p in vnames}
                pos += count * dt.itemsize
            elif name == "face":
                if sum(len(p) == 4 for p in props) == 1:                       # one list: a fixed record while every face is a triangle
                    dt = np.dtype(_face_record(props))
                    whole = min(count, (len(data) - pos) // dt.itemsize)
                    f = np.frombuffer(data, dt, count=whole, offset=pos)
                    if (f["n"] != 3).any():                                    # the first record that is not a triangle is still aligned
                        raise ValueError("%s: a face is not a triangle" % path)
                    if whole < count:
                        raise ValueError("%s: file ends inside the face element" % path)
                    idx = f["i"].astype(np.int64).reshape(-1, 3)
                    pos += count * dt.itemsize
                else:
                    rows = []
                    for _ in range(count):
                        for p in props:
                            if len(p) == 2:
                                pos += np.dtype(p[1]).itemsize
                                continue
                            ct, it = np.dtype("<" + p[2]), np.dtype("<" + p[3])
                            if pos + ct.itemsize > len(data):
                                raise ValueError("%s: file ends inside the face element" % path)
                            k = int(np.frombuffer(data, ct, count=1, offset=pos)[0])
                            pos += ct.itemsize
                            if p is lists[0]:
                                if k != 3:
                                    raise ValueError("%s: a face is not a triangle" % path)
                                if pos + 3 * it.itemsize > len(data):
                                    raise ValueError("%s: file ends inside the face element" % path)
                                rows.append(np.frombuffer(data, it, count=3, offset=pos).astype(np.int64))
                            pos += k * it.itemsize
                    idx = np.array(rows, np.int64).reshape(-1, 3)
            else:
                pos = _skip_binary_element(data, pos, count, props, "<", path)
    vertices = np.stack([col["x"], col["y"], col["z"]], 1).astype(np.float32)
    colours = None
    if all(c in col for c in ("red", "green", "blue")):
        colours = np.stack([np.clip(col[c], 0, 255) for c in ("red", "green", "blue")], 1).astype(np.uint8)
    if len(idx) and (idx.min() < -2 ** 31 or idx.max() > 2 ** 31 - 1):
        raise ValueError("%s: a vertex index is beyond int32" % path)
    return vertices, colours, np.ascontiguousarray(idx.astype(np.int32))


def _face_record(props):
    """The fixed record of a binary face element with one list property, while that list has three entries: count "n" and
    indices "i", the scalar properties around them as "s<k>"."""
    out = []
    for k, p in enumerate(props):
        if len(p) == 4:
            out += [("n", "<" + p[2]), ("i", "<" + p[3], (3,))]
        else:
            out.append(("s%d" % k, "<" + p[1]))
    return out


# ------------------------------------------------------------------------------------------------ device side

def sample_device(vertices, colours, faces, dev, density, seed=0, *, normals=False, face_index=False, max_samples=DEFAULT_MAX_SAMPLES):
    """sample_mesh on contiguous device tensors -> ({"xyz" (N,3) float32, "colours" (N,3) uint8 or None, "normals" (N,3)
    float32 or None, "face_index" (N,) int32 or None}, stats), tensors on the device.  One synchronisation: the read-back of
    the status words and the last sum."""
    import torch
    from . import _lib
    density, seed, max_samples = check_density(density), check_seed(seed), check_max_samples(max_samples)
    M, F = _shapes(vertices, colours, faces)
    lib = _lib.load()
    i32, i64 = torch.int32, torch.int64
    with torch.cuda.device(dev):
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        wsb = lib.mvs_mesh_sample_workspace_bytes(M, F)
        ws, quota = new(wsb, torch.uint8), new(F, i64)
        _lib.check(lib.mvs_mesh_sample_quota_f32(_lib.ptr(vertices), M, _lib.ptr(faces), F, density, _lib.ptr(quota), _lib.ptr(ws), wsb,
                                                 _lib.stream_ptr()), "mvs_mesh_sample_quota_f32")
        sums = torch.cumsum(quota, 0, dtype=i64)                               # exact: integers
        last = sums[-1:] if F else torch.zeros(1, dtype=i64, device=dev)
        host = torch.cat([ws[:12].view(i32).to(i64), last]).cpu().numpy()      # the one read-back
        invalid, zero_area, saturated, total = (int(x) for x in host)
        if saturated:
            raise ValueError("%d faces expect 2^20 samples or more each at density %g: the mesh and the spacing do not belong "
                             "together" % (saturated, density))
        N = total >> 16
        if N > max_samples:
            raise ValueError("%d samples are more than max_samples = %d (a larger spacing gives fewer)" % (N, max_samples))
        out = {"xyz": new((N, 3), torch.float32), "colours": None if colours is None else new((N, 3), torch.uint8),
               "normals": new((N, 3), torch.float32) if normals else None, "face_index": new(N, i32) if face_index else None}
        _lib.check(lib.mvs_mesh_sample_write_f32(_lib.ptr(vertices), _lib.ptr(colours), M, _lib.ptr(faces), F, _lib.ptr(sums), N, seed,
                                                 _lib.ptr(out["xyz"]), _lib.ptr(out["face_index"]), _lib.ptr(out["colours"]),
                                                 _lib.ptr(out["normals"]), _lib.stream_ptr()), "mvs_mesh_sample_write_f32")
    stats = {"faces": F, "invalid": invalid, "zero_area": zero_area, "samples": N, "area": total / 65536.0 / density}
    return out, stats


def sample_mesh(vertices, colours, faces, density, seed=0, device=None, *, normals=False, face_index=False,
                max_samples=DEFAULT_MAX_SAMPLES):
    """-> ({"xyz", "colours", "normals", "face_index"}, stats): numpy arrays, or tensors on the device when the vertices came
    as a tensor; an output that was not asked for (or colours without input colours) is None."""
    import torch
    density, seed, max_samples = check_density(density), check_seed(seed), check_max_samples(max_samples)   # before any GPU work
    dev, v, c, f = inputs(vertices, colours, faces, device, WHAT, _shapes)
    out, stats = sample_device(v, c, f, dev, density, seed, normals=normals, face_index=face_index, max_samples=max_samples)
    if not isinstance(vertices, torch.Tensor):
        out = {k: None if t is None else t.cpu().numpy() for k, t in out.items()}
    return out, stats


# ------------------------------------------------------------------------------------------------ command line

def add_options(ap, prefix=""):
    """--<prefix>spacing, as evaluate.py ("pred_", "gt_"), mesh.py ("eval_") and depthfusion.py ("mesh_eval_") take it: off
    by default."""
    ap.add_argument("--%sspacing" % prefix, type=float, default=None,
                    help="sample the mesh's surface at about this distance between samples (1 / spacing^2 samples per unit area)")


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="input PLY: any triangle mesh, ascii or binary little-endian")
    ap.add_argument("--out", required=True, help="output PLY: a point cloud as mvsnet_amd.fusion writes it")
    ap.add_argument("--spacing", type=float, required=True, help="about the distance between samples: 1 / spacing^2 per unit area")
    ap.add_argument("--seed", type=int, default=0, help="seed of the positions inside the triangles (0 .. 2^64 - 1)")
    ap.add_argument("--normals", action="store_true", help="write the face normals with the samples")
    ap.add_argument("--max_samples", type=int, default=DEFAULT_MAX_SAMPLES, help="refuse to write more samples than this")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    try:
        a.density = check_spacing(a.spacing)
        a.seed = check_seed(a.seed)
        a.max_samples = check_max_samples(a.max_samples)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.mesh_sample: --%s" % e)
    return a


def prepare_output(a):
    return refuse_existing("mesh_sample", a.out, a.force)


def main(argv=None):
    a = parse_args(argv)
    out = prepare_output(a)
    need_gpu("mesh_sample")
    from .fusion import write_ply
    try:
        vertices, colours, faces = read_ply_mesh(a.mesh)
        cloud, stats = sample_mesh(vertices, colours, faces, a.density, a.seed, normals=a.normals, max_samples=a.max_samples)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        rgb = cloud["colours"] if cloud["colours"] is not None else np.zeros((len(cloud["xyz"]), 3), np.uint8)   # no colours: black
        write_ply(out, cloud["xyz"], rgb, cloud["normals"])
    except (ValueError, OSError) as e:
        raise SystemExit("mvsnet_amd.mesh_sample: %s" % e)
    print(json.dumps(dict(stats, spacing=a.spacing, seed=a.seed, out=out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
