"""Simplification of a triangle mesh on the MI355X by vertex clustering: the vertices that fall into one cell of a uniform grid
become one vertex at their mean, and the faces follow.  The stage after the extraction of a mesh (mvsnet_amd.mesh) and the
removal of its small pieces (mvsnet_amd.mesh_clean), for any mesh that already exists.

    python -m mvsnet_amd.mesh_simplify --mesh IN.ply --out OUT.ply --cell C [--origin x:y:z] [--force]

The kernels are csrc/mesh_simplify.hip (mvs_mesh_cluster_keys_f32, mvs_mesh_cluster_heads_i64, mvs_mesh_cluster_sums_f32,
mvs_mesh_cluster_faces_i32, mvs_mesh_cluster_mark_i32) and mesh_components.hip's mvs_mesh_compact_write_f32; torch owns the
device memory, the stable sorts, the prefix sums and the one read-back that sizes the outputs.

Semantics (shared by the kernels, tests/mesh_simplify_reference.py and the tests).
  * Input: vertices (M,3) float32, colours (M,3) uint8 or None, faces (F,3) int32; M and F are at most 2^31 - 1.  cell is a
    finite float32 > 0, origin three finite float32.  With origin = None it is the per-axis minimum over the vertices whose
    three coordinates are finite (ValueError when there is none while F > 0; zeros when F = 0), and the extent of those
    vertices over the cell must stay below 2^21 on every axis (ValueError).
  * Cell of a vertex, in float64, every operation rounded on its own (no contraction), as mvs_voxel_keys_f32 does: per axis
    u = (double(x) - double(o)) / double(cell) and k = floor(u).  A vertex is clusterable when its coordinates are finite and
    every k lies in 0 .. 2^21 - 1 (NaN and +-inf fail the comparisons).  Its key is kx | ky << 21 | kz << 42 and its offset
    the integer q = floor((u - k) 2^20) per axis, in 0 .. 2^20 - 1; u - k and the product are exact.
  * Invalid faces.  A face is invalid when it names an index outside 0..M-1 (its vertices are then never dereferenced) or a
    vertex that is not clusterable.  Invalid faces are dropped and counted.  A face that repeats an index is valid (and ends
    up degenerate).
  * Clusters.  Only vertices that a valid face names contribute.  There is one cluster per distinct key among them, with n
    members, the integer sums S (3 x int64) of their offsets and C (3 x int64) of their colour bytes.  Its position per
    axis: a = double(S) / double(n 2^20); b = double(k) + a; c = b double(cell); d = double(o) + c; float32(d), each step
    rounded.  Its colour byte is (2 C + n) // (2 n), mesh.py's rounding.  All sums are integers: any order gives the same bytes.
  * Faces.  A valid face maps to the clusters of its three vertices; it is degenerate when two of them are equal.  Two
    faces that are not degenerate are duplicates when they name the same set of three clusters, in any order or
    orientation; of a set of duplicates the face with the smallest input index stays.  The surviving faces keep the input
    order and their own winding.
  * Output.  The clusters that a surviving face names, in ascending key order, with their colours; faces re-indexed to
    match.  There is no unreferenced vertex in the output.
  * Report: vertices_in, vertices_out, faces_in, faces_out, clusters, invalid_faces, degenerate_faces, duplicate_faces,
    unclusterable_vertices (of all M), cell, origin.  No kernel has a capped loop, so there is no error word.

How far a cluster's vertex lies from the mean of its members.  With f_i = u_i - k the fraction of member i, q_i / 2^20 <=
f_i < (q_i + 1) / 2^20, so S / (n 2^20) lies in (mean f - 2^-20, mean f]: per axis the position is within cell 2^-20 of
o + (k + mean f) cell.  What is left is rounding: of the result to float32, at most 2^-24 |d|, and of the float64 steps on
either side (u, the quotient, b, c, d; the twin's sum of n coordinates), each at most 2^-53 of a magnitude below
|o| + max |x| + cell.  The tests assert, per axis and with s = |o| + max |x_i| + cell,

    |position - mean_i double(x_i)|  <=  cell 2^-20  +  2^-24 s  +  (n + 8) 2^-52 s.

Paths.  The cluster indices of a face's ascending triple fit one int64 key while M <= 2^21 (the cluster count is known only
after the read-back; M bounds it); a larger mesh, or two_keys=True, takes two int64 keys and two stable sorts, least
significant first.  Both give the same bytes.
"""
from __future__ import annotations

import argparse
import math
import sys

import numpy as np

from .mesh_common import MAX_SIZE, arrays, number, ply_to_ply, refuse_existing, run, shapes

WHAT = "mesh simplification"
CELLS = 2 ** 21            # cells per axis; also the number of vertices up to which one int64 holds a face's three clusters
REPORT_FIELDS = ("vertices_in", "vertices_out", "faces_in", "faces_out", "clusters", "invalid_faces", "degenerate_faces",
                 "duplicate_faces", "unclusterable_vertices", "cell", "origin")


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def check_cell(cell):
    """-> the cell as a float that is exactly a float32; ValueError unless it is finite and > 0."""
    c = number("cell", cell, float32=True)
    if not (c > 0 and math.isfinite(c)):
        raise ValueError("cell must be positive and finite in float32, got %r" % (cell,))
    return c


def check_origin(origin):
    """-> (3,) float32; ValueError unless three finite numbers."""
    try:
        o = np.asarray(origin, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("origin must be three finite numbers, got %r" % (origin,))
    with np.errstate(over="ignore"):
        o32 = o.astype(np.float32)
    if o.shape != (3,) or not np.isfinite(o32).all():
        raise ValueError("origin must be three finite numbers, got %r" % (origin,))
    return o32


def check_options(cell, origin):
    """-> (cell, origin) as simplify_device takes them: check_cell and check_origin."""
    return check_cell(cell), check_origin(origin)


def check_voxels(simplify_voxels):
    """The cell in voxels as the command lines take it: None or 0 is off -> None; else a finite float > 0."""
    if simplify_voxels is None:
        return None
    s = number("simplify_voxels", simplify_voxels)
    if s == 0:
        return None
    if not (s > 0 and math.isfinite(s)):
        raise ValueError("simplify_voxels must be positive and finite, got %r" % (simplify_voxels,))
    return s


def parse_origin(text):
    """"x:y:z" -> (3,) float32."""
    tok = str(text).split(":")
    try:
        if len(tok) != 3:
            raise ValueError
        return check_origin([float(t) for t in tok])
    except ValueError:
        raise ValueError("origin %r: x:y:z with three finite numbers expected" % (text,))


def check_extent(lo, hi, cell):
    """With the origin at lo: every axis of the box [lo, hi] must span fewer than 2^21 cells."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if ((hi - lo) / float(cell) >= CELLS).any():
        raise ValueError("the mesh spans %s cells of %g: more than 2^21 on an axis" % ((hi - lo) / float(cell), cell))


# ------------------------------------------------------------------------------------------------ device side

def _default_origin(v, F, cell):
    """The minimum over the finite vertices of a device tensor, checked against the cell (one read-back of six numbers)."""
    import torch
    finite = torch.isfinite(v).all(1)
    w = v[finite]
    if w.shape[0] == 0:
        if F > 0:
            raise ValueError("no vertex has three finite coordinates: nothing to place the cells by (give an origin)")
        return np.zeros(3, np.float32)
    box = torch.stack([w.min(0)[0], w.max(0)[0]]).cpu().numpy()
    check_extent(box[0], box[1], cell)
    return box[0].astype(np.float32)


def simplify_device(vertices, colours, faces, dev, cell, origin, two_keys=None):
    """simplify_mesh on contiguous device tensors, with an origin -> (vertices, colours or None, faces, report), tensors on the
    device.  two_keys: None chooses by M, True forces the two-key sort of the faces (for tests: both give the same bytes)."""
    import torch
    from . import _lib
    cell, origin = check_options(cell, origin)
    M, F = shapes(vertices, colours, faces)
    two = M > CELLS if two_keys is None else bool(two_keys)
    if not two and M > CELLS:
        raise ValueError("one key holds the clusters of a face only up to 2^21 vertices, got %d" % M)
    lib = _lib.load()
    ox, oy, oz = (float(x) for x in origin)
    i32, i64 = torch.int32, torch.int64
    with torch.cuda.device(dev):
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        st = _lib.stream_ptr
        wsb = lib.mvs_mesh_cluster_workspace_bytes(M, F)
        ws = new(wsb, torch.uint8)
        keys, offsets = new(M, i64), new((M, 3), i32)
        _lib.check(lib.mvs_mesh_cluster_keys_f32(_lib.ptr(vertices), M, _lib.ptr(faces), F, ox, oy, oz, cell, _lib.ptr(keys),
                                                 _lib.ptr(offsets), _lib.ptr(ws), wsb, st()), "mvs_mesh_cluster_keys_f32")
        sorted_keys, order = torch.sort(keys, stable=True)
        head = new(M, i32)
        _lib.check(lib.mvs_mesh_cluster_heads_i64(_lib.ptr(sorted_keys), M, _lib.ptr(head), st()), "mvs_mesh_cluster_heads_i64")
        head_rank = torch.cumsum(head, 0, dtype=i32)
        vertex_cluster, cluster_v = new(M, i32), new((M, 3), torch.float32)
        cluster_c = None if colours is None else new((M, 3), torch.uint8)
        _lib.check(lib.mvs_mesh_cluster_sums_f32(_lib.ptr(sorted_keys), _lib.ptr(order), _lib.ptr(head_rank), _lib.ptr(offsets),
                                                 _lib.ptr(colours), M, ox, oy, oz, cell, _lib.ptr(vertex_cluster), _lib.ptr(cluster_v),
                                                 _lib.ptr(cluster_c), _lib.ptr(ws), wsb, st()), "mvs_mesh_cluster_sums_f32")
        cluster_f, key_lo = new((F, 3), i32), new(F, i64)
        key_hi = new(F, i64) if two else None
        _lib.check(lib.mvs_mesh_cluster_faces_i32(_lib.ptr(faces), M, F, _lib.ptr(vertex_cluster), _lib.ptr(cluster_f), _lib.ptr(key_lo),
                                                  _lib.ptr(key_hi), _lib.ptr(ws), wsb, st()), "mvs_mesh_cluster_faces_i32")
        if two:                                                                 # least significant key first, both sorts stable
            lo1, by_lo = torch.sort(key_lo, stable=True)
            sorted_hi, by_hi = torch.sort(key_hi[by_lo], stable=True)
            sorted_lo, face_order = lo1[by_hi].contiguous(), by_lo[by_hi].contiguous()
        else:
            (sorted_lo, face_order), sorted_hi = torch.sort(key_lo, stable=True), None
        face_keep, vertex_keep = new(F, i32), new(M, i32)
        _lib.check(lib.mvs_mesh_cluster_mark_i32(_lib.ptr(cluster_f), M, F, _lib.ptr(sorted_lo), _lib.ptr(sorted_hi), _lib.ptr(face_order),
                                                 _lib.ptr(face_keep), _lib.ptr(vertex_keep), _lib.ptr(ws), wsb, st()),
                   "mvs_mesh_cluster_mark_i32")
        face_rank = torch.cumsum(face_keep, 0, dtype=i32)
        vertex_rank = torch.cumsum(vertex_keep, 0, dtype=i32)
        zero = torch.zeros(1, dtype=i32, device=dev)
        last = lambda t: t[-1:] if t.numel() else zero
        sizes = torch.cat([ws[:16].view(i32), last(head_rank), last(face_rank), last(vertex_rank)]).cpu().numpy()   # the one read-back
        invalid, unclusterable, degenerate, duplicate, K, F_out, M_out = (int(x) for x in sizes)
        out_v = new((M_out, 3), torch.float32)
        out_c = None if colours is None else new((M_out, 3), torch.uint8)
        out_f = new((F_out, 3), i32)
        rc = lib.mvs_mesh_compact_write_f32(
            _lib.ptr(cluster_v), _lib.ptr(cluster_c), K, _lib.ptr(cluster_f), F, _lib.ptr(face_keep), _lib.ptr(face_rank),
            _lib.ptr(vertex_keep), _lib.ptr(vertex_rank), M_out, F_out, _lib.ptr(out_v), _lib.ptr(out_c), _lib.ptr(out_f), st())
        _lib.check(rc, "mvs_mesh_compact_write_f32")
        report = {"vertices_in": M, "vertices_out": M_out, "faces_in": F, "faces_out": F_out, "clusters": K, "invalid_faces": invalid,
                  "degenerate_faces": degenerate, "duplicate_faces": duplicate, "unclusterable_vertices": unclusterable,
                  "cell": cell, "origin": [ox, oy, oz]}
        return out_v, out_c, out_f, report


def simplify_mesh(vertices, colours, faces, cell, origin=None, device=None, *, two_keys=None):
    """-> (vertices (M',3) float32, colours (M',3) uint8 or None, faces (F',3) int32, report): numpy arrays, or tensors on the
    device when the vertices came as a tensor."""
    import torch
    cell = check_cell(cell)                                                    # before any GPU work
    origin = None if origin is None else check_origin(origin)
    M, F = arrays(vertices, colours, faces)
    if origin is None and not isinstance(vertices, torch.Tensor):              # arrays place their default origin on the host
        v = np.asarray(vertices, np.float32)
        finite = v[np.isfinite(v).all(1)]
        if len(finite) == 0 and F > 0:
            raise ValueError("no vertex has three finite coordinates: nothing to place the cells by (give an origin)")
        origin = finite.min(0) if len(finite) else np.zeros(3, np.float32)
        if len(finite):
            check_extent(origin, finite.max(0), cell)

    def stage(dev, v, c, f):
        with torch.cuda.device(dev):
            return simplify_device(v, c, f, dev, cell, _default_origin(v, F, cell) if origin is None else origin, two_keys=two_keys)

    return run(vertices, colours, faces, device, WHAT, stage)


# ------------------------------------------------------------------------------------------------ command line

def add_options(ap, prefix=""):
    """--simplify_voxels, as mesh.py and depthfusion.py take it (there under a prefix) -> its action."""
    return [ap.add_argument("--%ssimplify_voxels" % prefix, type=float, default=None,
                            help="simplify the mesh by vertex clustering in cells of this many voxels (not necessarily an integer)")]


def check_arguments(a, prefix=""):
    """The option of add_options on a parsed namespace -> dict(voxels), or None without it; ValueError naming the flag
    otherwise.  A given 0 is refused here, though check_voxels takes it for "off".  mesh.py and depthfusion.py (the prefix
    "mesh_") have worded this refusal differently ever since each got the flag, and both wordings are kept."""
    given = getattr(a, prefix + "simplify_voxels")
    if given is None:
        return None
    try:
        if check_voxels(given) is None:
            raise ValueError("0 given")
    except ValueError as e:
        raise ValueError("--%ssimplify_voxels must be positive and finite%s" % (prefix, " (%s)" % e if prefix else ", got %r" % (given,)))
    return dict(voxels=given)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="input PLY, as mvsnet_amd.mesh writes it")
    ap.add_argument("--out", required=True, help="output PLY")
    ap.add_argument("--cell", type=float, required=True, help="edge of a cell in world units")
    ap.add_argument("--origin", default=None, help="x:y:z, a corner of the grid of cells (default: the minimum of the finite vertices)")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    try:
        a.cell = check_cell(a.cell)
        a.origin = None if a.origin is None else parse_origin(a.origin)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.mesh_simplify: --%s" % e)
    return a


def prepare_output(a):
    return refuse_existing("mesh_simplify", a.out, a.force)


def main(argv=None):
    a = parse_args(argv)
    return ply_to_ply("mesh_simplify", a, lambda v, c, f: simplify_mesh(v, c, f, a.cell, a.origin))


if __name__ == "__main__":
    sys.exit(main())
