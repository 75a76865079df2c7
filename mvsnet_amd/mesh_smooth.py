"""Taubin smoothing of a triangle mesh on the MI355X: the lambda | mu relaxation that takes the voxel-scale noise out of a
surface-nets mesh without shrinking it.  The stage after the removal of small pieces (mvsnet_amd.mesh_clean) and before the
simplification (mvsnet_amd.mesh_simplify), for any mesh that already exists.

    python -m mvsnet_amd.mesh_smooth --mesh IN.ply --out OUT.ply --iterations N [--lambda 0.5] [--mu -0.53]
        [--boundary fixed|curve|free] [--max_displacement r] [--force]

The kernels are csrc/mesh_smooth.hip (mvs_mesh_smooth_edges_i64, mvs_mesh_smooth_heads_i64, mvs_mesh_smooth_rows_i32,
mvs_mesh_smooth_step_f32); torch owns the device memory, the sort of the edge keys, the inclusive scan of the heads and the one
read-back of the counts, which happens after the last pass has been enqueued.

Semantics (shared by the kernels, tests/mesh_smooth_reference.py and the tests).
  * Input: vertices (M,3) float32, colours (M,3) uint8 or None, faces (F,3) int32; M <= 2^31 - 1 and 6 F <= 2^31 - 1.  Colours
    and faces leave the call unchanged, byte for byte; only positions move.
  * Parameters: iterations, an integer 1 .. 1000; lam, a float32 in (0, 1], default 0.5; mu, a float32 in [-1, 0], default
    -0.53 (Taubin's pair); mu == 0 is plain Laplacian relaxation, one pass per iteration; boundary "fixed" (default), "curve" or
    "free"; max_displacement None or a finite float32 r > 0.  Anything else is a ValueError, raised before any GPU work.
  * Live edges.  A face is valid when its three indices lie in 0 .. M - 1; invalid faces are counted and their vertices are
    never dereferenced.  A vertex is finite when its three input coordinates are finite, decided once from the input.  A valid
    face (a, b, c) emits the six directed edges a>b, b>a, b>c, c>b, c>a, a>c.  A directed edge s>t is live when s != t and both
    ends are finite; its key is int64(s) << 31 | t, and a dead edge has the key 2^63 - 1.
  * Adjacency.  The 6 F keys are sorted; the distinct live keys, ascending, are the U unique directed edges.  The neighbours
    of v are the targets of its unique edges, ascending.  The multiplicity of an edge is the length of its run of equal keys
    (the runs of s>t and t>s have the same length by construction): 1 is a boundary edge, 3 or more a non-manifold edge; a
    face given twice makes its edges multiplicity 2, not boundary and not an error.  A vertex is a boundary vertex when one of
    its unique edges is a boundary edge.
  * Class of a vertex, decided once.  fixed: the vertex is not finite, or has no neighbour, or boundary == "fixed" and it is
    a boundary vertex.  curve: boundary == "curve" and it is a boundary vertex; its neighbour set is then only the targets of
    its boundary edges (at least one).  interior: everything else; its neighbour set is all its neighbours.
  * One pass with factor f reads buffer X and writes buffer Y (Jacobi: no vertex sees another's new position).  A fixed
    vertex is copied bit for bit.  Otherwise, per axis and in float64, every operation rounded on its own (no contraction,
    a correctly rounded quotient): s = 0, then s += double(X[j]) over the neighbour set in ascending j, one after the other;
    m = s / double(n); d = m - double(X[v]); e = double(f) d; y = double(X[v]) + e; with r: lo = double(V0[v]) - double(r),
    hi = double(V0[v]) + double(r), y = min(max(y, lo), hi), V0 the input position of the call; Y[v] = float32(y).  If any of
    the three results is not finite, the vertex keeps X[v] on all three axes.
  * One iteration: a pass with lam, then, unless mu == 0, a pass with mu.  The result is the buffer after `iterations` of them.
  * Report: vertices, faces, invalid_faces, non_finite_vertices, edges (U / 2), boundary_edges, non_manifold_edges (an
    undirected edge counts once), boundary_vertices, fixed_vertices, iterations, lam, mu, boundary, max_displacement.  No
    kernel has a capped loop, so there is no error word.
"""
from __future__ import annotations

import argparse
import math
import sys

from . import mesh_common
from .mesh_common import MAX_SIZE, integer, number, ply_to_ply, refuse_existing, run

WHAT = "mesh smoothing"
MAX_ITERATIONS = 1000
BOUNDARIES = ("fixed", "curve", "free")             # the kernels take the index
OPTION_NAMES = ("iterations", "lam", "mu", "boundary", "max_displacement")
REPORT_FIELDS = ("vertices", "faces", "invalid_faces", "non_finite_vertices", "edges", "boundary_edges", "non_manifold_edges",
                 "boundary_vertices", "fixed_vertices") + OPTION_NAMES
ROW_FLOATS = 3                                      # the step's row width: (M,3) as a mesh arrives; padded to 4 it measured slower


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def check_iterations(iterations, least=1):
    n = integer(iterations, least, MAX_ITERATIONS)
    if n is None:
        raise ValueError("iterations must be an integer %d .. %d, got %r" % (least, MAX_ITERATIONS, iterations))
    return n


def check_options(iterations, lam=0.5, mu=-0.53, boundary="fixed", max_displacement=None):
    """-> (iterations, lam, mu, boundary, max_displacement) with the floats exactly float32; ValueError otherwise."""
    iterations = check_iterations(iterations)
    l32, m32 = number("lam", lam, float32=True), number("mu", mu, float32=True)
    if not 0 < l32 <= 1:
        raise ValueError("lam must lie in (0, 1] as a float32, got %r" % (lam,))
    if not -1 <= m32 <= 0:
        raise ValueError("mu must lie in [-1, 0] as a float32, got %r" % (mu,))
    if not isinstance(boundary, str) or boundary not in BOUNDARIES:
        raise ValueError("boundary must be one of %s, got %r" % (", ".join(BOUNDARIES), boundary))
    r = None
    if max_displacement is not None:
        r = number("max_displacement", max_displacement, float32=True)
        if not (r > 0 and math.isfinite(r)):
            raise ValueError("max_displacement must be positive and finite in float32, got %r" % (max_displacement,))
    return iterations, l32, m32 + 0.0, boundary, r


def check_voxels(max_voxels):
    """--smooth_max_voxels as the command lines take it: a finite float > 0."""
    s = number("smooth_max_voxels", max_voxels)
    if not (s > 0 and math.isfinite(s)):
        raise ValueError("smooth_max_voxels must be positive and finite, got %r" % (max_voxels,))
    return s


def _shapes(vertices, colours, faces):
    M, F = mesh_common.shapes(vertices, colours, faces)
    if 6 * F > MAX_SIZE:
        raise ValueError("a mesh of %d faces has more than 2^31 - 1 directed edges" % F)
    return M, F


# ------------------------------------------------------------------------------------------------ device side

def smooth_device(vertices, colours, faces, dev, iterations, lam=0.5, mu=-0.53, boundary="fixed", max_displacement=None):
    """smooth_mesh on contiguous device tensors -> (vertices, colours, faces, report): the vertices are a new tensor, colours and
    faces the ones that came in.  Everything is enqueued on torch's current stream; the one read-back comes last."""
    import torch
    from . import _lib
    iterations, lam, mu, boundary, r = check_options(iterations, lam, mu, boundary, max_displacement)
    M, F = _shapes(vertices, colours, faces)
    E = 6 * F
    lib = _lib.load()
    i32 = torch.int32
    with torch.cuda.device(dev):
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        st = _lib.stream_ptr
        wsb = lib.mvs_mesh_smooth_workspace_bytes(M, F)
        ws = new(wsb, torch.uint8)
        keys = new(E, torch.int64)
        _lib.check(lib.mvs_mesh_smooth_edges_i64(_lib.ptr(vertices), M, _lib.ptr(faces), F, _lib.ptr(keys), _lib.ptr(ws), wsb, st()),
                   "mvs_mesh_smooth_edges_i64")
        sorted_keys = torch.sort(keys)[0]
        head = new(E, i32)
        _lib.check(lib.mvs_mesh_smooth_heads_i64(_lib.ptr(sorted_keys), F, _lib.ptr(head), _lib.ptr(ws), wsb, st()),
                   "mvs_mesh_smooth_heads_i64")
        head_rank = torch.cumsum(head, 0, dtype=i32)
        neighbours, row_start, vertex_class = new(E, i32), new(M + 1, i32), new(M, torch.uint8)
        _lib.check(lib.mvs_mesh_smooth_rows_i32(_lib.ptr(sorted_keys), _lib.ptr(head), _lib.ptr(head_rank), M, F,
                                                BOUNDARIES.index(boundary), _lib.ptr(neighbours), _lib.ptr(row_start),
                                                _lib.ptr(vertex_class), _lib.ptr(ws), wsb, st()), "mvs_mesh_smooth_rows_i32")
        x, passes = vertices, 0
        buffers = [new((M, 3), torch.float32) for _ in range(2)]               # the passes alternate; the input is never written
        for _ in range(iterations):
            for factor in (lam, mu) if mu != 0 else (lam,):
                y = buffers[passes % 2]
                _lib.check(lib.mvs_mesh_smooth_step_f32(_lib.ptr(x), _lib.ptr(vertices), _lib.ptr(row_start), _lib.ptr(neighbours),
                                                        _lib.ptr(vertex_class), M, E, ROW_FLOATS, factor, -1.0 if r is None else r,
                                                        _lib.ptr(y), st()), "mvs_mesh_smooth_step_f32")
                x, passes = y, passes + 1
        zero = torch.zeros(1, dtype=i32, device=dev)
        counts = torch.cat([ws[:24].view(i32), head_rank[-1:] if E else zero]).cpu().numpy()         # the one read-back
        invalid, non_finite, boundary_edges, non_manifold, boundary_vertices, fixed, U = (int(c) for c in counts)
        report = {"vertices": M, "faces": F, "invalid_faces": invalid, "non_finite_vertices": non_finite, "edges": U // 2,
                  "boundary_edges": boundary_edges, "non_manifold_edges": non_manifold, "boundary_vertices": boundary_vertices,
                  "fixed_vertices": fixed, "iterations": iterations, "lam": lam, "mu": mu, "boundary": boundary, "max_displacement": r}
        return x, colours, faces, report


def smooth_mesh(vertices, colours, faces, iterations, lam=0.5, mu=-0.53, boundary="fixed", max_displacement=None, device=None):
    """-> (vertices (M,3) float32, colours (M,3) uint8 or None, faces (F,3) int32, report): numpy arrays, or tensors on the
    device when the vertices came as a tensor."""
    options = check_options(iterations, lam, mu, boundary, max_displacement)   # before any GPU work
    return run(vertices, colours, faces, device, WHAT, lambda dev, v, c, f: smooth_device(v, c, f, dev, *options), _shapes)


# ------------------------------------------------------------------------------------------------ command line

def add_options(ap, prefix=""):
    """--smooth_iterations and its companions, as mesh.py and depthfusion.py take them (there under a prefix) -> their actions."""
    return [ap.add_argument("--%ssmooth_iterations" % prefix, type=int, default=0, help="Taubin smoothing iterations of the mesh (0: none)"),
            ap.add_argument("--%ssmooth_lambda" % prefix, type=float, default=0.5, help="smoothing: the shrinking factor, in (0, 1]"),
            ap.add_argument("--%ssmooth_mu" % prefix, type=float, default=-0.53, help="smoothing: the inflating factor, in [-1, 0] (0: Laplacian)"),
            ap.add_argument("--%ssmooth_boundary" % prefix, choices=BOUNDARIES, default="fixed",
                            help="smoothing: boundary vertices stay, move along the boundary curve, or move freely"),
            ap.add_argument("--%ssmooth_max_voxels" % prefix, type=float, default=1.0,
                            help="smoothing: no coordinate moves farther than this many voxels from where the extraction put it")]


def check_arguments(a, prefix=""):
    """The five options of add_options on a parsed namespace -> dict(iterations, lam, mu, boundary, max_voxels), or None when
    iterations is 0 (the other four are then checked all the same); ValueError naming the flags otherwise."""
    get = lambda name: getattr(a, "%ssmooth_%s" % (prefix, name))
    try:
        iterations = check_iterations(get("iterations"), least=0)
        _, lam, mu, boundary, _ = check_options(1, get("lambda"), get("mu"), get("boundary"))
        max_voxels = check_voxels(get("max_voxels"))
    except ValueError as e:
        raise ValueError("--%ssmooth_iterations, --%ssmooth_lambda, --%ssmooth_mu, --%ssmooth_max_voxels: %s" % ((prefix,) * 4 + (e,)))
    if iterations == 0:
        return None
    return dict(iterations=iterations, lam=lam, mu=mu, boundary=boundary, max_voxels=max_voxels)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="input PLY, as mvsnet_amd.mesh writes it")
    ap.add_argument("--out", required=True, help="output PLY")
    ap.add_argument("--iterations", type=int, required=True, help="iterations, 1 .. %d" % MAX_ITERATIONS)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.5, help="the shrinking factor, in (0, 1]")
    ap.add_argument("--mu", type=float, default=-0.53, help="the inflating factor, in [-1, 0] (0: plain Laplacian relaxation)")
    ap.add_argument("--boundary", choices=BOUNDARIES, default="fixed",
                    help="boundary vertices stay, move along the boundary curve, or move freely")
    ap.add_argument("--max_displacement", type=float, default=None, help="no coordinate moves farther than this from its input")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    try:
        a.iterations, a.lam, a.mu, a.boundary, a.max_displacement = check_options(a.iterations, a.lam, a.mu, a.boundary,
                                                                                  a.max_displacement)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.mesh_smooth: --%s" % str(e).replace("lam ", "lambda "))
    return a


def prepare_output(a):
    return refuse_existing("mesh_smooth", a.out, a.force)


def main(argv=None):
    a = parse_args(argv)
    return ply_to_ply("mesh_smooth", a, lambda v, c, f: smooth_mesh(v, c, f, a.iterations, a.lam, a.mu, a.boundary, a.max_displacement))


if __name__ == "__main__":
    sys.exit(main())
