"""Connected components of a triangle mesh on the MI355X and the removal of its small pieces: the stage between the
extraction of a mesh (mvsnet_amd.mesh) and its PLY.

    python -m mvsnet_amd.mesh_clean --mesh IN.ply --out OUT.ply [--min_component_faces N] [--min_component_extent E]
        [--keep_largest K] [--force]

The kernels are csrc/mesh_components.hip (mvs_mesh_components_label_i32, mvs_mesh_components_measure_f32,
mvs_mesh_compact_mark_i32, mvs_mesh_compact_write_f32); torch owns the device memory, the table of components, its one sort
and the two scans between marking and writing.

Semantics (shared by the kernels, tests/mesh_clean_reference.py and the tests).
  * Input: vertices (M,3) float32, colours (M,3) uint8 or None, faces (F,3) int32; M and F are at most 2^31 - 1.
  * Invalid faces.  A face is invalid when it names an index outside 0..M-1 (its vertices are then never dereferenced) or
    when one of its three vertices has a non-finite coordinate.  Invalid faces join nothing, have label -1 and are never
    kept.  A face that repeats an index is valid.
  * Connectivity and labels.  Two vertices are connected when a valid face names both.  The label of a vertex is the
    smallest vertex index of its component; the label of a valid face is the label of its first vertex.  A vertex that no
    valid face names is unreferenced: its own component, with zero faces.
  * Measures, for each component L with faces: n_L is its face count; its box is the per-axis minimum and maximum of the
    coordinates of the vertices its faces name; its size is d2_L = (ex ex + ey ey) + ez ez in float32 with e = max - min per
    axis, every operation rounded on its own (no contraction).  -0.0 and +0.0 in a box compare equal.
  * Selection.  A component with faces passes when n_L >= min_faces and d2_L >= float32(min_extent) float32(min_extent).
    With keep_largest = k > 0 the passing components are ranked by n_L descending, then label ascending, and only the first
    k stay.  min_faces = 0, min_extent = 0, keep_largest = 0 keeps every component with faces.
  * Output.  The kept faces in input order; the vertices that a kept face names in input order, with their colours; faces
    re-indexed to match.  Unreferenced vertices, the vertices of dropped components and invalid faces are always removed.
  * Report: components (with faces), components_kept, faces_in, faces_out, vertices_in, vertices_out, unreferenced,
    invalid_faces, error_word (the kernels' error word, 0 in every report that is returned: anything else raises) and
    largest: the 16 largest components, ranked as for keep_largest, as [label, faces, extent = sqrt(d2) in float64].
"""
from __future__ import annotations

import argparse
import math
import sys

import numpy as np

from .mesh_common import inputs, integer, ply_to_ply, refuse_existing, run

WHAT = "mesh cleaning"
LARGEST = 16
OPTION_NAMES = ("min_faces", "min_extent", "keep_largest")


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def check_options(min_faces=0, min_extent=0.0, keep_largest=0):
    """-> (min_faces, min_extent, keep_largest) as the selection takes them; ValueError otherwise."""
    out = []
    for name, value in (("min_faces", min_faces), ("keep_largest", keep_largest)):
        out.append(integer(value, 0))
        if out[-1] is None:
            raise ValueError("%s must be an integer >= 0, got %r" % (name, value))
    try:
        e = float(min_extent)
    except (TypeError, ValueError):
        raise ValueError("min_extent must be a number, got %r" % (min_extent,))
    if isinstance(min_extent, bool) or not (e >= 0 and math.isfinite(e)):
        raise ValueError("min_extent must be finite and >= 0, got %r" % (min_extent,))
    return out[0], e, out[1]


def wanted(min_faces=0, min_extent=0.0, keep_largest=0):
    """Whether the options ask for anything: all three at 0 mean that the cleaning does not run at all."""
    return bool(min_faces or min_extent or keep_largest)


# ------------------------------------------------------------------------------------------------ device side

class _Components:
    """Labels and measures of one mesh on the device: the two library calls and the table of the components with faces.
    ``table`` synchronises (it sizes the table)."""

    def __init__(self, vertices, faces, dev):
        import torch
        from . import _lib
        lib = _lib.load()
        self.dev, self.M, self.F = dev, int(vertices.shape[0]), int(faces.shape[0])
        M, F = self.M, self.F
        wsb = lib.mvs_mesh_components_workspace_bytes(M, F)
        self.ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        self.vertex_labels = torch.empty(M, dtype=torch.int32, device=dev)
        self.face_labels = torch.empty(F, dtype=torch.int32, device=dev)
        self.counts = torch.empty(M, dtype=torch.int32, device=dev)
        self.boxes = torch.empty((M, 6), dtype=torch.int32, device=dev)        # the kernel's uint32 words (mesh.py does the same)
        self.vertices, self.faces = vertices, faces
        self.label()
        self.measure()

    def label(self):
        from . import _lib
        rc = _lib.load().mvs_mesh_components_label_i32(
            _lib.ptr(self.vertices), self.M, _lib.ptr(self.faces), self.F, _lib.ptr(self.vertex_labels), _lib.ptr(self.face_labels),
            _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "mvs_mesh_components_label_i32")

    def measure(self):
        from . import _lib
        rc = _lib.load().mvs_mesh_components_measure_f32(
            _lib.ptr(self.vertices), self.M, self.F, _lib.ptr(self.vertex_labels), _lib.ptr(self.face_labels), _lib.ptr(self.counts),
            _lib.ptr(self.boxes), _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr())
        _lib.check(rc, "mvs_mesh_components_measure_f32")

    def status(self):
        """The first three status words as a device tensor: error, invalid faces, unreferenced vertices."""
        import torch
        return self.ws[:12].view(torch.int32)

    def table(self):
        """-> (labels (K,) int64 ascending, n (K,) int64, lo (K,3), hi (K,3) float32, d2 (K,) float32), on the device."""
        import torch
        labels = torch.nonzero(self.counts > 0).flatten()                      # synchronises: K sizes the table
        n = self.counts[labels].to(torch.int64)
        u = self.boxes[labels]
        box = torch.where(u < 0, u ^ (-2 ** 31), ~u).view(torch.float32)       # ordered unsigned image -> the float's bits
        lo, hi = box[:, :3].contiguous(), box[:, 3:].contiguous()
        e = hi - lo
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]       # one rounded operation per torch call
        return labels, n, lo, hi, d2


def _raise_on_error(word):
    from . import _lib
    if word != 0:
        raise _lib.MvsnetHipError("mesh components: a lane ran past the cap on walk steps and retries (error word %d); "
                                  "the labels are void" % word)


def _rank_key(labels, n):
    """int64 keys that sort by face count descending, then label ascending."""
    return ((2 ** 31 - n) << 32) | labels


def mesh_components(vertices, faces, device=None):
    """-> dict(face_labels (F,) int32, labels (K,) int32 ascending, faces (K,) int32, lo (K,3), hi (K,3) float32, unreferenced,
    invalid, error_word) as numpy and ints, for the K components with faces."""
    import torch
    dev, v, _, f = inputs(vertices, None, faces, device, WHAT)
    with torch.cuda.device(dev):
        comp = _Components(v, f, dev)
        labels, n, lo, hi, _ = comp.table()
        error, invalid, unreferenced = (int(x) for x in comp.status().cpu().numpy())
        _raise_on_error(error)
        return dict(face_labels=comp.face_labels.cpu().numpy(), labels=labels.to(torch.int32).cpu().numpy(),
                    faces=n.to(torch.int32).cpu().numpy(), lo=lo.cpu().numpy(), hi=hi.cpu().numpy(), unreferenced=unreferenced,
                    invalid=invalid, error_word=error)


def clean_device(vertices, colours, faces, dev, min_faces=0, min_extent=0.0, keep_largest=0):
    """clean_mesh on contiguous device tensors -> (vertices, colours or None, faces, report), tensors on the device."""
    import torch
    from . import _lib
    min_faces, min_extent, keep_largest = check_options(min_faces, min_extent, keep_largest)
    lib = _lib.load()
    with torch.cuda.device(dev):
        comp = _Components(vertices, faces, dev)
        M, F = comp.M, comp.F
        labels, n, lo, hi, d2 = comp.table()
        K = int(labels.numel())
        # selection on the table: element-wise, and one stable sort of an int64 key for keep_largest
        thr = float(np.float32(min_extent) * np.float32(min_extent))
        keep = (n >= min_faces) & (d2 >= thr)
        key = _rank_key(labels, n)
        if keep_largest > 0 and K:
            order = torch.sort(torch.where(keep, key, torch.full_like(key, 2 ** 63 - 1)), stable=True)[1][:keep_largest]
            first = torch.zeros_like(keep)
            first[order] = True
            keep = keep & first
        keep_label = torch.zeros(M, dtype=torch.int32, device=dev)
        keep_label[labels[keep]] = 1
        face_keep = torch.empty(F, dtype=torch.int32, device=dev)
        vertex_keep = torch.empty(M, dtype=torch.int32, device=dev)
        rc = lib.mvs_mesh_compact_mark_i32(_lib.ptr(faces), M, F, _lib.ptr(comp.face_labels), _lib.ptr(keep_label), _lib.ptr(face_keep),
                                           _lib.ptr(vertex_keep), _lib.stream_ptr())
        _lib.check(rc, "mvs_mesh_compact_mark_i32")
        face_rank = torch.cumsum(face_keep, 0, dtype=torch.int32)
        vertex_rank = torch.cumsum(vertex_keep, 0, dtype=torch.int32)
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        top = torch.sort(key)[1][:LARGEST]
        sizes = torch.cat([comp.status(), face_rank[-1:] if F else zero, vertex_rank[-1:] if M else zero,
                           keep.sum(dtype=torch.int32).reshape(1)]).cpu().numpy()   # the one read-back that sizes the outputs
        error, invalid, unreferenced, F_out, M_out, kept = (int(x) for x in sizes)
        _raise_on_error(error)
        out_v = torch.empty((M_out, 3), dtype=torch.float32, device=dev)
        out_c = None if colours is None else torch.empty((M_out, 3), dtype=torch.uint8, device=dev)
        out_f = torch.empty((F_out, 3), dtype=torch.int32, device=dev)
        rc = lib.mvs_mesh_compact_write_f32(
            _lib.ptr(vertices), _lib.ptr(colours), M, _lib.ptr(faces), F, _lib.ptr(face_keep), _lib.ptr(face_rank), _lib.ptr(vertex_keep),
            _lib.ptr(vertex_rank), M_out, F_out, _lib.ptr(out_v), _lib.ptr(out_c), _lib.ptr(out_f), _lib.stream_ptr())
        _lib.check(rc, "mvs_mesh_compact_write_f32")
        largest = [[int(a), int(b), float(math.sqrt(float(c)))] for a, b, c in
                   zip(labels[top].cpu().numpy(), n[top].cpu().numpy(), d2[top].cpu().numpy())]
        report = {"components": K, "components_kept": kept, "faces_in": F, "faces_out": F_out, "vertices_in": M, "vertices_out": M_out,
                  "unreferenced": unreferenced, "invalid_faces": invalid, "error_word": error, "largest": largest}
        return out_v, out_c, out_f, report


def clean_mesh(vertices, colours, faces, *, min_faces=0, min_extent=0.0, keep_largest=0, device=None):
    """-> (vertices (M',3) float32, colours (M',3) uint8 or None, faces (F',3) int32, report): numpy arrays, or tensors on the
    device when the vertices came as a tensor."""
    options = check_options(min_faces, min_extent, keep_largest)               # before any GPU work
    return run(vertices, colours, faces, device, WHAT, lambda dev, v, c, f: clean_device(v, c, f, dev, *options))


# ------------------------------------------------------------------------------------------------ command line

def add_options(ap, prefix=""):
    """The three selection options, as mesh.py and depthfusion.py also take them (there under a prefix) -> their actions."""
    return [ap.add_argument("--%smin_component_faces" % prefix, type=int, default=0, help="drop mesh components with fewer faces"),
            ap.add_argument("--%smin_component_extent" % prefix, type=float, default=0.0,
                            help="drop mesh components whose bounding-box diagonal is shorter, in world units"),
            ap.add_argument("--%skeep_largest" % prefix, type=int, default=0, help="keep only this many of the largest components (0: all)")]


def check_arguments(a, prefix=""):
    """The three options of add_options on a parsed namespace -> dict(min_faces, min_extent, keep_largest), or None when all
    three are 0 and nothing of the cleaning runs; ValueError naming the flags otherwise."""
    try:
        options = check_options(*(getattr(a, prefix + name) for name in ("min_component_faces", "min_component_extent", "keep_largest")))
    except ValueError as e:
        raise ValueError("--%smin_component_faces and --%skeep_largest must be integers >= 0, --%smin_component_extent finite "
                         "and >= 0 (%s)" % ((prefix,) * 3 + (e,)))
    return dict(zip(OPTION_NAMES, options)) if wanted(*options) else None


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="input PLY, as mvsnet_amd.mesh writes it")
    ap.add_argument("--out", required=True, help="output PLY")
    add_options(ap)
    ap.add_argument("--force", action="store_true", help="overwrite an existing output file")
    return ap


def parse_args(argv=None):
    a = build_parser().parse_args(argv)
    try:
        a.min_component_faces, a.min_component_extent, a.keep_largest = check_options(a.min_component_faces, a.min_component_extent,
                                                                                      a.keep_largest)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.mesh_clean: %s" % str(e).replace("min_faces", "--min_component_faces")
                         .replace("min_extent", "--min_component_extent").replace("keep_largest", "--keep_largest"))
    return a


def prepare_output(a):
    return refuse_existing("mesh_clean", a.out, a.force)


def main(argv=None):
    a = parse_args(argv)
    return ply_to_ply("mesh_clean", a, lambda v, c, f: clean_mesh(v, c, f, min_faces=a.min_component_faces,
                                                                  min_extent=a.min_component_extent, keep_largest=a.keep_largest))


if __name__ == "__main__":
    sys.exit(main())
