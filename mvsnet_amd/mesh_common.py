"""What the mesh stages share on the host (mesh_clean, mesh_smooth, mesh_simplify, mesh_colour, mesh_sample and mesh.py above
them): one copy of the number checks, the shape check, the way arrays become device tensors and come back, and the plumbing of
the command lines.  Plain functions, as include/geom_common.h is for the kernels.  Every caller keeps its
own range tests and its own error texts; tests/golden/mesh_stage_messages.json holds them to the letter."""
from __future__ import annotations

import json
import os

import numpy as np

MAX_SIZE = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ number checks

def number(name, value, float32=False):
    """-> value as a float, rounded to exactly a float32 if asked; ValueError unless it is a number and not a bool.  The range
    is the caller's to test."""
    try:
        if isinstance(value, bool):
            raise TypeError
        if not float32:
            return float(value)
        with np.errstate(over="ignore"):
            return float(np.float32(value))
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, value))


def integer(value, lo, hi=float("inf")):
    """-> int(value) when it is integral (numpy integers and integral floats included), no bool and in lo .. hi, else None:
    the message is the caller's."""
    try:
        ok = not isinstance(value, bool) and int(value) == value and lo <= int(value) <= hi
    except (TypeError, ValueError, OverflowError):
        ok = False
    return int(value) if ok else None


# ------------------------------------------------------------------------------------------------ arrays in, arrays out

def shapes(vertices, colours, faces):
    """-> (M, F) of vertices (M,3), colours (M,3) or None and faces (F,3), arrays or tensors; ValueError otherwise.  A stage
    with a tighter cap on F adds it after this call."""
    vs, fs = tuple(vertices.shape), tuple(faces.shape)
    if len(vs) != 2 or vs[1] != 3 or len(fs) != 2 or fs[1] != 3:
        raise ValueError("vertices must be (M,3) and faces (F,3), got %s and %s" % (vs, fs))
    if colours is not None and tuple(colours.shape) != vs:
        raise ValueError("colours must be %s like the vertices, got %s" % (vs, tuple(colours.shape)))
    if vs[0] > MAX_SIZE or fs[0] > MAX_SIZE:
        raise ValueError("a mesh of %d vertices and %d faces is beyond the kernels' int32 indices" % (vs[0], fs[0]))
    return vs[0], fs[0]


def _tensor(x, name, dtype, np_dtype, dev):
    import torch
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if x.dtype != dtype:
            raise ValueError("%s must be %s, got %s" % (name, dtype, x.dtype))
        return x.to(dev).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, np_dtype))).to(dev)


def arrays(vertices, colours, faces, shapes=shapes):
    """-> (M, F); ValueError for anything that is not an array or has the wrong shape (`shapes`: the stage's own check where it
    has a cap).  What `inputs` checks, for a stage that has host work of its own between the check and the device."""
    for x in (vertices, faces, colours):
        if x is not None and not hasattr(x, "shape"):
            raise ValueError("vertices, colours and faces must be arrays or tensors")
    return shapes(vertices, colours, faces)


def inputs(vertices, colours, faces, device, what, shapes=shapes):
    """-> (device, vertices, colours or None, faces) as contiguous tensors on the device, after `arrays`, so before any GPU
    work.  With device None a device tensor's own device is taken; `what` names the stage in the error texts of _lib.device."""
    import torch
    from . import _lib
    arrays(vertices, colours, faces, shapes)
    if device is None and isinstance(vertices, torch.Tensor) and vertices.is_cuda:
        device = vertices.device
    dev = _lib.device(device, what)
    return (dev, _tensor(vertices, "vertices", torch.float32, np.float32, dev), _tensor(colours, "colours", torch.uint8, np.uint8, dev),
            _tensor(faces, "faces", torch.int32, np.int32, dev))


def run(vertices, colours, faces, device, what, stage, shapes=shapes):
    """The body of clean_mesh, smooth_mesh, simplify_mesh and colour_mesh: ``stage(dev, v, c, f)`` on the tensors of `inputs`
    -> (vertices, colours or None, faces, report), as tensors on the device when the vertices came as a tensor, else as numpy
    arrays.  Nothing is copied or awaited here that the stage's own read-back has not already waited for."""
    import torch
    dev, v, c, f = inputs(vertices, colours, faces, device, what, shapes)
    out_v, out_c, out_f, report = stage(dev, v, c, f)
    if isinstance(vertices, torch.Tensor):
        return out_v, out_c, out_f, report
    return out_v.cpu().numpy(), None if out_c is None else out_c.cpu().numpy(), out_f.cpu().numpy(), report


# ------------------------------------------------------------------------------------------------ command lines

def refuse_existing(module, out, force):
    """An existing output is refused without --force, before any GPU work -> out."""
    if os.path.exists(out) and not force:
        raise SystemExit("mvsnet_amd.%s: %s exists; pass --force to overwrite it" % (module, out))
    return out


def need_gpu(module):
    from ._lib import gpu_ready
    why = gpu_ready()
    if why is not None:
        raise SystemExit("mvsnet_amd.%s needs a GPU and the HIP library: %s" % (module, why))


def ply_to_ply(module, a, stage):
    """main of a command line that reads the PLY a.mesh, runs ``stage(vertices, colours, faces)`` -> (vertices, colours, faces,
    report), writes the PLY a.out and prints the report with the output's name."""
    out = refuse_existing(module, a.out, a.force)
    need_gpu(module)
    from .mesh import read_mesh_ply, write_mesh_ply
    try:
        vertices, colours, faces, report = stage(*read_mesh_ply(a.mesh))
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        write_mesh_ply(out, vertices, colours, faces)
    except (ValueError, OSError) as e:
        raise SystemExit("mvsnet_amd.%s: %s" % (module, e))
    print(json.dumps(dict(report, out=out)))
    return 0
