"""The entry points of csrc/mesh_colour.hip with ALL of their operands inside one poisoned, guarded arena
(tests/device_arena.py), as tests/test_gpu_arena_mesh_smooth.py does for the smoothing: both patterns, a workspace of exactly the
queried size, every call that takes one refused one byte below it with its outputs still holding the pattern, every BADARG and
SHAPE case, every intermediate array compared with tests/mesh_colour_reference.py after its call, the sort between the first two
calls done in torch as colour_device does it, and the depth maps drawn by mvs_raster_mesh_f32 inside the same arena.

What first writes and what reads each piece of the workspace and each array that travels between the calls (written down
before the first run; a poisoned integer used as an index would be an out-of-bounds access, not a failed assertion):
  status    hipMemsetAsync(0) of the 64 words by keys, then atomic adds to word 0; normals clears word 1 and finish word 2 by
            hipMemsetAsync before they add to them.  Read by the test only
  keys      mc_keys_kernel stores all 3 F: faces[] indices are compared with M before vertices[] is read at them | the
            caller's sort
  sorted_keys  the caller's (torch).  normals: two binary searches inside 0..3F-1, then the run first..last-1 between them;
            the face of a key (key & 2^31-1) is compared with F before faces[] is read at it, and the three indices read
            there are compared with M before vertices[] is read at them
  normals   mc_normals_kernel stores all M rows | mc_accumulate_kernel reads all M rows; never an index
  depth     mvs_raster_mesh_f32 stores all V H W | accumulate reads depth[v, py, px] only after px, py were compared with
            [0, W-1] x [0, H-1] in float32; a value that is not > 0 ends the view for the vertex
  proj, centres  the caller's tables, read at [12 v], [3 v], v < V, through the scalar unit
  images    the caller's: read at four taps clamped to the image after the pixel test above held; byte offsets in 64 bits
  acc, seen the caller zeroes them (here: torch, on the arena's regions); accumulate reads and writes row j of the lane's own
            vertex, j < M, and only where a view saw it | finish reads all M rows
  colours out  mc_finish_kernel stores all M rows; the input colours are read at row j only where they are not NULL
"""
import os
import re

import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L

from tests import mesh_colour_reference as R
from tests import raster_reference as RR
from tests import render_reference as RN
from tests.device_arena import PATTERNS
from tests.test_gpu_arena_geometry import (E_BADARG, E_SHAPE, E_WORKSPACE, F32, F64, I32, I64, U8, arena, call, n, opt, opt_out, out, put,
                                           raster_setup, refused, run, same_bytes, size)

pytestmark = pytest.mark.gpu
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
ARENA_SCENES = ("one", "five", "mixed")
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def status(ws):
    return [int(x) for x in n(ws[:12]).view(np.int32)]


def accumulate_args(a, tv, tn, Mv, cams, images, depth, acc, seen, tag, options=None):
    o = dict(R.DEFAULTS, **(options or {}))
    V, H, W = len(cams), images[0].shape[0], images[0].shape[1]
    return dict(vertices=tv, normals=tn, M=Mv, proj=put(a, "proj" + tag, RN.projection_tables(cams)),
                centres=put(a, "centres" + tag, R.camera_centres(cams)), V=V, H=H, W=W, depth=depth,
                images=put(a, "images" + tag, np.stack(images), U8), md=float(np.float32(o["min_depth"])),
                ratio=float(R.occlusion_ratio(o["occlusion_rel"])), min_cos=float(np.float32(o["min_cos"])), power=o["angle_power"],
                acc=acc, seen=seen)


def pipeline(a, v, c, f, s, ws, wsb, tag="", short=True, colours=True):
    """The calls on one mesh and one scene, every array against the reference after its call -> the final colours as numpy."""
    Mv, Fv, Ev = len(v), len(f), 3 * len(f)
    go = run if short else (lambda a_, name, args, outs: L.check(call(name, args), name))
    nrm, info = R.normals(v, f)
    tv, tf = opt(a, "vertices" + tag, v, F32), opt(a, "faces" + tag, f, I32)
    # 1. keys
    p = dict(vertices=tv, M=Mv, faces=tf, F=Fv, keys=opt_out(a, "keys" + tag, Ev, dtype=I64), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_normals_keys_i64", p, [x for x in (p["keys"],) if x is not None])
    a.check()
    assert status(ws) == [info["invalid_faces"], 0, 0]
    sk = None
    if Ev:
        same_bytes(n(p["keys"]), info["keys"], "keys")
        sk = put(a, "sorted_keys" + tag, torch.sort(p["keys"])[0], I64)
        same_bytes(n(sk), info["sorted_keys"], "sorted_keys")
    # 2. normals
    q = dict(vertices=tv, M=Mv, faces=tf, F=Fv, sk=sk, normals=opt_out(a, "normals" + tag, Mv, 3, dtype=F32), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_normals_f32", q, [x for x in (q["normals"],) if x is not None])
    a.check()
    assert status(ws) == [info["invalid_faces"], info["zero_normals"], 0]
    if Mv:
        same_bytes(n(q["normals"]), nrm, "normals")
        a.freeze(q["normals"])
    # 3. the views, a group of one size at a time, each drawn by the rasteriser first
    acc, seen = opt_out(a, "acc" + tag, Mv, 4, dtype=F64), opt_out(a, "seen" + tag, Mv, dtype=I32)
    want_acc, want_seen = np.zeros((Mv, 4), np.float64), np.zeros(Mv, np.int32)
    if Mv:
        acc.zero_()                                                            # the caller zeroes both before the first call
        seen.zero_()
    for g, ((H, W), members) in enumerate(R.size_groups(s["images"])):
        cams, images = s["cams"][members], [s["images"][k] for k in members]
        gt = "%s g%d" % (tag, g)
        if Mv and Fv:
            r, _ = raster_setup(a, v, f, cams, H, W, 256, 16, index=False, tag=gt)
            r.update(vertices=tv, faces=tf)                                    # the mesh's own regions
            L.check(call("mvs_raster_mesh_f32", r), "mvs_raster_mesh_f32")
            depth = r["depth"]
            want_depth = RR.render(v, f, cams, H, W)[0]
            same_bytes(n(depth), want_depth, "depth")
            a.freeze(depth)
            R.accumulate(v, nrm, cams, images, want_depth, want_acc, want_seen)
        else:
            depth = out(a, "depth" + gt, len(cams), H, W)                      # never read: no vertex, or no normal that is not zero
            a.freeze(depth)
        L.check(call("mvs_mesh_colour_accumulate_f32", accumulate_args(a, tv, q["normals"], Mv, cams, images, depth, acc, seen, gt)),
                "mvs_mesh_colour_accumulate_f32")
        a.check()
        if Mv:
            same_bytes(n(acc), want_acc, "acc after group %d" % g)
            same_bytes(n(seen), want_seen, "seen after group %d" % g)
    # 4. finish
    tc = opt(a, "colours" + tag, c, U8) if colours else None
    z = dict(colours=tc, acc=acc, seen=seen, M=Mv, out=opt_out(a, "colours out" + tag, Mv, 3, dtype=U8), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_colour_finish_u8", z, [x for x in (z["out"],) if x is not None])
    a.check()
    want, unseen = R.finish(c if colours else None, want_acc, want_seen)
    assert status(ws) == [info["invalid_faces"], info["zero_normals"], unseen]
    if not Mv:
        return None
    same_bytes(n(z["out"]), want, "colours")
    return n(z["out"])


@both_patterns
@pytest.mark.parametrize("name", R.MESHES)
def test_keys_normals_accumulate_finish(name, pattern):
    v, c, f = R.mesh(name)
    k = R.MESHES.index(name)
    s = R.scene(ARENA_SCENES[k % 3])
    a = arena(pattern)
    wsb = size("mvs_mesh_colour_workspace_bytes", len(v), len(f))
    assert wsb == 256
    ws = a.take_bytes(wsb, name="colour workspace")
    got = pipeline(a, v, c, f, s, ws, wsb, colours=k % 2 == 0)
    assert (got is None) == (name == "none")
    if got is not None:
        same_bytes(got, R.case(name, ARENA_SCENES[k % 3], k % 2 == 0)[1], "the whole against the case table")


@both_patterns
def test_two_meshes_through_one_workspace(pattern):
    """A strip, the larger grid and the strip again through one workspace, the last on a side stream: equal bytes, and the
    status words are each call's own to clear."""
    a = arena(pattern)
    (gv, gc, gf), (sv, sc, sf) = R.mesh("grid"), R.mesh("strip65")
    wsb = size("mvs_mesh_colour_workspace_bytes", len(gv), len(gf))
    ws = a.take_bytes(wsb, name="colour workspace")
    first = pipeline(a, sv, sc, sf, R.scene("three"), ws, wsb, " a", short=False)
    pipeline(a, gv, gc, gf, R.scene("nine"), ws, wsb, " b", short=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = pipeline(a, sv, sc, sf, R.scene("three"), ws, wsb, " c", short=False)
    side.synchronize()
    same_bytes(first, again, "strip again")


@both_patterns
def test_refusals_leave_the_outputs_alone(pattern):
    v, c, f = R.mesh("strip63")
    s = R.scene("three")
    Mv, Fv = len(v), len(f)
    H, W = s["images"][0].shape[:2]
    a = arena(pattern)
    tv, tf, tc = put(a, "vertices", v), put(a, "faces", f, I32), put(a, "colours", c, U8)
    wsb = size("mvs_mesh_colour_workspace_bytes", Mv, Fv)
    o = [out(a, "out%d" % k, 8 * Mv, dtype=I64) for k in range(4)] + [a.take_bytes(wsb, name="colour workspace")]
    most = (2 ** 31 - 1) // 3
    keys = dict(vertices=tv, M=Mv, faces=tf, F=Fv, keys=o[0], ws=o[4], wsb=wsb)
    refused(a, call("mvs_mesh_normals_keys_i64", keys, M=-1), E_BADARG, o, "keys M -1")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, F=-1), E_BADARG, o, "keys F -1")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, vertices=None), E_BADARG, o, "keys vertices NULL")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, faces=None), E_BADARG, o, "keys faces NULL")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, keys=None), E_BADARG, o, "keys keys NULL")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, keys=tf), E_BADARG, o, "keys keys is faces")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, ws=None), E_BADARG, o, "keys workspace NULL")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, F=most + 1), E_SHAPE, o, "keys 3 F beyond 2^31 - 1")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, M=2 ** 31), E_SHAPE, o, "keys M 2^31")
    refused(a, call("mvs_mesh_normals_keys_i64", keys, wsb=wsb - 1), E_WORKSPACE, o, "keys")
    nrm = dict(vertices=tv, M=Mv, faces=tf, F=Fv, sk=o[0], normals=o[1], ws=o[4], wsb=wsb)
    refused(a, call("mvs_mesh_normals_f32", nrm, normals=None), E_BADARG, o, "normals normals NULL")
    refused(a, call("mvs_mesh_normals_f32", nrm, sk=None), E_BADARG, o, "normals sorted_keys NULL")
    refused(a, call("mvs_mesh_normals_f32", nrm, normals=tv), E_BADARG, o, "normals normals is vertices")
    refused(a, call("mvs_mesh_normals_f32", nrm, F=-1), E_BADARG, o, "normals F -1")
    refused(a, call("mvs_mesh_normals_f32", nrm, M=2 ** 31), E_SHAPE, o, "normals M 2^31")
    refused(a, call("mvs_mesh_normals_f32", nrm, F=most + 1), E_SHAPE, o, "normals 3 F beyond 2^31 - 1")
    refused(a, call("mvs_mesh_normals_f32", nrm, wsb=wsb - 1), E_WORKSPACE, o, "normals")
    depth = put(a, "depth", np.ones((3, H, W), np.float32))
    acc = accumulate_args(a, tv, tv, Mv, s["cams"], s["images"], depth, o[2], o[3], "")
    for bad, what in ((dict(power=9), "power 9"), (dict(power=-1), "power -1"), (dict(min_cos=NAN), "min_cos NaN"), (dict(min_cos=1.5), "min_cos 1.5"),
                      (dict(ratio=0.0), "ratio 0"), (dict(ratio=NAN), "ratio NaN"), (dict(ratio=float("inf")), "ratio inf"),
                      (dict(md=-1.0), "min_depth -1"), (dict(md=NAN), "min_depth NaN"), (dict(M=-1), "M -1"), (dict(V=-1), "V -1"),
                      (dict(H=0), "H 0"), (dict(W=-2), "W -2"), (dict(acc=None), "acc NULL"), (dict(seen=None), "seen NULL"),
                      (dict(normals=None), "normals NULL"), (dict(proj=None), "proj NULL"), (dict(centres=None), "centres NULL"),
                      (dict(depth=None), "depth NULL"), (dict(images=None), "images NULL"), (dict(acc=tv), "acc is vertices"),
                      (dict(seen=depth), "seen is depth"), (dict(seen=o[2]), "seen is acc")):
        refused(a, call("mvs_mesh_colour_accumulate_f32", acc, **bad), E_BADARG, o, "accumulate " + what)
    refused(a, call("mvs_mesh_colour_accumulate_f32", acc, M=2 ** 31), E_SHAPE, o, "accumulate M 2^31")
    refused(a, call("mvs_mesh_colour_accumulate_f32", acc, H=(1 << 20) + 1), E_SHAPE, o, "accumulate H 2^20 + 1")
    refused(a, call("mvs_mesh_colour_accumulate_f32", acc, W=(1 << 20) + 1), E_SHAPE, o, "accumulate W 2^20 + 1")
    refused(a, call("mvs_mesh_colour_accumulate_f32", acc, V=1 << 12, H=1 << 10, W=1 << 10), E_SHAPE, o, "accumulate 2^32 pixels")
    fin = dict(colours=tc, acc=o[0], seen=o[1], M=Mv, out=o[2], ws=o[4], wsb=wsb)
    refused(a, call("mvs_mesh_colour_finish_u8", fin, out=None), E_BADARG, o, "finish out NULL")
    refused(a, call("mvs_mesh_colour_finish_u8", fin, acc=None), E_BADARG, o, "finish acc NULL")
    refused(a, call("mvs_mesh_colour_finish_u8", fin, seen=None), E_BADARG, o, "finish seen NULL")
    refused(a, call("mvs_mesh_colour_finish_u8", fin, out=tc), E_BADARG, o, "finish out is colours")
    refused(a, call("mvs_mesh_colour_finish_u8", fin, out=o[0]), E_BADARG, o, "finish out is acc")
    refused(a, call("mvs_mesh_colour_finish_u8", fin, M=-1), E_BADARG, o, "finish M -1")
    refused(a, call("mvs_mesh_colour_finish_u8", fin, M=2 ** 31), E_SHAPE, o, "finish M 2^31")
    refused(a, call("mvs_mesh_colour_finish_u8", fin, wsb=wsb - 1), E_WORKSPACE, o, "finish")
    assert size("mvs_mesh_colour_workspace_bytes", -1, 0) == 0 and size("mvs_mesh_colour_workspace_bytes", 0, most + 1) == 0
    assert size("mvs_mesh_colour_workspace_bytes", 2 ** 31 - 1, most) == 256
    a.check()


def test_every_mesh_colour_entry_point_is_called_here():
    """The mvs_mesh_colour* and mvs_mesh_normals* names of _lib.SIGNATURES (they stand before mvs_fusion_workspace_bytes, outside
    the range that test_gpu_arena_geometry.py pins) against the names this file passes to call() and size()."""
    declared = {name for name in L.SIGNATURES if name.startswith("mvs_mesh_colour") or name.startswith("mvs_mesh_normals")}
    with open(os.path.abspath(__file__).replace(".pyc", ".py")) as fh:
        called = set(re.findall(r"\"(mvs_[a-z0-9_]+)\"", fh.read()))
    assert declared - called == set(), "no arena case calls %s" % sorted(declared - called)
    assert len(declared) == 5
    names = list(L.SIGNATURES)
    assert all(names.index(name) < names.index("mvs_fusion_workspace_bytes") for name in declared)
