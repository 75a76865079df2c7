"""The entry points of csrc/mesh_sample.hip with ALL of their operands inside one poisoned, guarded arena
(tests/device_arena.py), as tests/test_gpu_arena_mesh_simplify.py does for the clustering: both patterns, the workspace of
exactly the queried size, the quota call refused one byte below it with its outputs still holding the pattern, both calls
compared with tests/mesh_sample_reference.py, and the scan between them done in torch as sample_device does it.

What first writes and what reads each piece (written down before the first run; a poisoned integer used as an index would be
an out-of-bounds access, not a failed assertion):
  status    hipMemsetAsync(0) of the 64 words by quota, then one atomic add per workgroup to words 0, 1 and 2.  Read by the
            test (sample_device reads words 0..2) only; the write call has no workspace
  quota     msa_quota_kernel stores all F | the caller's scan
  sums      the caller's (torch.cumsum): msa_write_kernel reads sums[p] only at 0 <= p < F (every bisection keeps lo <= mid < hi
            <= F and ends after 32 steps); a value is only ever compared with a sample index or clamped into 0..2^31-1 for LDS
  faces     quota and write read face f < F; the three indices are checked against M before a vertex or a colour is read
  out_xyz, out_face, out_colours, out_normals  msa_write_kernel stores the rows g < N, all of them; rows from N on keep the
            pattern.  With N = 0 nothing is launched
"""
import os
import re

import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L

from tests import mesh_clean_reference as MC
from tests import mesh_sample_reference as R
from tests.device_arena import PATTERNS
from tests.test_gpu_arena_geometry import (E_BADARG, E_SHAPE, E_WORKSPACE, F32, I32, I64, U8, arena, call, frozen, n, opt, opt_out, out, put,
                                           refused, run, same_bytes, size)

pytestmark = pytest.mark.gpu
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
SPARE = 5                                                                      # output rows beyond N: they keep the pattern


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def case(name):
    """grid: a 12 x 12 grid of quads with invalid faces, non-finite vertices and a face without area; strip63 / 64 / 65: one strip
    of as many faces; gaps: 255 faces of one sample, 900 without area, 300 of one sample (a run beyond the LDS cap); lone: six
    vertices and no face; none: nothing.  -> (vertices, colours, faces, density)."""
    rs = np.random.RandomState(8)
    if name == "grid":
        v, f = (x.copy() for x in MC.grid(12))
        f[5], f[17], f[40], f[99], f[100] = [-1, 0, 1], [0, 1, len(v)], [3, 2 ** 31 - 1, 4], [-2 ** 31, 7, 8], [9, 9, 10]
        v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
        density = 300.0
    elif name.startswith("strip"):
        v, f = MC.strip(int(name[5:]), 1)
        density = 9.0
    elif name == "gaps":
        t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
        v = np.concatenate([t, t + np.float32(1)])
        f, density = np.array([[0, 1, 2]] * 255 + [[0, 0, 1]] * 900 + [[3, 4, 5]] * 300, np.int32), 2.0
    elif name == "lone":
        v, f, density = rs.rand(6, 3).astype(np.float32), np.zeros((0, 3), np.int32), 4.0
    else:
        v, f, density = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    return frozen(v, c, f) + (density,)


def status(ws):
    return [int(x) for x in n(ws[:12]).view(np.int32)]


def pipeline(a, v, c, f, density, seed, ws, wsb, outputs, tag="", short=True):
    """The two calls and the scan between them on one mesh, both against the reference -> the outputs as numpy."""
    Mv, Fv = len(v), len(f)
    want = R.sample(v, c, f, density, seed)
    q, invalid, zero, saturated = R.quota(v, f, density)
    tv, tf = opt(a, "vertices" + tag, v, F32), opt(a, "faces" + tag, f, I32)
    tc = None if c is None else opt(a, "colours" + tag, c, U8)
    # 1. quota
    p = dict(vertices=tv, M=Mv, faces=tf, F=Fv, density=float(density), quota=opt_out(a, "quota" + tag, Fv, dtype=I64), ws=ws, wsb=wsb)
    if short:
        run(a, "mvs_mesh_sample_quota_f32", p, [x for x in (p["quota"],) if x is not None])
    else:
        L.check(call("mvs_mesh_sample_quota_f32", p), "mvs_mesh_sample_quota_f32")
    a.check()
    assert status(ws) == [int(invalid.sum()), int(zero.sum()), 0]
    sums = None
    if Fv:
        same_bytes(n(p["quota"]), q, "quota")
        a.freeze(p["quota"])
        sums = put(a, "sums" + tag, torch.cumsum(p["quota"], 0, dtype=I64), I64)
        assert int(sums[-1]) >> 16 == want["stats"]["samples"]
    N = want["stats"]["samples"]
    # 2. write
    w = dict(vertices=tv, colours=tc, M=Mv, faces=tf, F=Fv, sums=sums, N=N, seed=int(seed),
             xyz=out(a, "xyz" + tag, N + SPARE, 3, dtype=F32),
             face=out(a, "face" + tag, N + SPARE, dtype=I32) if outputs["face_index"] else None,
             rgb=out(a, "rgb" + tag, N + SPARE, 3, dtype=U8) if tc is not None else None,
             nrm=out(a, "normals" + tag, N + SPARE, 3, dtype=F32) if outputs["normals"] else None)
    L.check(call("mvs_mesh_sample_write_f32", w), "mvs_mesh_sample_write_f32")
    a.check()
    got = {}
    for key, t, ref in (("xyz", w["xyz"], want["xyz"]), ("face_index", w["face"], want["face_index"]), ("colours", w["rgb"], want["colours"]),
                        ("normals", w["nrm"], want["normals"])):
        if t is None:
            continue
        same_bytes(n(t[:N]), ref, key)
        assert a.is_pattern(t[N:]), "%s: written beyond the samples" % key
        got[key] = n(t[:N])
    return got


@both_patterns
@pytest.mark.parametrize("outputs", [dict(colour=False, normals=False, face_index=False), dict(colour=True, normals=True, face_index=True)],
                         ids=["plain", "all outputs"])
@pytest.mark.parametrize("name", ["grid", "strip63", "strip64", "strip65", "gaps", "lone", "none"])
def test_quota_scan_write(name, outputs, pattern):
    v, c, f, density = case(name)
    a = arena(pattern)
    wsb = size("mvs_mesh_sample_workspace_bytes", len(v), len(f))
    assert wsb == 256
    ws = a.take_bytes(wsb, name="sample workspace")
    got = pipeline(a, v, c if outputs["colour"] else None, f, density, 3, ws, wsb, outputs)
    assert (name in ("lone", "none")) == (len(got["xyz"]) == 0) and (name != "grid" or len(got["xyz"]) > 2000)


@both_patterns
def test_two_meshes_through_one_workspace(pattern):
    """A strip, the grid and the strip again through one workspace, the last on a side stream: equal bytes, and the status words
    are each quota call's own to clear."""
    a = arena(pattern, mb=16)
    gv, gc, gf, gd = case("grid")
    sv, sc, sf, sd = case("strip65")
    wsb = size("mvs_mesh_sample_workspace_bytes", len(gv), len(gf))
    ws = a.take_bytes(wsb, name="sample workspace")
    every = dict(colour=True, normals=True, face_index=True)
    first = pipeline(a, sv, sc, sf, sd, 1, ws, wsb, every, " a", short=False)
    pipeline(a, gv, gc, gf, gd, 1, ws, wsb, every, " b", short=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = pipeline(a, sv, sc, sf, sd, 1, ws, wsb, every, " c", short=False)
    side.synchronize()
    assert set(first) == set(again) == {"xyz", "face_index", "colours", "normals"}
    for key in first:
        same_bytes(first[key], again[key], "strip again: " + key)


@both_patterns
def test_refusals_leave_the_outputs_alone(pattern):
    v, c, f, density = case("strip63")
    Mv, Fv = len(v), len(f)
    a = arena(pattern)
    tv, tf, tc = put(a, "vertices", v), put(a, "faces", f, I32), put(a, "colours", c, U8)
    wsb = size("mvs_mesh_sample_workspace_bytes", Mv, Fv)
    o = [out(a, "out%d" % k, 8 * Fv, dtype=I64) for k in range(5)] + [a.take_bytes(wsb, name="sample workspace")]
    quota = dict(vertices=tv, M=Mv, faces=tf, F=Fv, density=density, quota=o[0], ws=o[5], wsb=wsb)
    refused(a, call("mvs_mesh_sample_quota_f32", quota, M=-1), E_BADARG, o, "quota M -1")
    refused(a, call("mvs_mesh_sample_quota_f32", quota, density=0.0), E_BADARG, o, "quota density 0")
    refused(a, call("mvs_mesh_sample_quota_f32", quota, density=float("nan")), E_BADARG, o, "quota density NaN")
    refused(a, call("mvs_mesh_sample_quota_f32", quota, faces=None), E_BADARG, o, "quota faces NULL")
    refused(a, call("mvs_mesh_sample_quota_f32", quota, quota=None), E_BADARG, o, "quota quota NULL")
    refused(a, call("mvs_mesh_sample_quota_f32", quota, F=2 ** 26 + 1), E_SHAPE, o, "quota F beyond 2^26")
    refused(a, call("mvs_mesh_sample_quota_f32", quota, M=2 ** 31), E_SHAPE, o, "quota M 2^31")
    refused(a, call("mvs_mesh_sample_quota_f32", quota, wsb=wsb - 1), E_WORKSPACE, o, "quota")
    write = dict(vertices=tv, colours=None, M=Mv, faces=tf, F=Fv, sums=o[0], N=16, seed=0, xyz=o[1], face=o[2], rgb=None, nrm=o[4])
    refused(a, call("mvs_mesh_sample_write_f32", write, N=-1), E_BADARG, o, "write N -1")
    refused(a, call("mvs_mesh_sample_write_f32", write, N=2 ** 31), E_SHAPE, o, "write N 2^31")
    refused(a, call("mvs_mesh_sample_write_f32", write, sums=None), E_BADARG, o, "write sums NULL")
    refused(a, call("mvs_mesh_sample_write_f32", write, xyz=None), E_BADARG, o, "write xyz NULL")
    refused(a, call("mvs_mesh_sample_write_f32", write, rgb=o[3]), E_BADARG, o, "write colours out without colours in")
    refused(a, call("mvs_mesh_sample_write_f32", write, F=0), E_BADARG, o, "write samples without faces")
    refused(a, call("mvs_mesh_sample_write_f32", write, F=2 ** 26 + 1), E_SHAPE, o, "write F beyond 2^26")
    refused(a, call("mvs_mesh_sample_write_f32", write, colours=tc, rgb=o[3], N=0), 0, o, "write N 0")      # accepted: nothing to do
    assert size("mvs_mesh_sample_workspace_bytes", -1, 0) == 0 and size("mvs_mesh_sample_workspace_bytes", 0, 2 ** 26 + 1) == 0
    a.check()


def test_every_mesh_sample_entry_point_is_called_here():
    """The mvs_mesh_sample* names of _lib.SIGNATURES (they stand before mvs_fusion_workspace_bytes, outside the range that
    test_gpu_arena_geometry.py pins) against the names this file passes to call() and size()."""
    declared = {name for name in L.SIGNATURES if name.startswith("mvs_mesh_sample")}
    with open(os.path.abspath(__file__).replace(".pyc", ".py")) as fh:
        called = set(re.findall(r"\"(mvs_[a-z0-9_]+)\"", fh.read()))
    assert declared - called == set(), "no arena case calls %s" % sorted(declared - called)
    assert len(declared) == 3
    names = list(L.SIGNATURES)
    assert all(names.index(name) < names.index("mvs_fusion_workspace_bytes") for name in declared)
