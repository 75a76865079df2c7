"""The entry points of csrc/mesh_smooth.hip with ALL of their operands inside one poisoned, guarded arena
(tests/device_arena.py), as tests/test_gpu_arena_mesh_simplify.py does for the vertex clustering: both patterns, a workspace of
exactly the queried size, every call that takes one refused one byte below it with its outputs still holding the pattern, every
intermediate array compared with tests/mesh_smooth_reference.py after its call, and the sort and the scan between the calls
done in torch as smooth_device does them.

What first writes and what reads each piece of the workspace and each array that travels between the calls (written down
before the first run; a poisoned integer used as an index would be an out-of-bounds access, not a failed assertion):
  status    hipMemsetAsync(0) of the 64 words by edges, then atomic adds to words 0 and 1; heads clears words 2 and 3 and rows
            words 4 and 5 by hipMemsetAsync before they add to them.  Read by the test only
  keys      sm_edges_kernel stores all 6 F: faces[] indices are compared with M before vertices[] is read at them | the
            caller's sort
  sorted_keys  the caller's (torch).  heads, entries: read at i - 1, i, i + 1, i + 2 inside 0..E-1; starts: a binary search
            inside 0..E-1.  Its source and target (key >> 31, key & 2^31-1) are compared with M before anything is derived
  head      sm_heads_kernel stores all E | sm_entries_kernel reads all E
  head_rank the caller's scan: entries compares head_rank[i] - 1 with 0..E-1 before it stores neighbours[] there; starts
            copies head_rank[lo - 1], 0 < lo <= E, into row_start without using it as an index
  neighbours  sm_entries_kernel stores entries 0..U-1, the rest keeps the pattern | sm_class_kernel and sm_step_kernel read
            entries a..b-1 only after 0 <= a <= b <= E (N) held for the row bounds; a target is compared with M before X[] is
            read at it
  row_start sm_starts_kernel stores all M + 1 | class, step: v and v + 1, v < M
  vertex_class  sm_class_kernel stores all M | step reads all M; any value but 1 and 2 copies the vertex
  X, V0     inputs of a pass, all M rows read (V0 only with a bound); Y: sm_step_kernel stores all M rows, all row_floats
            floats of each
"""
import os
import re

import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L

from tests import mesh_smooth_reference as R
from tests.device_arena import PATTERNS
from tests.test_gpu_arena_geometry import (E_BADARG, E_SHAPE, E_WORKSPACE, F32, I32, I64, U8, arena, call, n, opt, opt_out, out, put,
                                           refused, run, same_bytes, size)

pytestmark = pytest.mark.gpu
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
MODES = ("fixed", "curve", "free")


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def tput(a, name, t, dtype):
    """What torch computed between two calls, as a read-only input; None when it is empty."""
    return put(a, name, t, dtype) if t.numel() else None


def status(ws):
    return [int(x) for x in n(ws[:24]).view(np.int32)]


def pipeline(a, v, f, boundary, mu, r, row, ws, wsb, tag="", short=True, iterations=2):
    """The four calls on one mesh, every array against the reference after its call -> the last pass's positions as numpy."""
    Mv, Fv, Ev = len(v), len(f), 6 * len(f)
    go = run if short else (lambda a_, name, args, outs: L.check(call(name, args), name))
    adj, ys = R.passes(v, f, iterations, 0.5, mu, boundary, r)
    counts = [adj[k] for k in ("invalid_faces", "non_finite_vertices", "boundary_edges", "non_manifold_edges", "boundary_vertices",
                               "fixed_vertices")]
    tv, tf = opt(a, "vertices" + tag, v, F32), opt(a, "faces" + tag, f, I32)
    # 1. edges
    p = dict(vertices=tv, M=Mv, faces=tf, F=Fv, keys=opt_out(a, "keys" + tag, Ev, dtype=I64), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_smooth_edges_i64", p, [x for x in (p["keys"],) if x is not None])
    a.check()
    assert status(ws) == counts[:2] + [0, 0, 0, 0]
    if Ev:
        same_bytes(n(p["keys"]), adj["keys"], "keys")
        sk = tput(a, "sorted_keys" + tag, torch.sort(p["keys"])[0], I64)
        same_bytes(n(sk), adj["sorted_keys"], "sorted_keys")
    else:
        sk = None
    # 2. heads
    h = dict(sk=sk, F=Fv, head=opt_out(a, "head" + tag, Ev, dtype=I32), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_smooth_heads_i64", h, [x for x in (h["head"],) if x is not None])
    a.check()
    assert status(ws) == counts[:4] + [0, 0]
    if Ev:
        same_bytes(n(h["head"]), adj["head"], "head")
        a.freeze(h["head"])
        rank = tput(a, "head_rank" + tag, torch.cumsum(h["head"], 0, dtype=I32), I32)
        assert int(rank[-1]) == adj["U"]
    else:
        rank = None
    # 3. rows
    U = adj["U"]
    w = dict(sk=sk, head=h["head"], rank=rank, M=Mv, F=Fv, boundary=MODES.index(boundary), nb=opt_out(a, "neighbours" + tag, Ev, dtype=I32),
             rs=out(a, "row_start" + tag, Mv + 1, dtype=I32), vc=opt_out(a, "vertex_class" + tag, Mv, dtype=U8), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_smooth_rows_i32", w, [x for x in (w["nb"], w["rs"], w["vc"]) if x is not None])
    a.check()
    assert status(ws) == counts
    same_bytes(n(w["rs"]), adj["row_start"], "row_start")
    a.freeze(w["rs"])
    if Ev:
        same_bytes(n(w["nb"][:U]), adj["neighbours"], "neighbours")
        assert a.is_pattern(w["nb"][U:]), "written beyond the unique edges"
        a.freeze(w["nb"])
    if Mv:
        same_bytes(n(w["vc"]), adj["vertex_class"], "vertex_class")
        a.freeze(w["vc"])
    # 4. the passes
    if not Mv:
        L.check(call("mvs_mesh_smooth_step_f32", dict(X=None, V0=None, rs=w["rs"], nb=None, vc=None, M=0, N=Ev, row=row, f=0.5, r=-1.0,
                                                      Y=None)), "mvs_mesh_smooth_step_f32")
        a.check()
        return None
    if row == 4:
        fourth = np.arange(Mv, dtype=np.float32)[:, None] + 0.5                # the fourth float travels from X to Y
        first = put(a, "padded vertices" + tag, np.concatenate([v, fourth], 1))
    else:
        first = tv
    x, factors = first, [np.float32(0.5)] + ([np.float32(mu)] if np.float32(mu) != 0 else [])
    for k, want in enumerate(ys):
        y = out(a, "Y%d%s" % (k, tag), Mv, row)
        s = dict(X=x, V0=first, rs=w["rs"], nb=w["nb"], vc=w["vc"], M=Mv, N=Ev, row=row, f=float(factors[k % len(factors)]),
                 r=-1.0 if r is None else float(np.float32(r)), Y=y)
        L.check(call("mvs_mesh_smooth_step_f32", s), "mvs_mesh_smooth_step_f32")
        a.check()
        same_bytes(n(y)[:, :3], want, "pass %d" % k)
        if row == 4:
            same_bytes(n(y)[:, 3:], fourth, "the fourth float of pass %d" % k)
        a.freeze(y)
        x = y
    return n(x)[:, :3]


@both_patterns
@pytest.mark.parametrize("row", [3, 4], ids=["rows of 3", "rows of 4"])
@pytest.mark.parametrize("name", R.MESHES)
def test_edges_heads_rows_step(name, row, pattern):
    v, _, f = R.mesh(name)
    a = arena(pattern)
    wsb = size("mvs_mesh_smooth_workspace_bytes", len(v), len(f))
    assert wsb == 256
    ws = a.take_bytes(wsb, name="smooth workspace")
    k = R.MESHES.index(name)
    boundary, mu, r = MODES[k % 3], (-0.53, 0.0)[k % 2], (None, 0.004)[(k // 2) % 2]
    got = pipeline(a, v, f, boundary, mu, r, row, ws, wsb)
    assert (got is None) == (name == "none")
    for other in MODES:                                                        # the classes of the other modes, on the same arrays
        if other != boundary and len(v):
            pipeline(a, v, f, other, -0.53, 0.004, row, ws, wsb, " " + other, short=False, iterations=1)


@both_patterns
def test_two_meshes_through_one_workspace(pattern):
    """A strip, the larger grid and the strip again through one workspace, the last on a side stream: equal bytes, and the
    status words are each call's own to clear."""
    a = arena(pattern)
    (gv, _, gf), (sv, _, sf) = R.mesh("grid"), R.mesh("strip65")
    wsb = size("mvs_mesh_smooth_workspace_bytes", len(gv), len(gf))
    assert size("mvs_mesh_smooth_workspace_bytes", len(sv), len(sf)) <= wsb
    ws = a.take_bytes(wsb, name="smooth workspace")
    first = pipeline(a, sv, sf, "curve", -0.53, None, 3, ws, wsb, " a", short=False)
    pipeline(a, gv, gf, "fixed", -0.53, 0.01, 3, ws, wsb, " b", short=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = pipeline(a, sv, sf, "curve", -0.53, None, 3, ws, wsb, " c", short=False)
    side.synchronize()
    same_bytes(first, again, "strip again")


@both_patterns
def test_refusals_leave_the_outputs_alone(pattern):
    v, _, f = R.mesh("strip63")
    Mv, Fv = len(v), len(f)
    a = arena(pattern)
    tv, tf = put(a, "vertices", v), put(a, "faces", f, I32)
    wsb = size("mvs_mesh_smooth_workspace_bytes", Mv, Fv)
    o = [out(a, "out%d" % k, 8 * Fv, dtype=I64) for k in range(5)] + [a.take_bytes(wsb, name="smooth workspace")]
    most = (2 ** 31 - 1) // 6
    edges = dict(vertices=tv, M=Mv, faces=tf, F=Fv, keys=o[0], ws=o[5], wsb=wsb)
    refused(a, call("mvs_mesh_smooth_edges_i64", edges, M=-1), E_BADARG, o, "edges M -1")
    refused(a, call("mvs_mesh_smooth_edges_i64", edges, faces=None), E_BADARG, o, "edges faces NULL")
    refused(a, call("mvs_mesh_smooth_edges_i64", edges, keys=None), E_BADARG, o, "edges keys NULL")
    refused(a, call("mvs_mesh_smooth_edges_i64", edges, F=most + 1), E_SHAPE, o, "edges 6 F beyond 2^31 - 1")
    refused(a, call("mvs_mesh_smooth_edges_i64", edges, M=2 ** 31), E_SHAPE, o, "edges M 2^31")
    refused(a, call("mvs_mesh_smooth_edges_i64", edges, wsb=wsb - 1), E_WORKSPACE, o, "edges")
    heads = dict(sk=o[0], F=Fv, head=o[1], ws=o[5], wsb=wsb)
    refused(a, call("mvs_mesh_smooth_heads_i64", heads, head=None), E_BADARG, o, "heads head NULL")
    refused(a, call("mvs_mesh_smooth_heads_i64", heads, F=-1), E_BADARG, o, "heads F -1")
    refused(a, call("mvs_mesh_smooth_heads_i64", heads, F=most + 1), E_SHAPE, o, "heads 6 F beyond 2^31 - 1")
    refused(a, call("mvs_mesh_smooth_heads_i64", heads, wsb=wsb - 1), E_WORKSPACE, o, "heads")
    rows = dict(sk=o[0], head=o[1], rank=o[2], M=Mv, F=Fv, boundary=0, nb=o[3], rs=o[4], vc=o[1], ws=o[5], wsb=wsb)
    refused(a, call("mvs_mesh_smooth_rows_i32", rows, rank=None), E_BADARG, o, "rows head_rank NULL")
    refused(a, call("mvs_mesh_smooth_rows_i32", rows, rs=None), E_BADARG, o, "rows row_start NULL")
    refused(a, call("mvs_mesh_smooth_rows_i32", rows, boundary=3), E_BADARG, o, "rows boundary 3")
    refused(a, call("mvs_mesh_smooth_rows_i32", rows, M=2 ** 31), E_SHAPE, o, "rows M 2^31")
    refused(a, call("mvs_mesh_smooth_rows_i32", rows, wsb=wsb - 1), E_WORKSPACE, o, "rows")
    step = dict(X=tv, V0=tv, rs=o[0], nb=o[1], vc=o[2], M=Mv, N=6 * Fv, row=3, f=0.5, r=-1.0, Y=o[3])
    refused(a, call("mvs_mesh_smooth_step_f32", step, Y=tv), E_BADARG, o, "step Y is X")
    refused(a, call("mvs_mesh_smooth_step_f32", step, Y=None), E_BADARG, o, "step Y NULL")
    refused(a, call("mvs_mesh_smooth_step_f32", step, row=5), E_BADARG, o, "step rows of 5")
    refused(a, call("mvs_mesh_smooth_step_f32", step, f=float("nan")), E_BADARG, o, "step factor NaN")
    refused(a, call("mvs_mesh_smooth_step_f32", step, r=float("inf")), E_BADARG, o, "step bound inf")
    refused(a, call("mvs_mesh_smooth_step_f32", step, M=-1), E_BADARG, o, "step M -1")
    refused(a, call("mvs_mesh_smooth_step_f32", step, N=2 ** 31), E_SHAPE, o, "step N 2^31")
    assert size("mvs_mesh_smooth_workspace_bytes", -1, 0) == 0 and size("mvs_mesh_smooth_workspace_bytes", 0, most + 1) == 0
    a.check()


def test_every_mesh_smooth_entry_point_is_called_here():
    """The mvs_mesh_smooth* names of _lib.SIGNATURES (they stand before mvs_fusion_workspace_bytes, outside the range that
    test_gpu_arena_geometry.py pins) against the names this file passes to call() and size()."""
    declared = {name for name in L.SIGNATURES if name.startswith("mvs_mesh_smooth")}
    with open(os.path.abspath(__file__).replace(".pyc", ".py")) as fh:
        called = set(re.findall(r"\"(mvs_[a-z0-9_]+)\"", fh.read()))
    assert declared - called == set(), "no arena case calls %s" % sorted(declared - called)
    assert len(declared) == 5
    names = list(L.SIGNATURES)
    assert all(names.index(name) < names.index("mvs_fusion_workspace_bytes") for name in declared)
