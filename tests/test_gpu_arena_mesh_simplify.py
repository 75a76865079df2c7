"""The entry points of csrc/mesh_simplify.hip with ALL of their operands inside one poisoned, guarded arena
(tests/device_arena.py), as tests/test_gpu_arena_geometry.py does for the other geometry kernels: both patterns, workspaces of
exactly the queried size, every call refused one byte below it with its outputs still holding the pattern, every step compared
with tests/mesh_simplify_reference.py, and the sorts and scans between the calls done in torch as simplify_device does them.

What first writes and what reads each piece of the workspace and each array that travels between the calls (written down
before the first run; a poisoned integer used as an index would be an out-of-bounds access, not a failed assertion):
  status    hipMemsetAsync(0) of the 64 words by keys, then atomic adds to words 0 and 1; faces clears word 2 and mark word 3 by
            hipMemsetAsync before they add to them.  Read by the test only
  used      hipMemsetAsync(0) of all M by keys, ms_use_kernel stores 1 | ms_drop_kernel reads all M.  No other call reads it
  sums      hipMemsetAsync(0) of all 8 M words by sums, then ms_sums_kernel adds to words 0..6 and stores word 7 of the slots
            that head_rank names (range-checked against M) | ms_finish_kernel reads the slots below head_rank[M - 1]
  keys      ms_cell_kernel stores all M | ms_use_kernel reads keys[] only at indices it checked against M; ms_drop_kernel
  offsets   ms_cell_kernel stores all M x 3 | ms_sums_kernel at order[i], checked against M
  sorted_keys, order, head_rank  the caller's (torch): order and head_rank - 1 are checked against M before they index
  head      ms_heads_kernel stores all M
  vertex_cluster  ms_sums_kernel stores at every order[i] inside 0..M-1: all M for a permutation | ms_faces_kernel at face
            indices it checked against M; its values are checked against M before ms_mark_kernel uses them as indices
  cluster_vertices, cluster_colours  ms_finish_kernel stores rows 0..K-1; rows K..M-1 keep the pattern.  The compaction reads
            rows below K only (it is called with M = K)
  cluster_faces, key_lo, key_hi  ms_faces_kernel stores all F | ms_mark_kernel at order[i], checked against F
  face_keep ms_mark_kernel stores at every order[i]: all F for a permutation;  vertex_keep  hipMemsetAsync(0) of all M by
            mark, then stores of 1 at cluster indices checked against M
"""
import re
import os

import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L

from tests import mesh_clean_reference as MC
from tests import mesh_simplify_reference as R
from tests.device_arena import PATTERNS
from tests.test_gpu_arena_geometry import (E_BADARG, E_SHAPE, E_WORKSPACE, F32, I32, I64, U8, arena, call, frozen, n, opt, opt_out, out, put,
                                           refused, run, same_bytes, size)

pytestmark = pytest.mark.gpu
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
ORIGIN = np.array([-0.13, -0.07, -1.5], np.float32)


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def case(name):
    """grid: a 12 x 12 grid of quads with invalid faces and non-finite vertices; strip63 / 64 / 65: one strip of as many faces;
    lone: six vertices and no face; none: nothing.  -> (vertices, colours, faces, cell)."""
    rs = np.random.RandomState(8)
    if name == "grid":
        v, f = (x.copy() for x in MC.grid(12))
        f[5], f[17], f[40], f[99] = [-1, 0, 1], [0, 1, len(v)], [3, 2 ** 31 - 1, 4], [-2 ** 31, 7, 8]
        v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
        cell = 0.6
    elif name.startswith("strip"):
        v, f = MC.strip(int(name[5:]), 1)
        cell = 1.05
    elif name == "lone":
        v, f, cell = rs.rand(6, 3).astype(np.float32), np.zeros((0, 3), np.int32), 0.25
    else:
        v, f, cell = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    return frozen(v, c, f) + (cell,)


def tput(a, name, t, dtype):
    """What torch computed between two calls, as a read-only input; None when it is empty."""
    return put(a, name, t, dtype) if t.numel() else None


def grid_args(cell):
    return dict(ox=float(ORIGIN[0]), oy=float(ORIGIN[1]), oz=float(ORIGIN[2]), cell=float(np.float32(cell)))


def status(ws, words):
    return [int(x) for x in n(ws[:4 * words]).view(np.int32)]


def pipeline(a, v, c, f, cell, two, ws, wsb, tag="", short=True):
    """The five calls and the compaction on one mesh, every step against the reference -> the outputs as numpy."""
    Mv, Fv = len(v), len(f)
    go = run if short else (lambda a_, name, args, outs: L.check(call(name, args), name))
    ok, _, key, q, _ = R.cells(v, cell, ORIGIN)
    _, valid, used, ukeys, cluster, _ = R._clusters(v, f, np.float32(cell), ORIGIN)
    K = len(ukeys)
    want = R.simplify(v, c, f, cell, ORIGIN)
    tv, tf = opt(a, "vertices" + tag, v, F32), opt(a, "faces" + tag, f, I32)
    tc = None if c is None else opt(a, "colours" + tag, c, U8)
    # 1. keys
    p = dict(vertices=tv, M=Mv, faces=tf, F=Fv, **grid_args(cell), keys=opt_out(a, "keys" + tag, Mv, dtype=I64),
             offsets=opt_out(a, "offsets" + tag, Mv, 3, dtype=I32), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_cluster_keys_f32", p, [x for x in (p["keys"], p["offsets"]) if x is not None])
    a.check()
    assert status(ws, 4) == [int((~valid).sum()), int((~ok).sum()), 0, 0]
    if Mv:
        same_bytes(n(p["keys"]), np.where(used, key, -1), "keys")
        same_bytes(n(p["offsets"]), q.astype(np.int32), "offsets")
        a.freeze(p["keys"])
        a.freeze(p["offsets"])
        sk, order = torch.sort(p["keys"], stable=True)
    else:
        sk = order = torch.zeros(0, dtype=I64, device="cuda")
    sk, order = tput(a, "sorted_keys" + tag, sk, I64), tput(a, "order" + tag, order, I64)
    # 2. heads
    h = dict(sk=sk, M=Mv, head=opt_out(a, "head" + tag, Mv, dtype=I32))
    L.check(call("mvs_mesh_cluster_heads_i64", h), "mvs_mesh_cluster_heads_i64")
    a.check()
    if Mv:
        s = n(sk)
        same_bytes(n(h["head"]), ((s >= 0) & (np.concatenate([[-2], s[:-1]]) != s)).astype(np.int32), "head")
        rank = tput(a, "head_rank" + tag, torch.cumsum(h["head"], 0, dtype=I32), I32)
        assert int(rank[-1]) == K
    else:
        rank = None
    # 3. sums
    s = dict(sk=sk, order=order, rank=rank, offsets=p["offsets"], colours=tc, M=Mv, **grid_args(cell),
             vc=opt_out(a, "vertex_cluster" + tag, Mv, dtype=I32), cv=opt_out(a, "cluster_vertices" + tag, Mv, 3, dtype=F32),
             cc=None if tc is None else opt_out(a, "cluster_colours" + tag, Mv, 3, dtype=U8), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_cluster_sums_f32", s, [x for x in (s["vc"], s["cv"], s["cc"]) if x is not None])
    a.check()
    assert status(ws, 4) == [int((~valid).sum()), int((~ok).sum()), 0, 0]
    if Mv:
        same_bytes(n(s["vc"]), cluster.astype(np.int32), "vertex_cluster")
        same_bytes(n(s["cv"][:K]), R.all_clusters(v, None, f, cell, ORIGIN), "cluster_vertices")
        assert a.is_pattern(s["cv"][K:]) and (tc is None or a.is_pattern(s["cc"][K:])), "written beyond the clusters"
        a.freeze(s["vc"])
    # 4. faces
    fa = dict(faces=tf, M=Mv, F=Fv, vc=s["vc"], cf=opt_out(a, "cluster_faces" + tag, Fv, 3, dtype=I32),
              lo=opt_out(a, "key_lo" + tag, Fv, dtype=I64), hi=opt_out(a, "key_hi" + tag, Fv, dtype=I64) if two else None, ws=ws, wsb=wsb)
    go(a, "mvs_mesh_cluster_faces_i32", fa, [x for x in (fa["cf"], fa["lo"], fa["hi"]) if x is not None])
    a.check()
    if Fv:
        g = np.full((Fv, 3), -1, np.int64)
        g[valid] = cluster[f[valid]]
        same_bytes(n(fa["cf"]), g.astype(np.int32), "cluster_faces")
        live = valid & (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
        t = np.sort(g, 1)
        dead = np.int64(2 ** 63 - 1)
        if two:
            same_bytes(n(fa["hi"]), np.where(live, t[:, 0], dead), "key_hi")
            same_bytes(n(fa["lo"]), np.where(live, (t[:, 1] << 32) | t[:, 2], dead), "key_lo")
            lo1, by_lo = torch.sort(fa["lo"], stable=True)
            shi, by_hi = torch.sort(fa["hi"][by_lo], stable=True)
            slo, forder = lo1[by_hi], by_lo[by_hi]
        else:
            same_bytes(n(fa["lo"]), np.where(live, (t[:, 0] << 42) | (t[:, 1] << 21) | t[:, 2], dead), "key_lo")
            (slo, forder), shi = torch.sort(fa["lo"], stable=True), None
        a.freeze(fa["cf"])
        slo, forder = tput(a, "sorted_lo" + tag, slo, I64), tput(a, "face_order" + tag, forder, I64)
        shi = None if shi is None else tput(a, "sorted_hi" + tag, shi, I64)
    else:
        slo = forder = shi = None
    # 5. mark
    m = dict(cf=fa["cf"], M=Mv, F=Fv, lo=slo, hi=shi, order=forder, fk=opt_out(a, "face_keep" + tag, Fv, dtype=I32),
             vk=opt_out(a, "vertex_keep" + tag, Mv, dtype=I32), ws=ws, wsb=wsb)
    go(a, "mvs_mesh_cluster_mark_i32", m, [x for x in (m["fk"], m["vk"]) if x is not None])
    a.check()
    rep = want[3]
    assert status(ws, 4) == [rep["invalid_faces"], rep["unclusterable_vertices"], rep["degenerate_faces"], rep["duplicate_faces"]]
    Mo, Fo = rep["vertices_out"], rep["faces_out"]
    if Fv:
        assert int(m["fk"].sum()) == Fo and set(np.unique(n(m["fk"]))) <= {0, 1}
    if Mv:
        vk = n(m["vk"])
        assert int(vk.sum()) == Mo and not vk[K:].any() and set(np.unique(vk)) <= {0, 1}
    # 6. the compaction of mesh_components.hip on the clusters
    frank = tput(a, "face_rank" + tag, torch.cumsum(m["fk"], 0, dtype=I32), I32) if Fv else None
    vrank = tput(a, "vertex_rank" + tag, torch.cumsum(m["vk"], 0, dtype=I32), I32) if Mv else None
    wr = dict(vertices=s["cv"], colours=s["cc"], M=K, faces=fa["cf"], F=Fv, face_keep=m["fk"], face_rank=frank, vertex_keep=m["vk"],
              vertex_rank=vrank, M_out=Mo, F_out=Fo, ov=opt_out(a, "out_vertices" + tag, Mo, 3, dtype=F32),
              oc=None if tc is None else opt_out(a, "out_colours" + tag, Mo, 3, dtype=U8), of=opt_out(a, "out_faces" + tag, Fo, 3, dtype=I32))
    L.check(call("mvs_mesh_compact_write_f32", wr), "mvs_mesh_compact_write_f32")
    a.check()
    got = [None if t is None else n(t) for t in (wr["ov"], wr["oc"], wr["of"])]
    for g_, w_, what in zip(got, want[:3], ("vertices", "colours", "faces")):
        if g_ is not None:
            same_bytes(g_, w_, what)
        else:
            assert w_ is None or len(w_) == 0
    return got


@both_patterns
@pytest.mark.parametrize("two", [False, True], ids=["one key", "two keys"])
@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("name", ["grid", "strip63", "strip64", "strip65", "lone", "none"])
def test_keys_heads_sums_faces_mark_write(name, colour, two, pattern):
    v, c, f, cell = case(name)
    a = arena(pattern)
    wsb = size("mvs_mesh_cluster_workspace_bytes", len(v), len(f))
    ws = a.take_bytes(wsb, name="cluster workspace")
    got = pipeline(a, v, c if colour else None, f, cell, two, ws, wsb)
    assert (name in ("lone", "none")) == (got[0] is None) and (name != "grid" or len(got[2]) > 8)


@both_patterns
def test_two_meshes_through_one_workspace(pattern):
    """A strip, the larger grid and the strip again through the grid's workspace, the last on a side stream: equal bytes, and
    the status words and the sums are each call's own to clear."""
    a = arena(pattern, mb=16)
    gv, gc, gf, gcell = case("grid")
    sv, sc, sf, scell = case("strip65")
    wsb = size("mvs_mesh_cluster_workspace_bytes", len(gv), len(gf))
    assert size("mvs_mesh_cluster_workspace_bytes", len(sv), len(sf)) <= wsb
    ws = a.take_bytes(wsb, name="cluster workspace")
    first = pipeline(a, sv, sc, sf, scell, False, ws, wsb, " a", short=False)
    pipeline(a, gv, gc, gf, gcell, False, ws, wsb, " b", short=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = pipeline(a, sv, sc, sf, scell, False, ws, wsb, " c", short=False)
    side.synchronize()
    for x, y in zip(first, again):
        same_bytes(x, y, "strip again")


@both_patterns
def test_refusals_leave_the_outputs_alone(pattern):
    v, c, f, cell = case("strip63")
    Mv, Fv = len(v), len(f)
    a = arena(pattern)
    tv, tf = put(a, "vertices", v), put(a, "faces", f, I32)
    wsb = size("mvs_mesh_cluster_workspace_bytes", Mv, Fv)
    o = [out(a, "out%d" % k, 8 * Mv, dtype=I64) for k in range(6)] + [a.take_bytes(wsb, name="cluster workspace")]
    keys = dict(vertices=tv, M=Mv, faces=tf, F=Fv, **grid_args(cell), keys=o[0], offsets=o[1], ws=o[6], wsb=wsb)
    refused(a, call("mvs_mesh_cluster_keys_f32", keys, M=-1), E_BADARG, o, "keys M -1")
    refused(a, call("mvs_mesh_cluster_keys_f32", keys, cell=0.0), E_BADARG, o, "keys cell 0")
    refused(a, call("mvs_mesh_cluster_keys_f32", keys, oy=float("nan")), E_BADARG, o, "keys origin NaN")
    refused(a, call("mvs_mesh_cluster_keys_f32", keys, faces=None), E_BADARG, o, "keys faces NULL")
    refused(a, call("mvs_mesh_cluster_keys_f32", keys, F=2 ** 31), E_SHAPE, o, "keys F 2^31")
    refused(a, call("mvs_mesh_cluster_keys_f32", keys, wsb=wsb - 1), E_WORKSPACE, o, "keys")
    refused(a, call("mvs_mesh_cluster_heads_i64", dict(sk=o[0], M=Mv, head=None)), E_BADARG, o, "heads head NULL")
    refused(a, call("mvs_mesh_cluster_heads_i64", dict(sk=o[0], M=2 ** 31, head=o[1])), E_SHAPE, o, "heads M 2^31")
    sums = dict(sk=o[0], order=o[1], rank=o[2], offsets=o[3], colours=None, M=Mv, **grid_args(cell), vc=o[4], cv=o[5], cc=None, ws=o[6], wsb=wsb)
    refused(a, call("mvs_mesh_cluster_sums_f32", sums, rank=None), E_BADARG, o, "sums head_rank NULL")
    refused(a, call("mvs_mesh_cluster_sums_f32", sums, cc=o[3]), E_BADARG, o, "sums colours out without colours in")
    refused(a, call("mvs_mesh_cluster_sums_f32", sums, M=2 ** 31), E_SHAPE, o, "sums M 2^31")
    refused(a, call("mvs_mesh_cluster_sums_f32", sums, wsb=wsb - 1), E_WORKSPACE, o, "sums")
    faces = dict(faces=tf, M=Mv, F=Fv, vc=o[0], cf=o[1], lo=o[2], hi=None, ws=o[6], wsb=wsb)
    refused(a, call("mvs_mesh_cluster_faces_i32", faces, lo=None), E_BADARG, o, "faces key_lo NULL")
    refused(a, call("mvs_mesh_cluster_faces_i32", faces, M=2 ** 21 + 1, wsb=2 ** 40), E_SHAPE, o, "faces one key beyond 2^21 vertices")
    refused(a, call("mvs_mesh_cluster_faces_i32", faces, wsb=wsb - 1), E_WORKSPACE, o, "faces")
    mark = dict(cf=o[1], M=Mv, F=Fv, lo=o[2], hi=None, order=o[3], fk=o[4], vk=o[5], ws=o[6], wsb=wsb)
    refused(a, call("mvs_mesh_cluster_mark_i32", mark, order=None), E_BADARG, o, "mark order NULL")
    refused(a, call("mvs_mesh_cluster_mark_i32", mark, F=-1), E_BADARG, o, "mark F -1")
    refused(a, call("mvs_mesh_cluster_mark_i32", mark, wsb=wsb - 1), E_WORKSPACE, o, "mark")
    assert size("mvs_mesh_cluster_workspace_bytes", -1, 0) == 0 and size("mvs_mesh_cluster_workspace_bytes", 2 ** 31, 0) == 0
    a.check()


def test_every_mesh_cluster_entry_point_is_called_here():
    """The mvs_mesh_cluster* names of _lib.SIGNATURES (they stand before mvs_fusion_workspace_bytes, outside the range that
    test_gpu_arena_geometry.py pins) against the names this file passes to call() and size()."""
    declared = {name for name in L.SIGNATURES if name.startswith("mvs_mesh_cluster")}
    with open(os.path.abspath(__file__).replace(".pyc", ".py")) as fh:
        called = set(re.findall(r"\"(mvs_[a-z0-9_]+)\"", fh.read()))
    assert declared - called == set(), "no arena case calls %s" % sorted(declared - called)
    assert len(declared) == 6
    names = list(L.SIGNATURES)
    assert all(names.index(name) < names.index("mvs_fusion_workspace_bytes") for name in declared)
