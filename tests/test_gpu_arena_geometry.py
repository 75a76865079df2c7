"""Every geometry entry point (include/mvsnet_hip.h from mvs_fusion_workspace_bytes to the end: fusion.hip, pointcloud.hip,
render.hip, view_selection.hip, tsdf.hip, raster.hip, mesh_components.hip) with ALL of its operands inside one poisoned, guarded
device arena (tests/device_arena.py), as tests/test_gpu_arena.py does for the hot path.

The comparisons are those of the families' own GPU tests, against the same numpy restatements (each case names the test it takes
its assertion from); what is new is WHERE the operands live: views into one uint8 tensor filled with 0xFF (NaN / -1; also the
cleared state GEO_EMPTY of the z-buffer keys, so a missing clear of those shows only under 0x7F) or 0x7F (3.4e38 / 2139062143: a
plausible count, an impossible offset), at 16-byte but never 256-byte multiples, 64 KiB of pattern on both sides, workspaces of
exactly the queried size, inputs read-only, outputs left as pattern.  Every case asserts: the oracle comparison; arena.check();
the call is refused with MVS_E_WORKSPACE one byte below the queried size and every output still holds the pattern afterwards;
capacity outputs hold the pattern beyond what was produced.  Calls go through the C ABI; what the Python plans do in torch
between two calls (the stable sort of the voxel keys, the scans of surface nets and of the compaction) is done in torch here
too and copied into an arena region.  Accumulators the header says the caller clears (the TSDF sums, the visibility mask) are
cleared by the test inside the arena.

What first writes each workspace piece and each caller-provided accumulator in a call, and what reads it -- read from the
launchers before this file was first run, because a poisoned integer used as an address is an out-of-bounds access, not a failed
assertion.  "all" = every element of the piece; an index is shown to be written before it is read.

  fusion.hip (fusion_launch; FuLayout)
    df        geo_filter_kernel stores all V*H*W                     | normal_map, pairs (gathers at s*HW + q, q inside the image), finalize
    nmap      fusion_normal_map_kernel stores all V*HW (float4)      | pairs (own pixel, gather at s*HW + q), finalize
    used      hipMemsetAsync(0) of all V*HW bytes (dedupe only)      | pairs, finalize; finalize stores 1 at used[w], w = witness
    part      pairs stores every plane of every slice for p < HW     | finalize sums slices 0..slices-1 of p < HW.  Every block
              (a slice with no sources stores zeros)                 |   (x, view, slice) of the grid stores, also when j0 == j1
    witness   pairs stores witness[j*HW + p] for j0 <= j < j1;       | finalize reads j < cnt, cnt = min(list length, max_sources):
              slices * chunk >= max_sources >= cnt covers j < cnt    |   every element read was stored by this view's pairs launch.
              values: -1 or s*HW + q with s < V, q < HW              |   As an index into `used` it is < V*HW
    keep      finalize stores all (every view, every p < HW)         | geo_compact_count_kernel, fusion_write_kernel
    fxyz,fnrm finalize stores all                                    | write (kept elements only)
    counts    geo_compact_count_kernel stores all nb                 | geo_scan_top_kernel
    offs      geo_scan_top_kernel stores all nb                      | write: offs[block] + rank < *count <= V*HW: inside the outputs
    count     geo_scan_top_kernel STORES the total (output, not +=)  | --
  pointcloud.hip
    starts    mvs_nn_f32: hipMemsetAsync(0) of both arrays (2 * stride ints, padding included); target build: ncell + 1 ints.
              pc_cell_count_kernel adds to cells < ncell; pc_scan (reduce, top, apply) rewrites all ncell + 1 in place
              | scatter: start[cellid[i]]; query: tstart[row + xa] .. tstart[row + xb + 1] <= tstart[ncell]
    bsum      pc_scan_reduce_kernel stores chunk totals 0..nb-1 of each array; scan_top rewrites them in place; entry nb of an
              array is never read | pc_scan_apply_kernel reads bsum[chunk], chunk < nb
    cells, ranks (tcell, trank, qcell, qrank)  pc_cell_count_kernel stores all n | scatter, icp step (tcell[bi], trank[bi], bi a
              target index the query returned: < n_target)
    sorted copies  pc_scatter_kernel stores sorted[start[cell] + rank]: a permutation of 0..n-1, so all n | query reads ts[k],
              tstart[a] <= k < tstart[b] <= n_target; icp reads ts[tstart[tcell[bi]] + trank[bi]]
    ICP partials  pc_icp_step_kernel stores 18 doubles for each of its nb blocks | pc_icp_final_kernel reads blocks < nb
    moments   pc_icp_final_kernel STORES all 18 | --
    stats partials psum[b], pcnt[b*17 + 0..16] stored by every block (all 16 threshold slots) | final reads k <= n_thresholds
    out       pc_stats_final_kernel STORES 2 + n_thresholds doubles | --
    keep      pc_voxel_mark_kernel stores keep[order[i]], all n when order is a permutation (the caller's sort) | count, write
    offs      compact_count stores 0..nb-1, hipMemsetAsync(0) entry nb, pc_scan rewrites all nb + 1 | write: offs[block], offs[nb]
    count     pc_compact_write_kernel STORES offs[nb] | --
  render.hip / raster.hip
    keys      hipMemsetAsync(0xFF) of all pixels | splat / small / large kernels (atomic minima at pixels inside the image), resolve
    raw map   geo_resolve_kernel stores all pixels (occlusion only) | rd_filter_kernel (tile loads clipped to the image)
    head      raster: hipMemsetAsync(0) of the 256-byte counter block | small kernel takes tickets; large kernel reads the count
    queue     the lane that drew ticket t < queue_capacity stores queue[t]; tickets are consecutive | large kernel reads
              e < min(count, queue_capacity): each was stored.  (face, view) of an entry are range-checked again
    depth, index  resolve / filter store all pixels (index only when not NULL) | --
  view_selection.hip
    tile counters  hipMemsetAsync(0) before every segment's launch | vs_score_kernel draws chunks with atomicAdd
    score_sum, shared, hist  hipMemsetAsync(0) by the call, then integer atomics: outputs, whatever they held
    mask      caller-cleared accumulator: the kernel ORs bits in (row[word] |= bits)
  tsdf.hip
    df        geo_filter_kernel stores all V*H*W | ts_integrate_kernel gathers inside the image (or element 0, masked)
    sum, count, rgb_sum, rgb_count  caller-cleared accumulators: read, added to, stored back for every node
    cell flags ts_classify_kernel stores all cells (one zero by hipMemsetAsync when an axis has one node) | edges, write
    face counts ts_edges_kernel stores all nodes (hipMemsetAsync(0) when an axis has one node) | write; the caller's scan
    totals    hipMemsetAsync(0) of both, then atomic adds: an output, whatever it held
    cell_rank, face_end  the caller's scans: write stores vertex rank - 1 only when < M, faces at face_end - count only when
              inside 0..F: a larger capacity is left alone beyond the totals
  mesh_components.hip
    status    hipMemsetAsync(0) of the 64 words by label; measure stores 0 to word 2 before it counts
    parents, minima  mc_init_kernel stores all M (parent[v] = v: every walk stays inside 0..M-1) | link (valid faces only:
              indices checked), roots, labels
    vertex_labels  roots stores the root of every v, then root_min[root] | face labels, boxes (label range-checked)
    face_labels  link stores all F (0 or -1), face_labels_kernel completes the valid ones
    vertex_keep  hipMemsetAsync(0) by mark, then stores of 1;  face_keep stored for all F
No element was found that is read before it is written, and every family works at 16-byte alignment (float4 copies and 64-bit
keys at 256-byte multiples of the workspace start): no kernel or launcher was changed.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L
from mvsnet_amd import evaluate as E
from mvsnet_amd import fusion as F
from mvsnet_amd import mesh as MESH
from mvsnet_amd import render as RN
from mvsnet_amd import select_views as SV

from tests import fusion_reference as FR
from tests import mesh_clean_reference as MC
from tests import mesh_reference as M
from tests import normals_reference as NR
from tests import pointcloud_reference as PR
from tests import raster_reference as RR
from tests import registration_reference as G
from tests import render_reference as R
from tests import view_selection_reference as VR
from tests.device_arena import PATTERNS, Arena

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
F32, F64, I16, I32, I64, U8 = torch.float32, torch.float64, torch.int16, torch.int32, torch.int64, torch.uint8
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


# ---- small helpers -----------------------------------------------------------------------------------------------------------
def arena(pattern, mb=8):
    return Arena(mb << 20, pattern, DEV)


def put(a, name, array, dtype=F32):
    """An input: copied in, read-only.  array: numpy or a tensor (what torch computed between two calls)."""
    shape = tuple(array.shape)
    return a.take(shape, dtype, data=array if isinstance(array, torch.Tensor) else np.ascontiguousarray(array), readonly=True, name=name)


def out(a, name, *shape, dtype=F32):
    return a.take(shape, dtype, name=name)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def size(name, *ints):
    return int(getattr(L.load(), name)(*[int(v) for v in ints]))


def call(name, args, **override):
    """One library call: `args` holds the arguments in the header's order without the stream; tensors become pointers."""
    p = dict(args)
    for k in override:
        assert k in p, k
    p.update(override)
    vals = [L.ptr(v) if isinstance(v, torch.Tensor) else int(v) if isinstance(v, (np.integer, bool)) else v for v in p.values()]
    return getattr(L.load(), name)(*vals, L.stream_ptr())


def refused(a, rc, code, outs, what):
    """The call was refused with `code` and every output region still holds the pattern."""
    assert rc == code, "%s: expected %d, got %d" % (what, code, rc)
    torch.cuda.synchronize()
    for o in outs:
        assert a.is_pattern(o), "%s wrote an output although it answered %d" % (what, rc)


def run(a, name, args, outs, key="wsb"):
    """Refused one byte below the queried workspace size with the outputs untouched, then succeeds at exactly that size."""
    refused(a, call(name, args, **{key: args[key] - 1}), E_WORKSPACE, outs, name + " one byte short")
    L.check(call(name, args), name)


def floats(*v):
    return (C.c_float * len(v))(*[float(x) for x in v])


def doubles(*v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def frozen(*arrays):
    for x in arrays:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return arrays


def same_bytes(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    bad = int((got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8)).sum())
    assert bad == 0, "%s: %d bytes differ" % (what, bad)


# ==== 1. fusion ===============================================================================================================
@functools.lru_cache(maxsize=None)
def fusion_scene(name):
    """sphere / noisy: the cached scenes of test_gpu_normals.py; kat: the exact line layout; tiny: 3 views of 5 x 7, one block
    holds a whole view (line layout, f = 64: every correspondence an integer shift)."""
    from tests import test_gpu_normals as TN
    if name == "sphere":
        return TN._scene("sphere")
    if name == "noisy":
        return TN._noisy_sphere()
    if name == "kat":
        return TN._scene("kat", low_prob_fraction=0.0)
    return FR.make_scene(kind="plane", V=3, H=5, W=7, layout="line", f=64.0, seed=7, image_scale=2)


def _key(sources):
    return None if sources is None else tuple(tuple(l) for l in sources)


@functools.lru_cache(maxsize=None)
def fusion_reference(name, N, dedupe, sources, images, normals=False, angle=None):
    s = fusion_scene(name)
    src = None if sources is None else [list(l) for l in sources]
    im = s["images"] if images else None
    if normals:
        return NR.reference_fusion_normals(s["depths"], s["probs"], s["cams"], im, num_consistent=N, sources=src, dedupe=dedupe,
                                           normal_angle_threshold=angle)
    return FR.reference_fusion(s["depths"], s["probs"], s["cams"], im, num_consistent=N, sources=src, dedupe=dedupe)


def fusion_setup(a, s, *, N, dedupe, sources=None, images=True, pixels=True, normals=False, cos=-1.0, tag=""):
    """-> (entry point, args, outputs).  Workspace of exactly the queried size; outputs and count left as pattern."""
    V, H, W = s["depths"].shape
    lists = F.source_lists(V, sources)
    ms = max(len(l) for l in lists)
    offs = np.zeros(V + 1, np.int32)
    offs[1:] = np.cumsum([len(l) for l in lists])
    idx = np.array([x for l in lists for x in l], np.int32)
    px = V * H * W
    p = dict(depth=put(a, "depth" + tag, s["depths"]), prob=put(a, "prob" + tag, s["probs"]), V=V, H=H, W=W,
             tables=put(a, "tables" + tag, F.camera_tables(s["cams"])), offs=put(a, "src_offsets" + tag, offs, I32),
             idx=put(a, "src_index" + tag, idx, I32) if len(idx) else None, ms=ms, prob_thr=0.8, reproj=1.0, drel=0.01, N=float(N),
             dedupe=int(dedupe))
    if normals:
        p.update(jump=0.05, cos=float(cos))
    im = put(a, "images" + tag, s["images"], U8) if images else None
    p.update(images=im, ih=im.shape[1] if images else 0, iw=im.shape[2] if images else 0,
             xyz=out(a, "xyz" + tag, px, 3), rgb=out(a, "rgb" + tag, px, 3, dtype=U8))
    if normals:
        p.update(nrm=out(a, "normals" + tag, px, 3))
    p.update(view=out(a, "view_index" + tag, px, dtype=I32), pix=out(a, "pixel_index" + tag, px, dtype=I32) if pixels else None,
             count=out(a, "count" + tag, 1, dtype=I32))
    wsb = size("mvs_fusion_normals_workspace_bytes" if normals else "mvs_fusion_workspace_bytes", V, H, W, ms, dedupe)
    assert wsb > 0
    p.update(ws=a.take_bytes(wsb, name="workspace" + tag), wsb=wsb)
    outs = [p[k] for k in ("xyz", "rgb", "nrm", "view", "pix", "count") if p.get(k) is not None]
    return ("mvs_fusion_normals_f32" if normals else "mvs_fusion_f32"), p, outs


def fusion_result(a, p):
    """The points, with everything at and beyond *count of the capacity outputs still pattern."""
    cnt = int(n(p["count"])[0])
    assert 0 <= cnt <= p["V"] * p["H"] * p["W"]
    res = {}
    for k in ("xyz", "rgb", "nrm", "view", "pix"):
        if p.get(k) is not None:
            assert a.is_pattern(p[k][cnt:]), "%s was written beyond the %d points" % (k, cnt)
            res[k] = n(p[k][:cnt])
    return res


def fusion_compare(s, ref, got, exact):
    """exact: test_gpu_fusion.test_device_dedupe_exact_on_kats; else test_gpu_fusion._compare_exact_where_margin."""
    from tests.test_gpu_fusion import _compare_exact_where_margin
    V, H, W = s["depths"].shape
    if not exact:
        _compare_exact_where_margin(s, ref, (got["xyz"], got["rgb"], got["view"], got["pix"]), H, W)
        return
    m = ref["margin"]
    assert m[np.isfinite(m)].min() > 1e-4                        # every decision of the restatement is clear on this scene
    assert np.array_equal(got["view"], ref["view_index"]) and np.array_equal(got["pix"], ref["pixel"])
    assert np.array_equal(got["rgb"], ref["rgb"])
    depth = s["depths"].reshape(-1)[got["view"].astype(np.int64) * H * W + got["pix"]].astype(np.float64)
    assert (np.abs(got["xyz"] - ref["xyz"]).max(axis=1) <= 1e-5 * depth).all()


FUSION_CASES = {
    # name: scene, N, dedupe, sources (None = every other view), images, exact
    "sphere, every source, no dedupe": ("sphere", 2, False, None, True, False),
    "kat, dedupe, four slices": ("kat", 2, True, None, True, True),
    "kat, dedupe, one source": ("kat", 1, True, ((1,), (2,), (3,), (4,), (3,)), True, True),
    "kat, no dedupe, one source, no images": ("kat", 1, False, ((1,), (2,), (3,), (4,), (3,)), False, True),
    "tiny, every source": ("tiny", 1, False, None, True, True),
    "tiny, dedupe": ("tiny", 1, True, None, False, True),
}


@both_patterns
@pytest.mark.parametrize("case", sorted(FUSION_CASES))
def test_fusion(case, pattern):
    name, N, dedupe, sources, images, exact = FUSION_CASES[case]
    s = fusion_scene(name)
    a = arena(pattern)
    fn, p, outs = fusion_setup(a, s, N=N, dedupe=dedupe, sources=sources, images=images)
    if dedupe and sources is None:
        assert p["ms"] == s["depths"].shape[0] - 1 > 1             # more than one slice (fusion_slices: min(16, max_sources) here)
    run(a, fn, p, outs)
    got = fusion_result(a, p)
    a.check()
    ref = fusion_reference(name, N, dedupe, sources, images)
    assert len(got["xyz"]) > 0 and (images or not got["rgb"].any())
    fusion_compare(s, ref, got, exact)


@both_patterns
@pytest.mark.parametrize("dedupe", [False, True])
def test_fusion_without_sources_images_and_pixel_index(dedupe, pattern):
    """max_sources = 0 (src_index NULL), images NULL, pixel_index NULL; num_consistent = 0 keeps exactly the valid pixels
    (test_gpu_fusion.test_compaction_at_block_boundaries).  A second call with pixel_index gives the pixels to compare with."""
    s = fusion_scene("tiny")
    V, H, W = s["depths"].shape
    a = arena(pattern)
    none = [[] for _ in range(V)]
    fn, p, outs = fusion_setup(a, s, N=0, dedupe=dedupe, sources=none, images=False, pixels=False)
    assert p["ms"] == 0 and p["idx"] is None
    run(a, fn, p, outs)
    got = fusion_result(a, p)
    fn, q, _ = fusion_setup(a, s, N=0, dedupe=dedupe, sources=none, images=False, pixels=True, tag=" (2)")
    L.check(call(fn, q), fn)
    full = fusion_result(a, q)
    a.check()
    for k in ("xyz", "rgb", "view"):
        same_bytes(got[k], full[k], k)
    valid = (s["depths"] > 0) & np.isfinite(s["depths"]) & (s["probs"] >= 0.8)
    assert np.array_equal(full["view"].astype(np.int64) * H * W + full["pix"], np.nonzero(valid.reshape(-1))[0])
    fusion_compare(s, fusion_reference("tiny", 0, dedupe, _key(none), False), full, True)


@both_patterns
def test_fusion_normals_threshold_off_is_fusion_plus_normals(pattern):
    """test_gpu_normals.test_fusion_threshold_off_is_todays_fusion_plus_normals: the bytes of mvs_fusion_f32, and the normals."""
    from tests.test_gpu_normals import _compare_fused_normals
    s = fusion_scene("sphere")
    a = arena(pattern)
    fn, p, outs = fusion_setup(a, s, N=2, dedupe=False, normals=True, cos=-1.0)
    run(a, fn, p, outs)
    got = fusion_result(a, p)
    fn2, q, _ = fusion_setup(a, s, N=2, dedupe=False, tag=" (plain)")
    L.check(call(fn2, q), fn2)
    plain = fusion_result(a, q)
    a.check()
    for k in ("xyz", "rgb", "view", "pix"):
        same_bytes(got[k], plain[k], k)
    ref = fusion_reference("sphere", 2, False, None, True, True)
    _compare_fused_normals(s, ref, (got["xyz"], got["rgb"], got["view"], got["pix"], got["nrm"]))


@both_patterns
def test_fusion_normals_with_the_angle_threshold(pattern):
    """test_gpu_normals.test_fusion_with_normal_angle_threshold."""
    from tests.test_gpu_normals import _compare_fused_normals, _valid
    s = fusion_scene("noisy")
    V, H, W = s["depths"].shape
    a = arena(pattern)
    fn, p, outs = fusion_setup(a, s, N=2, dedupe=False, normals=True, cos=F.normal_cos_threshold(10))
    run(a, fn, p, outs)
    got = fusion_result(a, p)
    a.check()
    ref = fusion_reference("noisy", 2, False, None, True, True, 10)
    key = got["view"].astype(np.int64) * H * W + got["pix"]
    assert (np.diff(key) > 0).all()
    dev_keep = np.zeros(V * H * W, bool)
    dev_keep[key] = True
    clear = ref["margin"].reshape(-1) > 1e-4
    assert clear[_valid(s).reshape(-1)].mean() >= 0.995
    assert np.array_equal(dev_keep[clear], ref["keep"].reshape(-1)[clear])
    assert got["nrm"].any(1).all()
    assert _compare_fused_normals(s, ref, (got["xyz"], got["rgb"], got["view"], got["pix"], got["nrm"])) == 0


@both_patterns
def test_fusion_normals_with_dedupe(pattern):
    """test_gpu_normals.test_dedupe_with_normals_on_kat: the layout with used, witness, nmap and fnrm all present."""
    from tests.test_gpu_normals import ANGLE_BOUND_DEG
    s = fusion_scene("kat")
    V, H, W = s["depths"].shape
    a = arena(pattern)
    fn, p, outs = fusion_setup(a, s, N=2, dedupe=True, normals=True)
    run(a, fn, p, outs)
    got = fusion_result(a, p)
    a.check()
    ref = fusion_reference("kat", 2, True, None, True, True)
    assert np.array_equal(got["view"], ref["view_index"]) and np.array_equal(got["pix"], ref["pixel"])
    assert len(got["xyz"]) == FR.plane_kat_counts(V, H, W, 4, 2)[1]
    assert NR.angle_deg(got["nrm"], np.array([0.0, 0.0, -1.0])).max() <= ANGLE_BOUND_DEG
    fusion_compare(s, ref, got, True)


@both_patterns
@pytest.mark.parametrize("name", ["sphere", "tiny"])
def test_depth_normals(name, pattern):
    """test_gpu_normals.test_normal_maps_match_reference (sphere) and test_degenerate_sizes_have_no_normals' neighbour, 5 x 7."""
    from tests.test_gpu_normals import ANGLE_BOUND_DEG, _valid
    s = fusion_scene(name)
    V, H, W = s["depths"].shape
    a = arena(pattern)
    p = dict(depth=put(a, "depth", s["depths"]), prob=put(a, "prob", s["probs"]), V=V, H=H, W=W,
             tables=put(a, "tables", F.camera_tables(s["cams"])), prob_thr=0.8, jump=0.05, normals=out(a, "normals", V, H, W, 3))
    L.check(call("mvs_depth_normals_f32", p), "mvs_depth_normals_f32")
    got = n(p["normals"])
    a.check()
    ref = NR.reference_normals(s["depths"], s["probs"], s["cams"])
    valid, clear = _valid(s), ref["margin"] > 1e-4
    assert clear[valid].mean() >= 0.999
    has = (got != 0).any(-1)                                       # (a NaN left of the pattern counts as a normal and fails below)
    assert not has[~valid].any() and np.array_equal(has[clear], ref["has"][clear])
    both = has & ref["has"] & clear
    assert both.sum() >= (0.95 if name == "sphere" else 0.5) * valid.sum()
    assert NR.angle_deg(got[both], ref["normals"][both]).max() <= ANGLE_BOUND_DEG
    assert np.abs(np.linalg.norm(got[both].astype(np.float64), axis=1) - 1).max() <= 3e-7


@both_patterns
def test_fusion_refusals_leave_the_outputs_alone(pattern):
    s = fusion_scene("tiny")
    a = arena(pattern)
    for normals in (False, True):
        fn, p, outs = fusion_setup(a, s, N=1, dedupe=True, normals=normals, tag=" n%d" % normals)
        refused(a, call(fn, p, reproj=0.0), E_BADARG, outs, fn + " reproj_threshold 0")
        refused(a, call(fn, p, depth=None), E_BADARG, outs, fn + " depth NULL")
        refused(a, call(fn, p, ms=65536), E_SHAPE, outs, fn + " max_sources 65536")
        refused(a, call(fn, p, wsb=p["wsb"] - 1), E_WORKSPACE, outs, fn)
        assert a.is_pattern(p["ws"])
    nm = dict(depth=p["depth"], prob=p["prob"], V=p["V"], H=p["H"], W=p["W"], tables=p["tables"], prob_thr=0.8, jump=0.05,
              normals=out(a, "normal maps", p["V"], p["H"], p["W"], 3))
    refused(a, call("mvs_depth_normals_f32", nm, jump=-1.0), E_BADARG, [nm["normals"]], "mvs_depth_normals_f32 jump -1")
    refused(a, call("mvs_depth_normals_f32", nm, V=65536), E_SHAPE, [nm["normals"]], "mvs_depth_normals_f32 V 65536")
    assert size("mvs_fusion_workspace_bytes", 0, 5, 7, 2, 1) == 0 and size("mvs_fusion_normals_workspace_bytes", 3, 5, 7, 65536, 1) == 0
    a.check()


# ==== 2. point cloud ==========================================================================================================
def grid_of(target, max_dist, cell):
    """evaluate.choose_grid on the target with a given cell: {"origin", "cell", "dims"}."""
    return E.choose_grid(torch.as_tensor(np.array(target)).to(DEV), max_dist, cell)


def grid_args(g):
    return dict(ox=g["origin"][0], oy=g["origin"][1], oz=g["origin"][2], cell=g["cell"], gx=g["dims"][0], gy=g["dims"][1], gz=g["dims"][2])


# nq, nt, cell (of targets in the unit cube), max_dist
NN_CASES = {"1023 on 1, one cell": (1023, 1, 2.0, 0.5), "1 on 1025, one cell": (1, 1025, 2.0, 0.2), "1025 on 1024": (1025, 1024, 0.125, 0.1),
            "3000 on 4000": (3000, 4000, 0.125, 0.05)}


@functools.lru_cache(maxsize=None)
def nn_case(case):
    nq, nt, cell, md = NN_CASES[case]
    return frozen(PR.uniform(nq, seed=nq), PR.uniform(nt, seed=nt + 7)) + (cell, md)


def nn_setup(a, q, t, g, md, tag=""):
    p = dict(query=put(a, "query" + tag, q), nq=len(q), target=put(a, "target" + tag, t), nt=len(t), **grid_args(g), md=md,
             dist=out(a, "dist" + tag, len(q)), index=out(a, "index" + tag, len(q), dtype=I32))
    wsb = size("mvs_nn_workspace_bytes", len(q), len(t), *g["dims"])
    assert wsb > 0
    p.update(ws=a.take_bytes(wsb, name="nn workspace" + tag), wsb=wsb)
    return p


def query_args(p, a, md, visited, tag):
    nq = p["nq"]
    q = {k: p[k] for k in ("nq", "nt", "ox", "oy", "oz", "cell", "gx", "gy", "gz")}
    q.update(md=md, dist=out(a, "dist" + tag, nq), index=out(a, "index" + tag, nq, dtype=I32),
             visited=out(a, "visited" + tag, nq, dtype=I32) if visited else None, ws=p["ws"], wsb=p["wsb"])
    return q


@both_patterns
@pytest.mark.parametrize("case", sorted(NN_CASES))
def test_nearest_then_query_on_the_workspace_it_left(case, pattern):
    """test_gpu_pointcloud_eval._check_against_reference for both calls; the workspace is const to mvs_nn_query_f32."""
    from tests.test_gpu_pointcloud_eval import _check_against_reference
    q, t, cell, md = nn_case(case)
    g = grid_of(t, md, cell)
    assert (g["dims"] == [1, 1, 1]) == (cell > 1) and np.prod(g["dims"]) <= 9 ** 3
    a = arena(pattern)
    p = nn_setup(a, q, t, g, md)
    run(a, "mvs_nn_f32", p, [p["dist"], p["index"]])
    d, i = n(p["dist"]), n(p["index"])
    a.freeze(p["ws"])
    a.check()
    _check_against_reference(q, t, md, d, i.astype(np.int64))
    # the same query again without `visited`: the same bytes; then another max_dist with `visited`
    same = query_args(p, a, md, False, " (again)")
    run(a, "mvs_nn_query_f32", same, [same["dist"], same["index"]])
    same_bytes(n(same["dist"]), d, "dist")
    same_bytes(n(same["index"]), i, "index")
    other = query_args(p, a, 0.37 * md, True, " (smaller cap)")
    run(a, "mvs_nn_query_f32", other, [other["dist"], other["index"], other["visited"]])
    d2, i2, seen = n(other["dist"]), n(other["index"]), n(other["visited"])
    a.check()
    _check_against_reference(q, t, 0.37 * md, d2, i2.astype(np.int64))
    assert (seen >= (i2 >= 0)).all() and (seen <= 64 * len(t)).all()   # a found point was compared; a count, not the pattern


@functools.lru_cache(maxsize=None)
def icp_case():
    tgt = G.asymmetric_scene(3000, seed=31)
    T0 = G.rigid()
    src = PR.transform(PR.noisy(G.asymmetric_scene(2500, seed=32), 0.3, seed=33), np.linalg.inv(T0))
    Ts = (np.eye(4), T0, G.rigid(degrees=1.5, translation=(0.7, -0.5, 0.4)))
    cp, cq = src.astype(np.float64).mean(0), tgt.astype(np.float64).mean(0)
    return frozen(src, tgt) + (Ts, cp, cq)


def target_setup(a, t, g, tag=""):
    p = dict(target=put(a, "target" + tag, t), nt=len(t), **grid_args(g))
    wsb = size("mvs_nn_target_workspace_bytes", len(t), *g["dims"])
    assert wsb > 0
    p.update(ws=a.take_bytes(wsb, name="target workspace" + tag), wsb=wsb)
    return p


def icp_setup(a, src, tp, T, cp, cq, md, order, with_corr, tag=""):
    ns = len(src)
    p = dict(source=src, ns=ns, order=order, T=doubles(*np.asarray(T)[:3].reshape(-1)), cp=doubles(*cp), cq=doubles(*cq),
             **{k: tp[k] for k in ("ox", "oy", "oz", "cell", "gx", "gy", "gz", "nt")}, tws=tp["ws"], twsb=tp["wsb"], md=md,
             moments=out(a, "moments" + tag, 18, dtype=F64), dist=out(a, "icp dist" + tag, ns) if with_corr else None,
             index=out(a, "icp index" + tag, ns, dtype=I32) if with_corr else None)
    wsb = size("mvs_icp_step_workspace_bytes", ns)
    p.update(ws=a.take_bytes(wsb, name="icp workspace" + tag), wsb=wsb)
    return p


def icp_check(src, tgt, T, cp, cq, md, m, d=None, i=None):
    """test_gpu_registration.test_one_step_matches_the_reference: which neighbour, then how it was summed; and the step of
    registration_reference where its correspondences are the device's."""
    from tests.test_gpu_pointcloud_eval import _check_against_reference
    from tests.test_gpu_registration import _check_moments
    assert m.shape == (18,) and np.isfinite(m).all()
    m_ref, idx_ref = G.step(src, tgt, T, md, cp, cq)
    if i is not None:
        _check_against_reference(PR.transform(src, T), tgt, md, d, i.astype(np.int64))
    idx = idx_ref if i is None else i.astype(np.int64)
    ref, bound = _check_moments(m, src, tgt, idx, T, cp, cq)
    if np.array_equal(idx, idx_ref):
        assert (np.abs(m - m_ref) <= bound).all()
    assert m[0] == (idx >= 0).sum()


@both_patterns
@pytest.mark.parametrize("mode", ["input order, no correspondences", "permuted, with correspondences"])
def test_target_build_then_three_icp_steps(mode, pattern):
    """One target build, frozen, then three steps with different T through one step workspace."""
    src, tgt, Ts, cp, cq = icp_case()
    md = G.MAX_CORR_DIST
    g = grid_of(tgt, md, 12.0)
    a = arena(pattern)
    tp = target_setup(a, tgt, g)
    run(a, "mvs_nn_target_build_f32", tp, [])
    a.freeze(tp["ws"])
    with_corr = mode.startswith("permuted")
    s_in = put(a, "source", src)
    order = put(a, "order", np.random.RandomState(5).permutation(len(src)).astype(np.int32), I32) if with_corr else None
    first = None
    for k, T in enumerate(Ts):
        p = icp_setup(a, s_in, tp, T, cp, cq, md, order, with_corr, tag=" %d" % k)
        if first is not None:
            p["ws"] = first["ws"]                                  # the same step workspace, call after call
        first = first or p
        outs = [x for x in (p["moments"], p["dist"], p["index"]) if x is not None]
        refused(a, call("mvs_icp_step_f32", p, twsb=p["twsb"] - 1), E_WORKSPACE, outs, "icp, target workspace one byte short")
        run(a, "mvs_icp_step_f32", p, outs)
        m = n(p["moments"])
        a.check()
        icp_check(src, tgt, T, cp, cq, md, m, *((n(p["dist"]), n(p["index"])) if with_corr else ()))
        if k == 1:
            assert m[0] > 0.8 * len(src)                           # T0 brings the clouds together


@both_patterns
@pytest.mark.parametrize("n_thr", [0, 16])
@pytest.mark.parametrize("npts", [1, 2049, 5000])
def test_dist_stats(npts, n_thr, pattern):
    """Counts exact, the inlier mean within 1e-6 (test_gpu_pointcloud_eval.test_metrics_match_reference); 2049 = two blocks."""
    rs = np.random.RandomState(npts)
    d = rs.uniform(0, 4, npts).astype(np.float32)
    d[rs.rand(npts) < 0.1] = np.inf
    md = 3.0
    thr = np.linspace(0.2, 3.0, n_thr).astype(np.float32)
    a = arena(pattern)
    p = dict(dist=put(a, "dist", d), n=npts, md=md, thr=floats(*thr) if n_thr else None, nthr=n_thr,
             out=out(a, "out", 2 + n_thr, dtype=F64))
    wsb = size("mvs_dist_stats_workspace_bytes", npts, n_thr)
    p.update(ws=a.take_bytes(wsb, name="stats workspace"), wsb=wsb)
    run(a, "mvs_dist_stats_f32", p, [p["out"]])
    got = n(p["out"])
    a.check()
    inl = d[d < np.float32(md)].astype(np.float64)
    assert got[1] == len(inl) and [int(x) for x in got[2:]] == [int((d < t).sum()) for t in thr]
    assert abs(got[0] - inl.sum()) <= 1e-6 * abs(inl.sum())


@both_patterns
@pytest.mark.parametrize("npts", [1, 1023, 1024, 1025, 3000])
def test_voxel_keys_sort_select(npts, pattern):
    """test_gpu_pointcloud_eval.test_voxel_compaction_at_block_boundaries (its cloud) and 3 000 uniform points: the keys, the
    stable sort in torch as evaluate._voxel does it, the selection; `out` holds the pattern beyond *count."""
    if npts == 3000:
        pts, s = PR.uniform(npts, 0.0, 10.0, seed=3), 1.5
    else:
        keep = np.random.RandomState(npts).rand(npts) < 0.3
        keep[0] = keep[-1] = True
        i = np.arange(npts)
        pts, s = np.zeros((npts, 3), np.float32), 1.0
        pts[:, 0] = np.where(keep, i + 0.5, 0.5)
        pts[:, 1] = (i % 7) / 16.0
    want = PR.voxel_first(pts, s)
    a = arena(pattern)
    x = put(a, "xyz", pts)
    lo = pts.astype(np.float64).min(0)
    k = dict(xyz=x, n=npts, mx=float(lo[0]), my=float(lo[1]), mz=float(lo[2]), cell=float(s), keys=out(a, "keys", npts, dtype=I64))
    L.check(call("mvs_voxel_keys_f32", k), "mvs_voxel_keys_f32")
    vk = PR.voxel_keys(pts, s)
    assert np.array_equal(n(k["keys"]), vk[:, 0] | (vk[:, 1] << 21) | (vk[:, 2] << 42))
    sk, order = torch.sort(k["keys"], stable=True)
    p = dict(xyz=x, n=npts, sk=put(a, "sorted keys", sk, I64), order=put(a, "order", order, I64), out=out(a, "out", npts, 3),
             count=out(a, "count", 1, dtype=I32))
    wsb = size("mvs_voxel_select_workspace_bytes", npts)
    p.update(ws=a.take_bytes(wsb, name="select workspace"), wsb=wsb)
    run(a, "mvs_voxel_select_f32", p, [p["out"], p["count"]])
    cnt = int(n(p["count"])[0])
    a.check()
    assert cnt == len(want) and n(p["out"][:cnt]).tobytes() == want.tobytes()
    assert a.is_pattern(p["out"][cnt:])


@both_patterns
def test_point_cloud_refusals_leave_the_outputs_alone(pattern):
    q, t, cell, md = nn_case("1025 on 1024")
    g = grid_of(t, md, cell)
    a = arena(pattern)
    p = nn_setup(a, q, t, g, md)
    outs = [p["dist"], p["index"]]
    refused(a, call("mvs_nn_f32", p, md=0.0), E_BADARG, outs, "nn max_dist 0")
    refused(a, call("mvs_nn_f32", p, gx=257, gy=257, gz=257), E_SHAPE, outs, "nn 257^3 cells")
    qa = query_args(p, a, md, True, " q")
    qo = [qa["dist"], qa["index"], qa["visited"]]
    refused(a, call("mvs_nn_query_f32", qa, cell=0.0), E_BADARG, qo, "query cell 0")
    refused(a, call("mvs_nn_query_f32", qa, gx=257, gy=257, gz=257), E_SHAPE, qo, "query 257^3 cells")
    refused(a, call("mvs_nn_query_f32", qa, wsb=qa["wsb"] - 1), E_WORKSPACE, qo, "query")
    tp = target_setup(a, t, g)
    refused(a, call("mvs_nn_target_build_f32", tp, nt=0), E_BADARG, [tp["ws"]], "target build n 0")
    refused(a, call("mvs_nn_target_build_f32", tp, gx=257, gy=257, gz=257), E_SHAPE, [tp["ws"]], "target build 257^3 cells")
    refused(a, call("mvs_nn_target_build_f32", tp, wsb=tp["wsb"] - 1), E_WORKSPACE, [tp["ws"]], "target build")
    ip = icp_setup(a, p["query"], tp, np.eye(4), (0, 0, 0), (0, 0, 0), md, None, True)
    io = [ip["moments"], ip["dist"], ip["index"]]
    refused(a, call("mvs_icp_step_f32", ip, T=doubles(*([float("nan")] * 12))), E_BADARG, io, "icp T NaN")
    refused(a, call("mvs_icp_step_f32", ip, gx=257, gy=257, gz=257), E_SHAPE, io, "icp 257^3 cells")
    sp = dict(dist=p["query"].view(-1), n=100, md=1.0, thr=floats(0.5, 2.0), nthr=2, out=out(a, "stats", 4, dtype=F64),
              ws=a.take_bytes(size("mvs_dist_stats_workspace_bytes", 100, 2)), wsb=size("mvs_dist_stats_workspace_bytes", 100, 2))
    refused(a, call("mvs_dist_stats_f32", sp), E_BADARG, [sp["out"]], "stats threshold above max_dist")
    refused(a, call("mvs_dist_stats_f32", sp, thr=floats(*([0.5] * 17)), nthr=17), E_SHAPE, [sp["out"]], "stats 17 thresholds")
    kp = dict(xyz=p["query"], n=10, mx=0.0, my=0.0, mz=0.0, cell=0.0, keys=out(a, "keys", 10, dtype=I64))
    refused(a, call("mvs_voxel_keys_f32", kp), E_BADARG, [kp["keys"]], "voxel keys cell 0")
    vp = dict(xyz=p["query"], n=0, sk=kp["keys"], order=kp["keys"], out=out(a, "vout", 10, 3), count=out(a, "vcount", 1, dtype=I32),
              ws=a.take_bytes(size("mvs_voxel_select_workspace_bytes", 10)), wsb=size("mvs_voxel_select_workspace_bytes", 10))
    refused(a, call("mvs_voxel_select_f32", vp), E_BADARG, [vp["out"], vp["count"]], "voxel select n 0")
    for name, args in (("mvs_nn_workspace_bytes", (10, 10, 257, 257, 257)), ("mvs_nn_target_workspace_bytes", (0, 1, 1, 1)),
                       ("mvs_icp_step_workspace_bytes", (0,)), ("mvs_dist_stats_workspace_bytes", (10, 17)),
                       ("mvs_voxel_select_workspace_bytes", (0,))):
        assert size(name, *args) == 0, name
    assert a.is_pattern(p["ws"])
    a.check()


# ==== 3. render ===============================================================================================================
def cloud_cams(H, W):
    return R.scale_cams(R.scene_cloud()[1], 40, 48, H, W)


# name: H, W, every n-th point, splat, occlusion, index, permuted order
RENDER_CASES = {
    "40x48 plain": (40, 48, 1, 0, None, True, False),
    "40x48 splat 1, occlusion, permuted": (40, 48, 2, 1, (1, 0.1, 2), True, True),
    "37x53 occlusion radius 2, no index": (37, 53, 2, 0, (2, 0.1, 2), False, False),
    "37x53 splat 2, no index, permuted": (37, 53, 1, 2, None, False, True),
    "5x7 splat 1": (5, 7, 1, 1, None, True, True),
}


@functools.lru_cache(maxsize=None)
def render_reference(H, W, every, splat, occlusion):
    return frozen(*R.render(R.scene_cloud()[0][::every], cloud_cams(H, W), H, W, splat=splat, occlusion=occlusion))


def render_setup(a, pts, cams, H, W, splat, occlusion, index, order, tag="", ws=None):
    V = len(cams)
    k, rel, count = occlusion if occlusion else (0, 0.0, 0)
    p = dict(xyz=put(a, "xyz" + tag, pts), n=len(pts), order=put(a, "order" + tag, order, I32) if order is not None else None,
             proj=put(a, "proj" + tag, RN.projection_tables(cams)), V=V, H=H, W=W, splat=splat, md=0.0, k=k,
             ratio=RN.occlusion_ratio(rel) if k else 0.0, count=count, depth=out(a, "depth" + tag, V, H, W),
             index=out(a, "index" + tag, V, H, W, dtype=I32) if index else None)
    wsb = size("mvs_render_workspace_bytes", V, H, W, 1 if occlusion else 0)
    assert wsb > 0
    p.update(ws=a.take_bytes(wsb, name="render workspace" + tag) if ws is None else ws, wsb=wsb)
    return p, [x for x in (p["depth"], p["index"]) if x is not None]


@both_patterns
@pytest.mark.parametrize("case", sorted(RENDER_CASES))
def test_render_points(case, pattern):
    """test_gpu_render._assert_same against render_reference.render (depth bits and index equal)."""
    from tests.test_gpu_render import _assert_same
    H, W, every, splat, occlusion, index, permuted = RENDER_CASES[case]
    pts = R.scene_cloud()[0][::every]
    order = np.random.RandomState(2).permutation(len(pts)).astype(np.int32) if permuted else None
    a = arena(pattern)
    p, outs = render_setup(a, pts, cloud_cams(H, W), H, W, splat, occlusion, index, order)
    run(a, "mvs_render_points_f32", p, outs)
    depth = n(p["depth"])
    want = render_reference(H, W, every, splat, occlusion)
    a.check()
    assert (want[0] > 0).mean() > 0.05
    _assert_same((depth, n(p["index"]) if index else want[1].copy()), want)


@both_patterns
def test_render_refusals_leave_the_outputs_alone(pattern):
    a = arena(pattern)
    p, outs = render_setup(a, R.scene_cloud()[0][::8], cloud_cams(5, 7), 5, 7, 1, (1, 0.1, 2), True, None)
    outs = outs + [p["ws"]]
    refused(a, call("mvs_render_points_f32", p, splat=33), E_BADARG, outs, "splat 33")
    refused(a, call("mvs_render_points_f32", p, ratio=1.0), E_BADARG, outs, "occl_ratio 1")
    refused(a, call("mvs_render_points_f32", p, H=(1 << 24) + 1), E_SHAPE, outs, "H 2^24 + 1")
    refused(a, call("mvs_render_points_f32", p, wsb=p["wsb"] - 1), E_WORKSPACE, outs, "render")
    # without occlusion the query is smaller by the raw map, and that smaller size is refused with occlusion on
    assert size("mvs_render_workspace_bytes", 5, 5, 7, 0) < p["wsb"] and size("mvs_render_workspace_bytes", 5, 0, 7, 0) == 0
    refused(a, call("mvs_render_points_f32", p, wsb=size("mvs_render_workspace_bytes", 5, 5, 7, 0)), E_WORKSPACE, outs, "raw map")
    a.check()


# ==== 4. view selection =======================================================================================================
@functools.lru_cache(maxsize=None)
def view_case(zbuffer):
    """The five-view sphere cloud at 40 x 48 (test_gpu_view_selection's scene): points, cams, z-buffer, visibility, mask."""
    pts, cams = R.scene_cloud()[0], VR.scene_cams((40, 48))
    z = VR.zbuffer(pts, cams, 40, 48, 1, None, 0.0) if zbuffer else None
    vis = VR.visibility(pts, cams, 40, 48, 0.0, z, 0.01)
    return frozen(pts, cams, z, vis, VR.pack_mask(vis))


def visibility_args(a, xyz, cams, bits, zbuf, mask, words, H=40, W=48, tag=""):
    return dict(xyz=xyz, n=xyz.shape[0], proj=put(a, "proj" + tag, RN.projection_tables(cams)), bits=put(a, "view_bits" + tag, np.asarray(bits, np.int32), I32),
                V=len(cams), H=H, W=W, md=0.0, zbuf=put(a, "zbuf" + tag, zbuf) if zbuf is not None else None, ztol=SV.z_tolerance(0.01),
                mask=mask, words=words)


@both_patterns
@pytest.mark.parametrize("zbuffer", [False, True], ids=["frustum", "zbuffer"])
def test_view_visibility(zbuffer, pattern):
    """test_gpu_view_selection._assert_same on the mask, against view_selection_reference.visibility.  The mask is the caller's
    to clear: it is cleared here, inside the arena."""
    pts, cams, z, vis, want = view_case(zbuffer)
    a = arena(pattern)
    mask = out(a, "mask", len(pts), 1, dtype=I64)
    p = visibility_args(a, put(a, "xyz", pts), cams, range(5), z, mask, 1)
    mask.zero_()
    L.check(call("mvs_view_visibility_f32", p), "mvs_view_visibility_f32")
    got = n(mask)
    a.check()
    assert vis.sum(0).min() > 0
    same_bytes(got, want, "mask")


@both_patterns
@pytest.mark.parametrize("permuted", [False, True], ids=["input order", "permuted"])
def test_view_scores(permuted, pattern):
    """test_gpu_view_selection._assert_same on score_sum and shared (the kernel's upper triangles) against pair_scores; both
    outputs and the tile counters start as pattern: the call clears them."""
    pts, cams, _, vis, mask = view_case(True)
    score, shared = VR.pair_scores(pts, vis, cams)
    a = arena(pattern)
    order = put(a, "order", np.random.RandomState(4).permutation(len(pts)).astype(np.int32), I32) if permuted else None
    p = dict(xyz=put(a, "xyz", pts), n=len(pts), order=order, mask=put(a, "mask", mask.view(np.int64), I64), words=1,
             centres=put(a, "centres", SV.camera_centres(cams)), V=5, table=put(a, "table", SV.weight_table().view(np.int16), I16),
             score=out(a, "score_sum", 5, 5, dtype=I64), shared=out(a, "shared", 5, 5, dtype=I64))
    wsb = size("mvs_view_scores_workspace_bytes", len(pts), 5)
    p.update(ws=a.take_bytes(wsb, name="tile counters"), wsb=wsb)
    run(a, "mvs_view_scores_f32", p, [p["score"], p["shared"]])
    got_s, got_n = n(p["score"]), n(p["shared"])
    a.check()
    assert shared[np.triu_indices(5, 1)].min() > 0
    same_bytes(got_s, np.triu(score, 1), "score_sum")
    same_bytes(got_n, np.triu(shared, 1), "shared")


@functools.lru_cache(maxsize=None)
def hist_case():
    pts, cams, _, vis, mask = view_case(True)
    bits = VR.depths(pts, cams).view(np.uint32)                          # (n, V)
    V = vis.shape[1]
    h0 = np.stack([np.bincount(bits[vis[:, v], v] >> 16, minlength=65536) for v in range(V)]).astype(np.uint32)
    # per view the fullest high half and its upper neighbour (empty for some views: a histogram of zeros is an answer too)
    prefixes = np.stack([[int(h0[v].argmax()), int(h0[v].argmax()) + 1] for v in range(V)]).astype(np.int32)
    h1 = np.zeros((V, 2, 65536), np.uint32)
    for v in range(V):
        w = bits[vis[:, v], v]
        for j in range(2):
            h1[v, j] = np.bincount(w[(w >> 16) == prefixes[v, j]] & 0xFFFF, minlength=65536)
    return frozen(h0, prefixes, h1)


@both_patterns
@pytest.mark.parametrize("which", [0, 1], ids=["pass 0", "pass 1"])
def test_view_depth_hist(which, pattern):
    """The histograms view_selection_reference.radix_select builds (counts of the high halves, then of the low halves inside a
    prefix), byte for byte as test_gpu_view_selection compares; hist starts as pattern: the call clears it."""
    pts, cams, _, vis, mask = view_case(True)
    h0, prefixes, h1 = hist_case()
    a = arena(pattern, 16)
    p = dict(xyz=put(a, "xyz", pts), n=len(pts), proj=put(a, "proj", RN.projection_tables(cams)), V=5,
             mask=put(a, "mask", mask.view(np.int64), I64), words=1, which=which,
             prefixes=put(a, "prefixes", prefixes, I32) if which else None,
             hist=out(a, "hist", 5, 1 + which, 65536, dtype=I32))
    L.check(call("mvs_view_depth_hist_f32", p), "mvs_view_depth_hist_f32")
    got = n(p["hist"]).view(np.uint32)
    a.check()
    want = h1 if which else h0.reshape(5, 1, 65536)
    assert want.sum() > 1000
    same_bytes(got, want, "hist")


@both_patterns
def test_view_selection_refusals_leave_the_outputs_alone(pattern):
    pts, cams, z, vis, mask = view_case(True)
    a = arena(pattern)
    xyz = put(a, "xyz", pts)
    m = out(a, "mask", len(pts), 1, dtype=I64)
    p = visibility_args(a, xyz, cams, range(5), z, m, 1)
    refused(a, call("mvs_view_visibility_f32", p, md=-1.0), E_BADARG, [m], "visibility min_depth -1")
    refused(a, call("mvs_view_visibility_f32", p, ztol=0.5), E_BADARG, [m], "visibility z_tol 0.5")
    refused(a, call("mvs_view_visibility_f32", p, V=65), E_SHAPE, [m], "visibility 65 views in one word")
    refused(a, call("mvs_view_visibility_f32", p, H=(1 << 24) + 1), E_SHAPE, [m], "visibility H 2^24 + 1")
    s = dict(xyz=xyz, n=len(pts), order=None, mask=put(a, "mask in", mask.view(np.int64), I64), words=1,
             centres=put(a, "centres", SV.camera_centres(cams)), V=5, table=put(a, "table", SV.weight_table().view(np.int16), I16),
             score=out(a, "score_sum", 5, 5, dtype=I64), shared=out(a, "shared", 5, 5, dtype=I64))
    wsb = size("mvs_view_scores_workspace_bytes", len(pts), 5)
    s.update(ws=a.take_bytes(wsb, name="tile counters"), wsb=wsb)
    so = [s["score"], s["shared"], s["ws"]]
    refused(a, call("mvs_view_scores_f32", s, table=None), E_BADARG, so, "scores table NULL")
    refused(a, call("mvs_view_scores_f32", s, n=0), E_SHAPE, so, "scores n 0")
    refused(a, call("mvs_view_scores_f32", s, V=513), E_SHAPE, so, "scores 513 views")
    refused(a, call("mvs_view_scores_f32", s, wsb=wsb - 1), E_WORKSPACE, so, "scores")
    h = dict(xyz=xyz, n=len(pts), proj=p["proj"], V=5, mask=s["mask"], words=1, which=0, prefixes=None,
             hist=out(a, "hist", 5, 65536, dtype=I32))
    refused(a, call("mvs_view_depth_hist_f32", h, which=2), E_BADARG, [h["hist"]], "hist pass 2")
    refused(a, call("mvs_view_depth_hist_f32", h, which=1), E_BADARG, [h["hist"]], "hist pass 1 without prefixes")
    refused(a, call("mvs_view_depth_hist_f32", h, V=65), E_SHAPE, [h["hist"]], "hist 65 views in one word")
    assert size("mvs_view_scores_workspace_bytes", 0, 5) == 0 and size("mvs_view_scores_workspace_bytes", 10, 513) == 0
    a.check()


# ==== 5. tsdf and surface nets ================================================================================================
def volume_origin(dims):
    from tests.test_gpu_mesh import _origin
    return _origin(dims)


@functools.lru_cache(maxsize=None)
def tsdf_reference(dims, colour, views=(0, 1, 2, 3, 4)):
    """mesh_reference.integrate of the plane scene's views into a small volume that the plane Z = 4 passes through."""
    sc = M.scene("plane")
    sel = list(views)
    vol = M.new_volume(volume_origin(dims), M.SCENE_VOXEL, dims, M.SCENE_TRUNC, colour=colour)
    return M.integrate(vol, sc["depths"][sel], sc["probs"][sel], sc["cams"][sel], sc["images"][sel] if colour else None)


def volume_regions(a, dims, colour, tag=""):
    """sum, count (and the colour sums) as pattern, cleared inside the arena as the header asks of the caller."""
    nx, ny, nz = dims
    v = dict(sum=out(a, "sum" + tag, nz, ny, nx), count=out(a, "count" + tag, nz, ny, nx, dtype=I32),
             rgb_sum=out(a, "rgb_sum" + tag, nz, ny, nx, 3, dtype=I32) if colour else None,
             rgb_count=out(a, "rgb_count" + tag, nz, ny, nx, dtype=I32) if colour else None)
    return v


def clear_volume(v):
    for t in v.values():
        if t is not None:
            t.zero_()


def integrate_args(a, dims, vol, views, colour, tag="", ws=None):
    sc = M.scene("plane")
    sel = list(views)
    origin, voxel, dims, trunc = MESH.check_volume(volume_origin(dims), M.SCENE_VOXEL, dims, M.SCENE_TRUNC)
    V, H, W = sc["depths"][sel].shape
    im = put(a, "images" + tag, sc["images"][sel], U8) if colour else None
    p = dict(depth=put(a, "depth" + tag, sc["depths"][sel]), prob=put(a, "prob" + tag, sc["probs"][sel]), V=V, H=H, W=W,
             proj=put(a, "proj" + tag, RN.projection_tables(sc["cams"][sel])), images=im, ih=im.shape[1] if colour else 0,
             iw=im.shape[2] if colour else 0, origin=floats(*origin), voxel=voxel, nx=dims[0], ny=dims[1], nz=dims[2], trunc=trunc,
             prob_thr=0.8, flags=0, sum=vol["sum"], count=vol["count"], rgb_sum=vol["rgb_sum"] if colour else None,
             rgb_count=vol["rgb_count"] if colour else None)
    wsb = size("mvs_tsdf_integrate_workspace_bytes", V, H, W)
    assert wsb > 0
    p.update(ws=a.take_bytes(wsb, name="integrate workspace" + tag) if ws is None else ws, wsb=wsb)
    return p


def assert_volume(vol, want):
    """test_gpu_mesh._assert_state: every word of the sums equal."""
    for k in ("sum", "count", "rgb_sum", "rgb_count"):
        if want[k] is not None:
            same_bytes(n(vol[k]), want[k], k)


@both_patterns
@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("dims", [(24, 20, 12), (65, 9, 7), (1, 7, 7)])
def test_tsdf_integrate(dims, colour, pattern):
    a = arena(pattern)
    vol = volume_regions(a, dims, colour)
    p = integrate_args(a, dims, vol, range(5), colour)
    outs = [t for t in vol.values() if t is not None]
    refused(a, call("mvs_tsdf_integrate_f32", p, wsb=p["wsb"] - 1), E_WORKSPACE, outs, "integrate one byte short")
    clear_volume(vol)
    L.check(call("mvs_tsdf_integrate_f32", p), "mvs_tsdf_integrate_f32")
    want = tsdf_reference(dims, colour)
    assert (want["count"] > 0).mean() > 0.5
    assert_volume(vol, want)
    a.check()


@functools.lru_cache(maxsize=None)
def nets_volume(kind):
    if kind == "sphere":
        return M.analytic_sphere()
    return tsdf_reference({"plane": (24, 20, 12), "wide": (65, 9, 7), "flat": (1, 7, 7)}[kind], True)


@both_patterns
@pytest.mark.parametrize("spare", [0, 5], ids=["exact capacity", "spare capacity"])
@pytest.mark.parametrize("kind,min_count", [("plane", 1), ("plane", 3), ("wide", 1), ("sphere", 1), ("flat", 1)])
def test_surface_nets_count_scan_write(kind, min_count, spare, pattern):
    """test_gpu_mesh._assert_mesh against mesh_reference.extract; the two scans are torch's, as TsdfVolume.extract does them.
    With spare capacity, vertices / colours / faces beyond the totals keep the pattern."""
    from tests.test_gpu_mesh import _assert_mesh
    ref = nets_volume(kind)
    nx, ny, nz = ref["dims"]
    colour = ref["rgb_sum"] is not None
    nodes, cells = nx * ny * nz, max(nx - 1, 0) * max(ny - 1, 0) * max(nz - 1, 0)
    want = M.extract(ref, min_count)
    a = arena(pattern)
    vol = dict(sum=put(a, "sum", ref["sum"]), count=put(a, "count", ref["count"], I32),
               rgb_sum=put(a, "rgb_sum", ref["rgb_sum"].view(np.int32), I32) if colour else None,
               rgb_count=put(a, "rgb_count", ref["rgb_count"], I32) if colour else None)
    wsb = size("mvs_surface_nets_workspace_bytes", nx, ny, nz)
    ws = a.take_bytes(wsb, name="surface-nets workspace")
    c = dict(sum=vol["sum"], count=vol["count"], nx=nx, ny=ny, nz=nz, min_count=min_count, totals=out(a, "totals", 2, dtype=I32), ws=ws, wsb=wsb)
    run(a, "mvs_surface_nets_count_f32", c, [c["totals"], ws])
    Mv, Fv = (int(x) for x in n(c["totals"]))
    a.freeze(ws)                                                   # the write call takes what the count call left
    assert (Mv, Fv) == (len(want["vertices"]), len(want["faces"])) and (Mv > 0) == (kind != "flat")
    words = ws.view(I32)
    face_at = ((max(cells, 1) * 4 + 255) // 256 * 256) // 4
    same_bytes(n(words[:max(cells, 1)]) >> 1 & 1, want["active"].astype(np.int32) if cells else np.zeros(1, np.int32), "active bits")
    rank = put(a, "cell_rank", torch.cumsum(words[:max(cells, 1)] >> 1, 0, dtype=I32), I32)
    fend = put(a, "face_end", torch.cumsum(words[face_at:face_at + nodes], 0, dtype=I32), I32)
    capM, capF = Mv + spare, Fv + spare
    origin, voxel, _, _ = MESH.check_volume(ref["origin"], ref["voxel"], ref["dims"], ref["trunc"])
    w = dict(sum=vol["sum"], count=vol["count"], rgb_sum=vol["rgb_sum"], rgb_count=vol["rgb_count"], origin=floats(*origin), voxel=voxel,
             nx=nx, ny=ny, nz=nz, min_count=min_count, rank=rank, fend=fend, M=capM, F=capF,
             vertices=out(a, "vertices", capM, 3) if capM else None, colours=out(a, "colours", capM, 3, dtype=U8) if capM else None,
             faces=out(a, "faces", capF, 3, dtype=I32) if capF else None, ws=ws, wsb=wsb)
    outs = [w[k] for k in ("vertices", "colours", "faces") if w[k] is not None]
    run(a, "mvs_surface_nets_write_f32", w, outs)
    torch.cuda.synchronize()
    for t, cnt in ((w["vertices"], Mv), (w["colours"], Mv), (w["faces"], Fv)):
        if t is not None:
            assert a.is_pattern(t[cnt:]), "written beyond the totals"
    a.check()
    if Mv:
        _assert_mesh((n(w["vertices"][:Mv]), n(w["colours"][:Mv]), n(w["faces"][:Fv]) if capF else np.zeros((0, 3), np.int32)), want)


@both_patterns
def test_tsdf_refusals_leave_the_outputs_alone(pattern):
    dims = (5, 4, 3)
    a = arena(pattern)
    vol = volume_regions(a, dims, True)
    p = integrate_args(a, dims, vol, range(2), True)
    outs = [t for t in vol.values()] + [p["ws"]]
    refused(a, call("mvs_tsdf_integrate_f32", p, flags=1), E_BADARG, outs, "integrate flags 1")
    refused(a, call("mvs_tsdf_integrate_f32", p, rgb_sum=None), E_BADARG, outs, "integrate images without rgb_sum")
    refused(a, call("mvs_tsdf_integrate_f32", p, nx=2048, ny=2048, nz=2048), E_SHAPE, outs, "integrate 2^33 nodes")
    wsb = size("mvs_surface_nets_workspace_bytes", *dims)
    ws = a.take_bytes(wsb, name="surface-nets workspace")
    ref = M.new_volume(volume_origin(dims), M.SCENE_VOXEL, dims, M.SCENE_TRUNC)
    s_in, c_in = put(a, "sum in", ref["sum"]), put(a, "count in", ref["count"], I32)
    c = dict(sum=s_in, count=c_in, nx=5, ny=4, nz=3, min_count=1, totals=out(a, "totals", 2, dtype=I32), ws=ws, wsb=wsb)
    refused(a, call("mvs_surface_nets_count_f32", c, min_count=0), E_BADARG, [c["totals"], ws], "count min_count 0")
    refused(a, call("mvs_surface_nets_count_f32", c, nx=2048, ny=2048, nz=2048), E_SHAPE, [c["totals"], ws], "count 2^33 nodes")
    w = dict(sum=s_in, count=c_in, rgb_sum=None, rgb_count=None, origin=floats(0, 0, 0), voxel=0.05, nx=5, ny=4, nz=3, min_count=1,
             rank=c_in, fend=c_in, M=4, F=4, vertices=out(a, "vertices", 4, 3), colours=out(a, "colours", 4, 3, dtype=U8),
             faces=out(a, "faces", 4, 3, dtype=I32), ws=ws, wsb=wsb)
    wo = [w["vertices"], w["colours"], w["faces"], ws]
    refused(a, call("mvs_surface_nets_write_f32", w, M=-1), E_BADARG, wo, "write M -1")
    refused(a, call("mvs_surface_nets_write_f32", w, voxel=0.0), E_BADARG, wo, "write voxel 0")
    refused(a, call("mvs_surface_nets_write_f32", w, nx=2048, ny=2048, nz=2048), E_SHAPE, wo, "write 2^33 nodes")
    refused(a, call("mvs_surface_nets_write_f32", w, wsb=wsb - 1), E_WORKSPACE, wo, "write")
    assert size("mvs_tsdf_integrate_workspace_bytes", 0, 5, 7) == 0 and size("mvs_surface_nets_workspace_bytes", 2048, 2048, 2048) == 0
    a.check()


# ==== 6. raster ===============================================================================================================
@functools.lru_cache(maxsize=None)
def raster_case(name):
    """mixed: raster_reference.mixed_mesh in one 40 x 48 view (two boxes above 256 pixels, the rest small); sphere: uv_sphere in
    three of the scene's views; tiny: the aligned grid of three vertices a side at 6 x 8."""
    if name == "mixed":
        v, f = RR.mixed_mesh()
        cams, H, W = RR.pixel_cam(40, 48), 40, 48
    elif name == "sphere":
        v, f = RR.uv_sphere()
        cams, H, W = R.scene("sphere")["cams"][:3], 40, 48
    else:
        v, f = RR.aligned_grid(3)
        cams, H, W = RR.pixel_cam(6, 8), 6, 8
    return frozen(v, f, np.asarray(cams)) + (H, W) + (frozen(*RR.render(v, f, cams, H, W)[:2]),)


def raster_setup(a, v, f, cams, H, W, lp, qc, index=True, order=None, tag="", ws=None):
    V = len(cams)
    p = dict(vertices=put(a, "vertices" + tag, v), M=len(v), faces=put(a, "faces" + tag, f, I32), F=len(f),
             order=put(a, "order" + tag, order, I32) if order is not None else None, proj=put(a, "proj" + tag, RN.projection_tables(cams)),
             V=V, H=H, W=W, md=0.0, cull=0, lp=lp, qc=qc, depth=out(a, "depth" + tag, V, H, W),
             index=out(a, "index" + tag, V, H, W, dtype=I32) if index else None)
    wsb = size("mvs_raster_workspace_bytes", V, H, W, qc)
    assert wsb > 0
    p.update(ws=a.take_bytes(wsb, name="raster workspace" + tag) if ws is None else ws, wsb=wsb)
    return p, [x for x in (p["depth"], p["index"]) if x is not None]


# name: mesh, large_pixels, queue_capacity, index, permuted, pairs that ask for the queue (None: not counted)
RASTER_CASES = {
    "mixed, queue used": ("mixed", 256, 16, True, False, 2),
    "mixed, queue overflows": ("mixed", 0, 1, True, True, None),
    "mixed, no queue": ("mixed", 256, 0, True, False, None),
    "mixed, every box queued, no index": ("mixed", 0, 4096, False, True, None),
    "sphere in three views": ("sphere", 16, 64, True, False, None),
}


@both_patterns
@pytest.mark.parametrize("case", sorted(RASTER_CASES))
def test_raster_mesh(case, pattern):
    """test_gpu_raster._assert_same against raster_reference.render; neither the queue nor its overflow changes a byte
    (test_large_path_queue_and_overflow_never_change_a_byte), and the counter is what the call itself cleared and counted."""
    from tests.test_gpu_raster import _assert_same
    name, lp, qc, index, permuted, asked = RASTER_CASES[case]
    v, f, cams, H, W, want = raster_case(name)
    order = np.random.RandomState(6).permutation(len(f)).astype(np.int32) if permuted else None
    a = arena(pattern)
    p, outs = raster_setup(a, v, f, cams, H, W, lp, qc, index, order)
    run(a, "mvs_raster_mesh_f32", p, outs)
    depth = n(p["depth"])
    a.check()
    _assert_same((depth, n(p["index"]) if index else want[1].copy()), want)
    queued = int(n(p["ws"][:8]).view(np.uint64)[0])
    if asked is not None:
        assert queued == asked
    if "overflows" in case:
        assert queued > qc                                         # more pairs asked than the queue holds: the rest were drawn in place


@both_patterns
@pytest.mark.parametrize("channels", [1, 8])
def test_raster_interpolate(channels, pattern):
    """test_gpu_raster.test_interpolation_of_constants_world_positions_and_colours: the bits of raster_reference.interpolate,
    over the index map the mesh call wrote into the arena."""
    v, f, cams, H, W, want = raster_case("sphere")
    attr = np.concatenate([v, -v, np.full((len(v), 2), 3.0, np.float32)], 1)[:, :channels] if channels > 1 else np.ones((len(v), 1), np.float32)
    a = arena(pattern)
    p, outs = raster_setup(a, v, f, cams, H, W, 256, 16)
    L.check(call("mvs_raster_mesh_f32", p), "mvs_raster_mesh_f32")
    a.freeze(p["index"])
    q = dict(vertices=p["vertices"], M=p["M"], faces=p["faces"], F=p["F"], proj=p["proj"], V=3, H=H, W=W, md=0.0, index=p["index"],
             attr=put(a, "attr", attr), C=channels, out=out(a, "out", 3, H, W, channels))
    L.check(call("mvs_raster_interpolate_f32", q), "mvs_raster_interpolate_f32")
    got = n(q["out"])
    a.check()
    same_bytes(n(p["index"]), want[1], "index")
    ref = RR.interpolate(v, f, cams, H, W, want[1], attr)
    same_bytes(got, ref, "interpolated")
    if channels == 1:
        assert (got[want[1] >= 0] == 1.0).all() and (got[want[1] < 0] == 0.0).all()


@both_patterns
def test_raster_refusals_leave_the_outputs_alone(pattern):
    v, f, cams, H, W, want = raster_case("tiny")
    a = arena(pattern)
    p, outs = raster_setup(a, v, f, cams, H, W, 256, 16)
    outs = outs + [p["ws"]]
    refused(a, call("mvs_raster_mesh_f32", p, cull=2), E_BADARG, outs, "cull 2")
    refused(a, call("mvs_raster_mesh_f32", p, qc=-1), E_BADARG, outs, "queue_capacity -1")
    refused(a, call("mvs_raster_mesh_f32", p, H=(1 << 20) + 1), E_SHAPE, outs, "H 2^20 + 1")
    refused(a, call("mvs_raster_mesh_f32", p, qc=4096), E_WORKSPACE, outs, "a queue the workspace was not sized for")
    refused(a, call("mvs_raster_mesh_f32", p, wsb=p["wsb"] - 1), E_WORKSPACE, outs, "raster")
    L.check(call("mvs_raster_mesh_f32", p), "mvs_raster_mesh_f32")
    q = dict(vertices=p["vertices"], M=p["M"], faces=p["faces"], F=p["F"], proj=p["proj"], V=1, H=H, W=W, md=0.0, index=p["index"],
             attr=put(a, "attr", np.ones((len(v), 2), np.float32)), C=2, out=out(a, "out", 1, H, W, 2))
    refused(a, call("mvs_raster_interpolate_f32", q, C=9), E_BADARG, [q["out"]], "interpolate 9 channels")
    refused(a, call("mvs_raster_interpolate_f32", q, md=float("nan")), E_BADARG, [q["out"]], "interpolate min_depth NaN")
    refused(a, call("mvs_raster_interpolate_f32", q, V=1 << 12, H=1 << 10, W=1 << 10), E_SHAPE, [q["out"]], "interpolate 2^32 pixels")
    assert size("mvs_raster_workspace_bytes", 1, 6, 8, -1) == 0 and size("mvs_raster_workspace_bytes", 1, (1 << 20) + 1, 8, 0) == 0
    a.check()


# ==== 7. mesh components ======================================================================================================
@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """grid: the 12 x 12 grid of test_gpu_mesh_clean.test_invalid_faces_and_vertices_between_guard_words with its invalid faces and
    non-finite vertices, every fourth row of quads left out (three components); strip63 / 64 / 65: one strip of as many faces; lone:
    six vertices and no face; none: nothing."""
    rs = np.random.RandomState(8)
    if name == "grid":
        v, f = (x.copy() for x in MC.grid(12, gap=4))
        f[5], f[17], f[40], f[99] = [-1, 0, 1], [0, 1, len(v)], [3, 2 ** 31 - 1, 4], [-2 ** 31, 7, 8]
        v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
        v[3, 2], v[4, 2] = -0.0, 0.0
    elif name.startswith("strip"):
        v, f = MC.strip(int(name[5:]), 1)
    elif name == "lone":
        v, f = rs.rand(6, 3).astype(np.float32), np.zeros((0, 3), np.int32)
    else:
        v, f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    return frozen(v, c, f)


def opt(a, name, array, dtype):
    return put(a, name, array, dtype) if len(array) else None


def opt_out(a, name, rows, *cols, dtype):
    return out(a, name, rows, *cols, dtype=dtype) if rows else None


@both_patterns
@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("name", ["grid", "strip63", "strip64", "strip65", "lone", "none"])
def test_mesh_label_measure_mark_write(name, colour, pattern):
    """test_gpu_mesh_clean._assert_components and _assert_clean piece by piece, against mesh_clean_reference: labels, counts and
    boxes, the status words, the keep flags, and the compacted mesh with the prefix sums done in torch as clean_device does."""
    v, c, f = mesh_case(name)
    Mv, Fv = len(v), len(f)
    comp = MC.components(v, f)
    a = arena(pattern)
    tv, tf = opt(a, "vertices", v, F32), opt(a, "faces", f, I32)
    wsb = size("mvs_mesh_components_workspace_bytes", Mv, Fv)
    ws = a.take_bytes(wsb, name="components workspace")
    lab = dict(vertices=tv, M=Mv, faces=tf, F=Fv, vl=opt_out(a, "vertex_labels", Mv, dtype=I32), fl=opt_out(a, "face_labels", Fv, dtype=I32),
               ws=ws, wsb=wsb)
    run(a, "mvs_mesh_components_label_i32", lab, [x for x in (lab["vl"], lab["fl"]) if x is not None])
    a.check()
    if Mv:
        same_bytes(n(lab["vl"]), comp["vertex_labels"], "vertex_labels")
    if Fv:
        same_bytes(n(lab["fl"]), comp["face_labels"], "face_labels")
    assert [int(x) for x in n(ws[:8]).view(np.int32)] == [0, comp["invalid"]]
    mea = dict(vertices=tv, M=Mv, F=Fv, vl=lab["vl"], fl=lab["fl"], counts=opt_out(a, "counts", Mv, dtype=I32),
               boxes=opt_out(a, "boxes", Mv, 6, dtype=I32), ws=ws, wsb=wsb)
    if Mv:
        a.freeze(lab["vl"])
    if Fv:
        a.freeze(lab["fl"])
    run(a, "mvs_mesh_components_measure_f32", mea, [x for x in (mea["counts"], mea["boxes"]) if x is not None])
    a.check()
    assert [int(x) for x in n(ws[:12]).view(np.int32)] == [0, comp["invalid"], comp["unreferenced"]]
    if Mv:
        counts, u = n(mea["counts"]), n(mea["boxes"])
        want = np.zeros(Mv, np.int32)
        want[comp["labels"]] = comp["faces"]
        same_bytes(counts, want, "counts")
        box = np.where(u < 0, u ^ np.int32(-2 ** 31), ~u).view(np.float32)      # the ordered image back to the float's bits
        assert np.array_equal(box[comp["labels"], :3], comp["lo"]) and np.array_equal(box[comp["labels"], 3:], comp["hi"])
        rest = np.ones(Mv, bool)
        rest[comp["labels"]] = False
        assert (u[rest, :3] == -1).all() and (u[rest, 3:] == 0).all()
    # keep the two largest components, as clean(keep_largest=2) selects them (the grid has three)
    keep = MC.select(comp, keep_largest=2)
    keep_label = np.zeros(Mv, np.int32)
    keep_label[comp["labels"][keep]] = 1
    mark = dict(faces=tf, M=Mv, F=Fv, fl=lab["fl"], keep_label=opt(a, "keep_label", keep_label, I32),
                face_keep=opt_out(a, "face_keep", Fv, dtype=I32), vertex_keep=opt_out(a, "vertex_keep", Mv, dtype=I32))
    L.check(call("mvs_mesh_compact_mark_i32", mark), "mvs_mesh_compact_mark_i32")
    wv, wc, wf, rep = MC.clean(v, c if colour else None, f, keep_largest=2)
    fk = np.isin(comp["face_labels"], comp["labels"][keep]) & (comp["face_labels"] >= 0)
    vk = np.zeros(Mv, bool)
    vk[f[fk].reshape(-1)] = True
    if Fv:
        same_bytes(n(mark["face_keep"]), fk.astype(np.int32), "face_keep")
    if Mv:
        same_bytes(n(mark["vertex_keep"]), vk.astype(np.int32), "vertex_keep")
    a.check()
    frank = put(a, "face_rank", torch.cumsum(mark["face_keep"], 0, dtype=I32), I32) if Fv else None
    vrank = put(a, "vertex_rank", torch.cumsum(mark["vertex_keep"], 0, dtype=I32), I32) if Mv else None
    Mo, Fo = int(vk.sum()), int(fk.sum())
    assert (Mo, Fo) == (len(wv), len(wf)) and (name in ("lone", "none")) == (Mo == 0)
    capM, capF = min(Mo + 3, Mv), min(Fo + 3, Fv)                  # more room than needed where the header allows it (M_out <= M)
    wr = dict(vertices=tv, colours=opt(a, "colours", c, U8) if colour else None, M=Mv, faces=tf, F=Fv, face_keep=mark["face_keep"],
              face_rank=frank, vertex_keep=mark["vertex_keep"], vertex_rank=vrank, M_out=capM, F_out=capF,
              ov=opt_out(a, "out_vertices", capM, 3, dtype=F32), oc=opt_out(a, "out_colours", capM, 3, dtype=U8) if colour else None,
              of=opt_out(a, "out_faces", capF, 3, dtype=I32))
    L.check(call("mvs_mesh_compact_write_f32", wr), "mvs_mesh_compact_write_f32")
    torch.cuda.synchronize()
    a.check()
    for t, cnt in ((wr["ov"], Mo), (wr["oc"], Mo), (wr["of"], Fo)):
        if t is not None:
            assert a.is_pattern(t[cnt:]), "written beyond the kept count"
    if Mo:
        assert n(wr["ov"][:Mo]).tobytes() == wv.tobytes() and n(wr["of"][:Fo]).tobytes() == wf.tobytes()
        assert not colour or n(wr["oc"][:Mo]).tobytes() == wc.tobytes()
    assert rep["components_kept"] == int(keep.sum()) and (name != "grid" or (rep["invalid_faces"] > 4 and rep["components"] == 3 and Mo < Mv))


@both_patterns
def test_mesh_refusals_leave_the_outputs_alone(pattern):
    v, c, f = mesh_case("strip63")
    Mv, Fv = len(v), len(f)
    a = arena(pattern)
    tv, tf = put(a, "vertices", v), put(a, "faces", f, I32)
    wsb = size("mvs_mesh_components_workspace_bytes", Mv, Fv)
    o = [out(a, "out%d" % k, 8 * Mv, dtype=I32) for k in range(6)] + [a.take_bytes(wsb, name="components workspace")]
    lab = dict(vertices=tv, M=Mv, faces=tf, F=Fv, vl=o[0], fl=o[1], ws=o[6], wsb=wsb)
    refused(a, call("mvs_mesh_components_label_i32", lab, M=-1), E_BADARG, o, "label M -1")
    refused(a, call("mvs_mesh_components_label_i32", lab, faces=None), E_BADARG, o, "label faces NULL")
    refused(a, call("mvs_mesh_components_label_i32", lab, F=2 ** 31), E_SHAPE, o, "label F 2^31")
    refused(a, call("mvs_mesh_components_label_i32", lab, wsb=wsb - 1), E_WORKSPACE, o, "label")
    mea = dict(vertices=tv, M=Mv, F=Fv, vl=o[0], fl=o[1], counts=o[2], boxes=o[3], ws=o[6], wsb=wsb)
    refused(a, call("mvs_mesh_components_measure_f32", mea, counts=None), E_BADARG, o, "measure counts NULL")
    refused(a, call("mvs_mesh_components_measure_f32", mea, M=2 ** 31), E_SHAPE, o, "measure M 2^31")
    refused(a, call("mvs_mesh_components_measure_f32", mea, wsb=wsb - 1), E_WORKSPACE, o, "measure")
    mark = dict(faces=tf, M=Mv, F=Fv, fl=o[1], keep_label=o[0], face_keep=o[4], vertex_keep=o[5])
    refused(a, call("mvs_mesh_compact_mark_i32", mark, keep_label=None), E_BADARG, o, "mark keep_label NULL")
    refused(a, call("mvs_mesh_compact_mark_i32", mark, M=2 ** 31), E_SHAPE, o, "mark M 2^31")
    wr = dict(vertices=tv, colours=None, M=Mv, faces=tf, F=Fv, face_keep=o[4], face_rank=o[4], vertex_keep=o[5], vertex_rank=o[5],
              M_out=Mv + 1, F_out=1, ov=o[2], oc=None, of=o[3])
    refused(a, call("mvs_mesh_compact_write_f32", wr), E_BADARG, o, "write M_out above M")
    refused(a, call("mvs_mesh_compact_write_f32", wr, M_out=1, ov=None), E_BADARG, o, "write out_vertices NULL")
    refused(a, call("mvs_mesh_compact_write_f32", wr, M_out=1, F=2 ** 31), E_SHAPE, o, "write F 2^31")
    assert size("mvs_mesh_components_workspace_bytes", -1, 0) == 0 and size("mvs_mesh_components_workspace_bytes", 2 ** 31, 0) == 0
    a.check()


# ==== 8. calls that follow each other =========================================================================================
@both_patterns
def test_fusion_small_large_small_through_one_workspace(pattern):
    """Two different inputs back to back and a larger shape between two runs of a smaller one, one workspace (the larger's
    size); the two small runs give equal bytes.  The second small run goes to a side stream."""
    small, large = fusion_scene("tiny"), fusion_scene("kat")
    a = arena(pattern)
    fn, big, _ = fusion_setup(a, large, N=2, dedupe=True, normals=True, tag=" large")
    runs = []
    for k in range(2):
        fn, p, _ = fusion_setup(a, small, N=1, dedupe=True, normals=True, tag=" small %d" % k)
        assert p["wsb"] < big["wsb"]
        p.update(ws=big["ws"], wsb=big["wsb"])
        runs.append(p)
    L.check(call(fn, runs[0]), fn)
    L.check(call(fn, big), fn)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.check(call(fn, runs[1]), fn)
    side.synchronize()
    r0, r1, rb = fusion_result(a, runs[0]), fusion_result(a, runs[1]), fusion_result(a, big)
    a.check()
    for k in r0:
        same_bytes(r0[k], r1[k], k)
    fusion_compare(small, fusion_reference("tiny", 1, True, None, True, True), r0, True)
    fusion_compare(large, fusion_reference("kat", 2, True, None, True, True), rb, True)


@both_patterns
def test_nearest_and_voxel_select_small_large_small(pattern):
    from tests.test_gpu_pointcloud_eval import _check_against_reference
    a = arena(pattern)
    qs, ts, cs, ms = nn_case("1023 on 1, one cell")
    ql, tl, cl, ml = nn_case("3000 on 4000")
    big = nn_setup(a, ql, tl, grid_of(tl, ml, cl), ml, " large")
    smalls = []
    for k in range(2):
        p = nn_setup(a, qs, ts, grid_of(ts, ms, cs), ms, " small %d" % k)
        p.update(ws=big["ws"], wsb=big["wsb"])
        smalls.append(p)
    L.check(call("mvs_nn_f32", smalls[0]), "mvs_nn_f32")
    L.check(call("mvs_nn_f32", big), "mvs_nn_f32")
    L.check(call("mvs_nn_f32", smalls[1]), "mvs_nn_f32")
    for k in ("dist", "index"):
        same_bytes(n(smalls[0][k]), n(smalls[1][k]), k)
    a.check()
    _check_against_reference(qs, ts, ms, n(smalls[0]["dist"]), n(smalls[0]["index"]).astype(np.int64))
    _check_against_reference(ql, tl, ml, n(big["dist"]), n(big["index"]).astype(np.int64))
    # statistics of the two distance arrays through one workspace
    wsb = size("mvs_dist_stats_workspace_bytes", 3000, 2)
    ws = a.take_bytes(wsb, name="stats workspace")
    outs = []
    for p, md in ((smalls[0], ms), (big, ml), (smalls[1], ms)):
        o = out(a, "stats %d" % len(outs), 4, dtype=F64)
        L.check(call("mvs_dist_stats_f32", dict(dist=p["dist"], n=p["nq"], md=md, thr=floats(0.4 * md, md), nthr=2, out=o, ws=ws, wsb=wsb)),
                "mvs_dist_stats_f32")
        outs.append(n(o))
    a.check()
    same_bytes(outs[0], outs[2], "stats")
    d = n(big["dist"])
    assert outs[1][1] == (d < np.float32(ml)).sum() and outs[1][2] == (d < np.float32(0.4 * ml)).sum()


@both_patterns
def test_tsdf_views_in_two_calls_equal_one_call(pattern):
    """test_gpu_mesh.test_two_calls_equal_one_call inside the arena: views 0..2 then 3..4 through one workspace, equal to one call
    of 0..4 and to mesh_reference.integrate.  Both volumes are cleared by the test."""
    dims = (24, 20, 12)
    a = arena(pattern)
    one, two = volume_regions(a, dims, True, " one"), volume_regions(a, dims, True, " two")
    clear_volume(one)
    clear_volume(two)
    whole = integrate_args(a, dims, one, range(5), True, " 0..4")
    L.check(call("mvs_tsdf_integrate_f32", whole), "mvs_tsdf_integrate_f32")
    first = integrate_args(a, dims, two, (0, 1, 2), True, " 0..2", ws=whole["ws"])
    second = integrate_args(a, dims, two, (3, 4), True, " 3..4", ws=whole["ws"])
    L.check(call("mvs_tsdf_integrate_f32", first), "mvs_tsdf_integrate_f32")
    L.check(call("mvs_tsdf_integrate_f32", second), "mvs_tsdf_integrate_f32")
    want = tsdf_reference(dims, True)
    assert_volume(one, want)
    assert_volume(two, want)
    a.check()


@both_patterns
def test_two_visibility_calls_set_different_bits_of_one_mask(pattern):
    """Views 0..2 at bits 0..2, then views 3 and 4 at bits 3 and 70 of a two-word mask the test cleared once; a bit position
    outside the mask (200) is left out."""
    pts, cams, z, vis, _ = view_case(True)
    a = arena(pattern)
    xyz = put(a, "xyz", pts)
    mask = out(a, "mask", len(pts), 2, dtype=I64)
    mask.zero_()
    L.check(call("mvs_view_visibility_f32", visibility_args(a, xyz, cams[:3], [0, 1, 2], z[:3], mask, 2, tag=" a")), "mvs_view_visibility_f32")
    L.check(call("mvs_view_visibility_f32", visibility_args(a, xyz, cams[3:], [3, 70], z[3:], mask, 2, tag=" b")), "mvs_view_visibility_f32")
    L.check(call("mvs_view_visibility_f32", visibility_args(a, xyz, cams[:1], [200], z[:1], mask, 2, tag=" c")), "mvs_view_visibility_f32")
    got = n(mask).view(np.uint64)
    a.check()
    want = np.zeros((len(pts), 2), np.uint64)
    for v, bit in enumerate([0, 1, 2, 3, 70]):
        want[:, bit // 64] |= vis[:, v].astype(np.uint64) << np.uint64(bit % 64)
    same_bytes(got, want, "mask")


@both_patterns
def test_render_and_raster_twice_with_another_input_between(pattern):
    """Each of the two z-buffer calls run twice into one workspace with a different cloud / mesh in between, the last run on a
    side stream: the workspace's keys, raw map, counter and queue are the call's to clear."""
    from tests.test_gpu_render import _assert_same
    a = arena(pattern)
    pts = R.scene_cloud()[0]
    occ = (1, 0.1, 2)
    r0, _ = render_setup(a, pts[::2], cloud_cams(40, 48), 40, 48, 0, occ, True, None, " a")
    r1, _ = render_setup(a, pts, cloud_cams(40, 48), 40, 48, 1, occ, True, None, " b", ws=r0["ws"])
    r2, _ = render_setup(a, pts[::2], cloud_cams(40, 48), 40, 48, 0, occ, True, None, " c", ws=r0["ws"])
    v, f, cams, H, W, want = raster_case("mixed")
    sv, sf, scams, _, _, swant = raster_case("sphere")
    m1, _ = raster_setup(a, sv, sf, scams, 40, 48, 16, 64, tag=" b")
    m0, _ = raster_setup(a, v, f, cams, H, W, 0, 8, tag=" a", ws=m1["ws"])
    m2, _ = raster_setup(a, v, f, cams, H, W, 0, 8, tag=" c", ws=m1["ws"])
    assert m0["wsb"] < m1["wsb"]
    for p in (r0, r1):
        L.check(call("mvs_render_points_f32", p), "mvs_render_points_f32")
    for p in (m0, m1):
        L.check(call("mvs_raster_mesh_f32", p), "mvs_raster_mesh_f32")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        L.check(call("mvs_render_points_f32", r2), "mvs_render_points_f32")
        L.check(call("mvs_raster_mesh_f32", m2), "mvs_raster_mesh_f32")
    side.synchronize()
    a.check()
    for x, y in ((r0, r2), (m0, m2)):
        same_bytes(n(x["depth"]), n(y["depth"]), "depth")
        same_bytes(n(x["index"]), n(y["index"]), "index")
    _assert_same((n(r0["depth"]), n(r0["index"])), render_reference(40, 48, 2, 0, occ))
    _assert_same((n(r1["depth"]), n(r1["index"])), render_reference(40, 48, 1, 1, occ))
    _assert_same((n(m0["depth"]), n(m0["index"])), want)
    _assert_same((n(m1["depth"]), n(m1["index"])), swant)


@both_patterns
def test_components_of_two_meshes_through_one_workspace(pattern):
    """Label and measure of a strip, of the larger grid, and of the strip again through the grid's workspace: equal bytes, and the
    status words are each call's own."""
    a = arena(pattern)
    gv, _, gf = mesh_case("grid")
    sv, _, sf = mesh_case("strip65")
    wsb = size("mvs_mesh_components_workspace_bytes", len(gv), len(gf))
    ws = a.take_bytes(wsb, name="components workspace")
    runs = []
    for k, (v, f) in enumerate(((sv, sf), (gv, gf), (sv, sf))):
        Mv, Fv = len(v), len(f)
        assert size("mvs_mesh_components_workspace_bytes", Mv, Fv) <= wsb
        tv = put(a, "vertices %d" % k, v)
        lab = dict(vertices=tv, M=Mv, faces=put(a, "faces %d" % k, f, I32), F=Fv, vl=out(a, "vertex_labels %d" % k, Mv, dtype=I32),
                   fl=out(a, "face_labels %d" % k, Fv, dtype=I32), ws=ws, wsb=wsb)
        L.check(call("mvs_mesh_components_label_i32", lab), "mvs_mesh_components_label_i32")
        mea = dict(vertices=tv, M=Mv, F=Fv, vl=lab["vl"], fl=lab["fl"], counts=out(a, "counts %d" % k, Mv, dtype=I32),
                   boxes=out(a, "boxes %d" % k, Mv, 6, dtype=I32), ws=ws, wsb=wsb)
        L.check(call("mvs_mesh_components_measure_f32", mea), "mvs_mesh_components_measure_f32")
        comp = MC.components(v, f)
        assert [int(x) for x in n(ws[:12]).view(np.int32)] == [0, comp["invalid"], comp["unreferenced"]]
        same_bytes(n(lab["vl"]), comp["vertex_labels"], "vertex_labels")
        same_bytes(n(lab["fl"]), comp["face_labels"], "face_labels")
        runs.append([n(x) for x in (lab["vl"], lab["fl"], mea["counts"], mea["boxes"])])
    a.check()
    for x, y in zip(runs[0], runs[2]):
        same_bytes(x, y, "strip again")


# ==== 9. every geometry entry point has a case here ===========================================================================
def test_every_geometry_entry_point_is_called_here():
    """The names from mvs_fusion_workspace_bytes to the end of _lib.SIGNATURES (the header's order) against the names this file
    passes to call() and size(): a later entry point cannot be added without an arena case."""
    names = list(L.SIGNATURES)
    declared = set(names[names.index("mvs_fusion_workspace_bytes"):])
    with open(os.path.abspath(__file__).replace(".pyc", ".py")) as fh:
        text = fh.read()
    called = set(re.findall(r"\"(mvs_[a-z0-9_]+)\"", text))
    assert declared - called == set(), "no arena case calls %s" % sorted(declared - called)
    assert len(declared) == 36
