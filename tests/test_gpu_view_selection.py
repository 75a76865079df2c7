"""GPU tests of the view selection (csrc/view_selection.hip through mvsnet_amd.select_views) against the float32 restatement
of tests/view_selection_reference.py, byte for byte: the visibility mask in every mode, the pair matrices from one mask word
to several tiles and in any processing order, sums beyond 32 bits, clouds beyond one launch of the pair kernel, degenerate
inputs, the exact depth percentiles, the C ABI's argument checks and the command line end to end."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_reference as F
from tests import render_reference as R
from tests import view_selection_reference as VR
from tests._helpers import make_session

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"40x48": (40, 48), "37x53": (37, 53)}
MODES = {"frustum": dict(),
         "zbuffer": dict(visibility="zbuffer"),
         "zbuffer splat 1": dict(visibility="zbuffer", splat=1),
         "zbuffer occlusion": dict(visibility="zbuffer", occlusion=(1, 0.1, 2)),
         "min_depth": dict(min_depth=4.5)}


def _reference(points, cams, sizes, visibility="frustum", z_rel=0.01, splat=0, occlusion=None, min_depth=0.0, percentiles=(1, 99),
               table=None):
    """The restatement's answer for views of the given sizes (one (H, W) per view), grouped by size as the plan groups them."""
    points, cams = np.asarray(points, np.float32), np.asarray(cams, np.float64)
    vis = np.zeros((len(points), len(cams)), bool)
    for size in dict.fromkeys(sizes):
        members = [v for v, s in enumerate(sizes) if s == size]
        z = VR.zbuffer(points, cams[members], size[0], size[1], splat, occlusion, min_depth) if visibility == "zbuffer" else None
        vis[:, members] = VR.visibility(points, cams[members], size[0], size[1], min_depth, z, z_rel)
    score, shared = VR.pair_scores(points, vis, cams, table)
    ranges = VR.depth_ranges(points, vis, cams, *percentiles)
    return dict(mask=VR.pack_mask(vis), visible=vis.sum(0).astype(np.int64), score_sum=score, shared=shared,
                min_depth=ranges[:, 0].copy(), max_depth=ranges[:, 1].copy())


def _device(points, cams, sizes, run=None, **kw):
    from mvsnet_amd import select_views as S
    plan = S.ViewSelectionPlan(points, [(v, cams[v], sizes[v]) for v in range(len(cams))], **kw)
    return plan, {k: t.cpu().numpy() for k, t in plan.run(**(run or {})).items()}


def _assert_same(got, want):
    assert got["mask"].dtype == np.int64 and got["visible"].dtype == np.int64 and got["min_depth"].dtype == np.float32
    assert got["score_sum"].dtype == np.int64 and got["shared"].dtype == np.int64
    diff = {k: int((np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)).sum())
            if got[k].shape == want[k].shape else -1 for k in want}
    print("bytes that differ:", diff)
    assert not any(diff.values()), diff


@functools.lru_cache(maxsize=None)
def _scene_reference(size, mode):
    return _reference(R.scene_cloud()[0], VR.scene_cams(SIZES[size]), [SIZES[size]] * 5, **MODES[mode])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", list(SIZES))
def test_five_view_scene_equals_the_float32_reference(size, mode):
    want = _scene_reference(size, mode)
    assert want["visible"].min() > 0
    if mode != "frustum":
        assert (want["visible"] < _scene_reference(size, "frustum")["visible"]).all()
    _, got = _device(R.scene_cloud()[0], VR.scene_cams(SIZES[size]), [SIZES[size]] * 5, **MODES[mode])
    _assert_same(got, want)


@pytest.mark.parametrize("mode", ["frustum", "zbuffer splat 1"])
def test_two_size_groups_in_one_plan(mode):
    sizes = [SIZES["40x48"], SIZES["37x53"]] * 2 + [SIZES["40x48"]]
    cams = np.stack([VR.scene_cams(sizes[v])[v] for v in range(5)])
    plan, got = _device(R.scene_cloud()[0], cams, sizes, **MODES[mode])
    assert [m for _, m in plan.groups] == [[0, 2, 4], [1, 3]]
    _assert_same(got, _reference(R.scene_cloud()[0], cams, sizes, **MODES[mode]))


@functools.lru_cache(maxsize=None)
def _ring(V, n):
    pts = R.scene_cloud()[0][np.sort(np.random.RandomState(V).choice(9600, n, replace=False))]
    cams = VR.ring_cameras(V)
    return pts, cams, _reference(pts, cams, [(40, 48)] * V)


@pytest.mark.parametrize("V,n", [(37, 2000), (64, 500), (65, 500), (70, 2000), (200, 600)])
def test_pair_matrices_on_a_ring_of_cameras(V, n):
    """37: one mask word; 64 / 65: the word boundary itself; 70: two words, pairs inside either and across; 200: four words,
    ten tiles, diagonal and off-diagonal, the last word partly filled."""
    import torch
    pts, cams, want = _ring(V, n)
    per_point = np.array([bin(int(w)).count("1") for w in want["mask"].reshape(-1)]).reshape(n, -1).sum(1)
    print("views per point: min %d median %d max %d; pairs with a score %d of %d" %
          (per_point.min(), np.median(per_point), per_point.max(), (want["score_sum"] > 0).sum() // 2, V * (V - 1) // 2))
    assert per_point.max() > V // 4 and (want["shared"] > 0).sum() > V
    plan, got = _device(pts, cams, [(40, 48)] * V)
    _assert_same(got, want)
    assert plan.order is not None and sorted(plan.order.cpu().tolist()) == list(range(n))
    reverse = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=plan.dev)
    for order in (None, reverse, "plan"):                                      # the plan's order again: two runs, same bytes
        again = {k: t.cpu().numpy() for k, t in plan.run(order=order).items()}
        _assert_same(again, want)


def _looking_at(point, angles_deg, distance=4.0, H=40, W=48, f=40.0):
    """Cameras in the x-z plane around `point`, at the given angles as seen from it, looking at it."""
    point = np.asarray(point, np.float64)
    cams = np.zeros((len(angles_deg), 2, 4, 4))
    for i, a in enumerate(np.radians(angles_deg)):
        C = point + distance * np.array([np.sin(a), 0.0, -np.cos(a)])
        Rm = F._look_at(C, point)
        cams[i, 0, :3, :3], cams[i, 0, :3, 3], cams[i, 0, 3, 3] = Rm, -Rm @ C, 1.0
        cams[i, 1, :3, :3] = [[f, 0, W / 2.0 + 0.1371], [0, f, H / 2.0 - 0.0613], [0, 0, 1.0]]
    return cams


@pytest.mark.parametrize("copies,order", [(70000, "voxel"), ((1 << 23) + 37, None)])
def test_copies_of_one_point_sum_beyond_32_bits(copies, order):
    """70 000 copies: 70 000 x 65 535 > 2^32 in one accumulator.  2^23 + 37 copies: more than one launch of the pair kernel
    takes.  The restatement of one point times the number of copies is the answer."""
    point = np.float32([[0.25, -0.125, 4.0]])
    cams = _looking_at(point[0], [0.0, 5.0, 40.0])
    one = _reference(point, cams, [(40, 48)] * 3)
    assert one["visible"].tolist() == [1, 1, 1] and one["score_sum"][0, 1] > 65000 and one["score_sum"][0, 2] > 0
    assert one["score_sum"][0, 1] * copies > 2 ** 32
    _, got = _device(np.tile(point, (copies, 1)), cams, [(40, 48)] * 3, order=order)
    assert (got["mask"] == 7).all()
    assert np.array_equal(got["visible"], one["visible"] * copies)
    assert np.array_equal(got["score_sum"], one["score_sum"] * copies) and np.array_equal(got["shared"], one["shared"] * copies)
    assert np.array_equal(got["min_depth"], one["min_depth"]) and np.array_equal(got["max_depth"], one["max_depth"])


def test_degenerate_inputs():
    cams = VR.scene_cams((40, 48))
    sizes = [(40, 48)] * 5
    cloud = R.scene_cloud()[0]
    centres = VR.camera_centres(cams)
    for pts in (cloud[:1], centres[:1]):                                       # n = 1; a point at a camera centre, alone
        _assert_same(_device(pts, cams, sizes)[1], _reference(pts, cams, sizes))
    nan, inf = float("nan"), float("inf")
    junk = np.array([[nan, 0, 4], [0, inf, 4], [0, 0, -inf], [1e38, 1e38, 4.0], [1e30, -1e30, 4.0], [nan, nan, nan]], np.float32)
    behind = np.float32([[0, 0, -50.0], [1, 1, -60.0]])                        # behind every camera of the arc
    mixed = np.concatenate([junk, centres, behind, cloud[::7]])
    want = _reference(mixed, cams, sizes)
    assert not want["mask"][:len(junk)].any() and not want["mask"][len(junk) + 5:len(junk) + 7].any()
    for order in ("voxel", None):
        _assert_same(_device(mixed, cams, sizes, order=order)[1], want)
    _assert_same(_device(np.concatenate([junk, behind]), cams, sizes, order=None)[1],
                 _reference(np.concatenate([junk, behind]), cams, sizes))
    # a view that sees nothing: the camera turned away
    away = np.array(cams)
    away[3, 0, :3, :] = np.diag([-1.0, 1.0, -1.0]) @ away[3, 0, :3, :]
    want = _reference(cloud, away, sizes)
    assert want["visible"][3] == 0 and not want["score_sum"][3].any() and want["min_depth"][3] == 0 == want["max_depth"][3]
    _assert_same(_device(cloud, away, sizes)[1], want)
    # V = 1: empty matrices
    want = _reference(cloud, cams[:1], sizes[:1])
    assert want["score_sum"].shape == (1, 1)
    _assert_same(_device(cloud, cams[:1], sizes[:1])[1], want)


def test_pair_kernel_on_a_hand_made_mask():
    """Every bit of every word set, the bits past V too: the pair kernel reads only the V views, a point at a camera centre
    counts as shared and contributes 0, an obtuse pair contributes 0, and the 3-4-5 pair contributes T[4915] = 408."""
    from mvsnet_amd import select_views as S
    centres = np.float32([[5, 0, 0], [4, 3, 0], [-4, 3, 0]])
    cams = np.zeros((3, 2, 4, 4))
    cams[:, 0], cams[:, 1, :3, :3] = np.eye(4), np.eye(3)
    cams[:, 0, :3, 3] = -centres
    pts = np.float32([[0, 0, 0], [5, 0, 0], [0.5, 7.0, -2.0], [4, 3, 0]])
    plan = S.ViewSelectionPlan(pts, cams=cams, size=(8, 8), order=None)
    plan.run()
    plan.mask.fill_(-1)
    plan.enqueue_scores()
    score, shared = VR.pair_scores(pts, np.ones((4, 3), bool), cams)
    got_score, got_shared = (t.cpu().numpy() for t in (plan.score_sum, plan.shared))
    assert np.array_equal(got_score, np.triu(score)) and np.array_equal(got_shared, np.triu(shared))
    assert shared[0, 1] == 4 and score[0, 2] == VR.pair_terms(centres[0] - pts[2], centres[2] - pts[2], S.weight_table())
    assert VR.pair_scores(pts[:1], np.ones((1, 3), bool), cams)[0][0, 1] == 408


def test_depth_percentiles_across_a_power_of_two_and_with_ties():
    cam = R.identity_cam(40, 48, 40.0)[None]
    rs = np.random.RandomState(2)
    for z in (np.linspace(1.5, 2.5, 1000), np.repeat([1.75, 2.0, 2.25], 50), np.float32(2.0) + np.arange(300) * np.float32(2.0 ** -22)):
        z = np.asarray(z, np.float32)[rs.permutation(len(z))]
        pts = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
        for pc in ((1, 99), (0, 100), (50, 50)):
            want = _reference(pts, cam, [(40, 48)], percentiles=pc)
            s = np.sort(z)
            assert want["min_depth"][0] == s[len(z) * pc[0] // 100] and want["visible"][0] == len(z)    # w is z itself here
            _assert_same(_device(pts, cam, [(40, 48)], percentiles=pc)[1], want)


def test_argument_checks_come_before_any_gpu_work():
    import torch
    from mvsnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, V = 4, 70
    xyz = torch.zeros((n, 3), device=dev)
    proj = torch.zeros(512 * 12, device=dev)
    bits = torch.zeros(513, dtype=torch.int32, device=dev)
    mask = torch.zeros((n, 9), dtype=torch.int64, device=dev)
    centres = torch.zeros(513 * 3, device=dev)
    table = torch.zeros(8192, dtype=torch.int16, device=dev)
    out = torch.full((513 * 513,), -7, dtype=torch.int64, device=dev)
    hist = torch.full((2 * 65536,), -7, dtype=torch.int32, device=dev)
    wsb = lib.mvs_view_scores_workspace_bytes(n, V)
    ws = torch.zeros(max(wsb, 256), dtype=torch.uint8, device=dev)
    p, st = _lib.ptr, _lib.stream_ptr()
    BADARG, SHAPE, WORKSPACE = -1, -2, -3
    assert wsb > 0 and lib.mvs_view_scores_workspace_bytes(n, 513) == 0 and lib.mvs_view_scores_workspace_bytes(0, V) == 0
    scores = lambda **k: lib.mvs_view_scores_f32(k.get("xyz", p(xyz)), k.get("n", n), None, p(mask), k.get("mw", 2), p(centres),
                                                 k.get("V", V), k.get("table", p(table)), p(out), p(out), p(ws), k.get("wsb", wsb), st)
    assert scores(V=513, mw=9) == SHAPE and scores(mw=1) == SHAPE and scores(n=0) == SHAPE
    assert scores(table=None) == BADARG and scores(xyz=None) == BADARG and scores(V=0) == BADARG
    assert scores(wsb=wsb - 1) == WORKSPACE and scores(wsb=0) == WORKSPACE
    vis = lambda **k: lib.mvs_view_visibility_f32(p(xyz), k.get("n", n), p(proj), k.get("bits", p(bits)), k.get("V", V), 8, 8,
                                                  k.get("min_depth", 0.0), None, 1.0, p(mask), k.get("mw", 2), st)
    assert vis(V=513, mw=9) == SHAPE and vis(mw=1) == SHAPE and vis(n=0) == SHAPE
    assert vis(bits=None) == BADARG and vis(min_depth=-1.0) == BADARG and vis(min_depth=float("nan")) == BADARG
    dh = lambda **k: lib.mvs_view_depth_hist_f32(p(xyz), k.get("n", n), p(proj), k.get("V", 1), p(mask), k.get("mw", 1),
                                                 k.get("which", 0), k.get("prefixes", None), k.get("hist", p(hist)), st)
    assert dh(V=513, mw=9) == SHAPE and dh(V=70, mw=1) == SHAPE and dh(n=0) == SHAPE
    assert dh(which=2) == BADARG and dh(which=1) == BADARG and dh(prefixes=p(bits)) == BADARG and dh(hist=None) == BADARG
    torch.cuda.synchronize()
    assert (out == -7).all() and (hist == -7).all() and not mask.any()         # nothing was cleared, nothing was written
    assert scores() == 0 and dh() == 0 and vis() == 0                          # the same calls with valid arguments run
    torch.cuda.synchronize()
    assert not out[:V * V].any() and (out[V * V:] == -7).all() and not hist[:65536].any() and (hist[65536:] == -7).all()


def test_command_line_writes_the_file_the_restatement_gives(tmp_path):
    from mvsnet_amd import fusion as Fu
    from mvsnet_amd import render as Rn
    from mvsnet_amd import select_views as S
    from mvsnet_amd.mvs_data_generation import make_generator
    session = make_session(str(tmp_path / "s"))
    out = os.path.join(session, "covisibility.json")
    os.remove(out)
    views = Rn.session_views(session)
    yy, xx = np.mgrid[0:48:0.5, 0:64:0.5]                                      # a plane at 600 mm, four points per pixel of view 0
    cloud = F._backproject(views[0][1], xx.reshape(-1), yy.reshape(-1), np.full(xx.size, 600.0)).astype(np.float32)
    ply = str(tmp_path / "g.ply")
    Fu.write_ply(ply, cloud, np.zeros((len(cloud), 3), np.uint8))
    cmd = [sys.executable, "-m", "mvsnet_amd.select_views", "--cloud", ply, "--session", session, "--num_views", "2",
           "--depth_percentiles", "2:98"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    want = _reference(cloud, np.stack([v[1] for v in views]), [v[2] for v in views], percentiles=(2, 98))
    assert report["points"] == len(cloud) and report["views"] == 4 and report["visible"] == want["visible"].tolist()
    nb = S.select_neighbours(want["score_sum"], want["shared"], num_views=2)
    expected = S.covisibility([v[0] for v in views], nb, want["score_sum"], want["shared"], want["min_depth"], want["max_depth"])
    written = open(out).read()
    assert json.loads(written) == expected and all(len(e["views"]) == 2 for e in expected.values())
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)      # the file exists now
    assert r.returncode != 0 and "--force" in r.stderr and "Traceback" not in r.stderr
    assert open(out).read() == written
    gen = make_generator(session, view_num=3, image_width=64, image_height=64, depth_num=8, base_image_size=8)
    assert [c.views for c in gen.clusters] == [expected[str(i)]["views"] for i in range(4)]
