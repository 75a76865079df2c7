"""GPU tests of the point-cloud evaluation (csrc/pointcloud.hip through mvsnet_amd.evaluate) against the float64 reference of
tests/pointcloud_reference.py: capped nearest neighbours on several cloud kinds, independence of the grid, metrics,
preprocessing, reproducibility and graph capture, the fusion end to end, both command lines, and cKDTree at 1M x 1M."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_reference as FR
from tests import pointcloud_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_nn(q, t, max_dist, cell=None):
    from mvsnet_amd import evaluate as E
    plan = E.NearestPlan(q, t, max_dist, cell=cell)
    plan.enqueue()
    return plan.result() + (plan.grid,)


def _tolerance(q, t, d_all):
    Rmax = max(float(np.abs(q).max()), float(np.abs(t).max()))
    return 1e-6 * (Rmax + np.where(np.isfinite(d_all), d_all, 0.0))


def _check_against_reference(q, t, max_dist, d, idx):
    rd, ri, d_all, gap = R.nearest(q, t, max_dist)
    tol = _tolerance(q, t, d_all)
    clear = (np.abs(d_all - max_dist) > tol) & (gap > tol)
    assert clear.mean() >= 0.999, clear.mean()
    assert np.array_equal(np.isfinite(d)[clear], np.isfinite(rd)[clear])
    assert np.array_equal(idx[clear], ri[clear])
    both = np.isfinite(d) & np.isfinite(rd)
    assert (np.abs(d[both] - d_all[both]) <= tol[both]).all(), np.abs(d[both] - d_all[both]).max()
    assert (idx[~np.isfinite(d)] == -1).all() and (idx[np.isfinite(d)] >= 0).all()
    return rd


def _kinds():
    base = R.plane_sphere(9000, extent=100.0, seed=1)
    surf_q = R.noisy(R.plane_sphere(7000, extent=100.0, seed=2), 0.3, seed=3)
    uni = R.uniform(1500, seed=4)
    dup = np.concatenate([uni, uni[::-1], uni])                              # every target point three times
    centres = [(0, 0, 0), (2e4, 0, 0), (0, 2e4, 0), (0, 0, 2e4), (2e4, 2e4, 2e4)]
    ct = R.clusters(8000, centres, 30.0, seed=5)
    cq = R.noisy(ct[::2], 0.02, seed=6)                                       # near copies: the nearest point is clear
    return {
        "uniform": (R.uniform(5000, seed=7), R.uniform(6000, seed=8), 0.05),
        "surfaces": (surf_q, base, 5.0),
        "outliers": (R.with_outliers(surf_q, 0.05, -60, 60, seed=9), base, 2.0),
        "far_outside_capped": (R.uniform(3000, 200.0, 300.0, seed=10), R.uniform(500, 0.0, 10.0, seed=11), 5.0),
        "far_outside_found": (R.uniform(3000, 200.0, 300.0, seed=10), R.uniform(500, 0.0, 10.0, seed=11), 1000.0),
        "duplicates": (R.uniform(3000, seed=12), dup, 0.2),
        "one_point": (R.uniform(2000, -1.0, 1.0, seed=13), np.array([[0.25, -0.5, 0.125]], np.float32), 3.0),
        "clusters_cell_cap": (cq, ct, 1.0),
        "max_dist_below_spacing": (R.uniform(4000, seed=14), R.uniform(2000, seed=15), 0.03),
        "max_dist_above_extent": (R.uniform(4000, seed=16), R.uniform(3000, seed=17), 10.0),
    }


@pytest.mark.parametrize("kind", sorted(_kinds()))
def test_nearest_matches_float64_reference(kind):
    q, t, md = _kinds()[kind]
    d, idx, grid = _device_nn(q, t, md)
    rd = _check_against_reference(q, t, md, d, idx)
    if kind == "clusters_cell_cap":
        assert np.prod(grid["dims"]) > (1 << 23)                              # the cap set the cell size
    if kind == "far_outside_capped":
        assert not np.isfinite(d).any()
    if kind in ("far_outside_found", "max_dist_above_extent", "one_point"):
        assert np.isfinite(d).all() and np.isfinite(rd).all()
    if kind == "outliers":
        assert 0.02 < (~np.isfinite(d)).mean() < 0.06
    if kind == "duplicates":
        assert (idx < 1500).all()                                             # ties go to the smallest index
    if kind == "max_dist_below_spacing":
        assert 0.02 < np.isfinite(d).mean() < 0.5


@pytest.mark.parametrize("kind", ["surfaces", "outliers", "duplicates", "far_outside_found"])
def test_result_does_not_depend_on_the_grid(kind):
    q, t, md = _kinds()[kind]
    d0, i0, g0 = _device_nn(q, t, md)
    for scale in (0.05, 0.3, 4.0):
        d, i, g = _device_nn(q, t, md, cell=g0["cell"] * scale)
        assert d.tobytes() == d0.tobytes() and i.tobytes() == i0.tobytes(), scale


def _eval_case():
    gt = R.plane_sphere(12000, extent=100.0, seed=21)
    pred = R.with_outliers(R.noisy(R.plane_sphere(9000, extent=100.0, seed=22), 0.4, seed=23), 0.04, -70, 70, seed=24)
    return pred, gt, 3.0, (0.5, 1.0, 2.0)


def _reference_metrics(pred, gt, md, th):
    dp, _, ap, _ = R.nearest(pred, gt, md)
    dg, _, ag, _ = R.nearest(gt, pred, md)
    return R.metrics(dp, dg, md, th), (ap, dp), (ag, dg)


def test_metrics_match_reference():
    from mvsnet_amd import evaluate as E
    pred, gt, md, th = _eval_case()
    got = E.evaluate_point_clouds(pred, gt, max_dist=md, thresholds=th)
    ref, (ap, _), (ag, _) = _reference_metrics(pred, gt, md, th)
    assert got["pred_points"] == got["pred_points_used"] == len(pred) and got["gt_points_used"] == len(gt)
    tp, tg = _tolerance(pred, gt, ap), _tolerance(gt, pred, ag)
    # counts exact up to the points whose float64 distance lies within the tolerance of the limit
    amb = lambda a, tol, lim: int((np.abs(a - lim) <= tol).sum())
    for a, tol, n, frac in ((ap, tp, len(pred), "accuracy_inlier_fraction"), (ag, tg, len(gt), "completeness_inlier_fraction")):
        assert abs(round(got[frac] * n) - int((a < md).sum())) <= amb(a, tol, md), frac
    for k, tau in enumerate(th):
        assert abs(round(got["precision"][k] * len(pred)) - int((ap < tau).sum())) <= amb(ap, tp, tau)
        assert abs(round(got["recall"][k] * len(gt)) - int((ag < tau).sum())) <= amb(ag, tg, tau)
        assert abs(got["fscore"][k] - ref["fscore"][k]) <= 1e-3
    clear = amb(ap, tp, md) == 0 and amb(ag, tg, md) == 0
    for k in ("accuracy", "completeness", "overall", "accuracy_median", "completeness_median"):
        assert abs(got[k] - ref[k]) <= (1e-6 if clear else 1e-4) * abs(ref[k]), k
    assert 0.9 < got["accuracy_inlier_fraction"] < 0.99 and got["fscore"][0] > 0


def test_preprocessing_on_device_matches_reference():
    from mvsnet_amd import evaluate as E
    pred, gt, md, th = _eval_case()
    th_ = np.radians(20.0)
    T = np.array([[np.cos(th_), -np.sin(th_), 0, 1.5], [np.sin(th_), np.cos(th_), 0, -2.25], [0, 0, 1, 0.5], [0, 0, 0, 1]])
    crop = (-40.0, -45.0, -1.0, 45.0, 40.0, 50.0)
    plan = E.EvaluationPlan(pred, gt, max_dist=md, thresholds=th, transform=T, crop=crop, voxel_pred=1.5, voxel_gt=0.75)
    p_crop, g_crop = R.crop(R.transform(pred, T), crop[:3], crop[3:]), R.crop(gt, crop[:3], crop[3:])
    p_ref, g_ref = R.voxel_first(p_crop, 1.5), R.voxel_first(g_crop, 0.75)
    assert plan.pred.cpu().numpy().tobytes() == p_ref.tobytes()
    assert plan.gt.cpu().numpy().tobytes() == g_ref.tobytes()
    assert len(p_ref) < len(p_crop) < len(pred) and len(g_ref) < len(g_crop) < len(gt)
    plan.enqueue()
    got = plan.result()
    assert got["pred_points_used"] == len(p_ref) and got["gt_points_used"] == len(g_ref) and got["pred_points"] == len(pred)
    ref, _, _ = _reference_metrics(p_ref, g_ref, md, th)
    assert abs(got["accuracy"] - ref["accuracy"]) <= 1e-6 * ref["accuracy"]
    assert abs(got["completeness"] - ref["completeness"]) <= 1e-6 * ref["completeness"]
    with pytest.raises(ValueError, match="cloud is empty after preprocessing"):
        E.evaluate_point_clouds(pred, gt, max_dist=md, crop=(1e3, 1e3, 1e3, 2e3, 2e3, 2e3))


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 256 * 1024 + 1])
def test_voxel_compaction_at_block_boundaries(n):
    """The compaction of mvs_voxel_select_f32 where its scans can go wrong: one point; one below, exactly and one above a
    compaction block of 1024 points; and 257 blocks, the first count that takes the single-workgroup scan of the block
    counts (256 per round) into a second round.  A survivor sits alone in voxel i of the x axis and every other point shares
    point 0's voxel, so the keep flags are the pattern: the first and the last point, about 30 % of the rest, and (257 blocks)
    none in blocks 1, 100 and 255."""
    from mvsnet_amd import evaluate as E
    keep = np.random.RandomState(n).rand(n) < 0.3
    keep[0] = keep[-1] = True
    blocks = -(-n // 1024)
    for b in ((1, 100, blocks - 2) if blocks > 3 else ()):
        keep[b * 1024:(b + 1) * 1024] = False
    i = np.arange(n)
    pts = np.zeros((n, 3), np.float32)
    pts[:, 0] = np.where(keep, i + 0.5, 0.5)                                   # exact in float32 up to 2^18 + 1/2
    pts[:, 1] = (i % 7) / 16.0                                                 # distinct points inside a voxel
    want = R.voxel_first(pts, 1.0)
    assert want.tobytes() == pts[keep].tobytes()
    got, _ = E.preprocess(pts, pts[:1], voxel_pred=1.0)
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_reproducible_and_graph_replay():
    import torch
    from mvsnet_amd import evaluate as E
    pred, gt, md, th = _eval_case()
    plan = E.EvaluationPlan(pred, gt, max_dist=md, thresholds=th)
    plan.enqueue()
    m1 = plan.result()
    d1 = [x.copy() for x in plan.distances]
    i1 = plan.acc.index.cpu().numpy().copy(), plan.comp.index.cpu().numpy().copy()
    plan.enqueue()
    m2 = plan.result()
    assert json.dumps(m1) == json.dumps(m2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(d1, plan.distances))
    # every output overwritten with values the replay has to replace
    for t in (plan.acc.dist, plan.comp.dist, plan.stats):
        t.fill_(float("nan"))
    plan.acc.index.fill_(-7)
    plan.comp.index.fill_(-7)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            plan.enqueue()
    g.replay()
    torch.cuda.synchronize()
    m3 = plan.result()
    assert json.dumps(m1) == json.dumps(m3)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(d1, plan.distances))
    assert plan.acc.index.cpu().numpy().tobytes() == i1[0].tobytes()
    assert plan.comp.index.cpu().numpy().tobytes() == i1[1].tobytes()


def _sphere_scene_gt(xyz, h):
    """Dense sample of the "sphere" scene's surface (plane z = 5.5 over the cloud's footprint, sphere (0,0,4) r 0.8)."""
    lo, hi = xyz[:, :2].min(0) - 0.1, xyz[:, :2].max(0) + 0.1
    gx, gy = np.meshgrid(np.arange(lo[0], hi[0], h), np.arange(lo[1], hi[1], h))
    plane = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 5.5)], 1)
    n = int(4 * np.pi * 0.8 ** 2 / h ** 2)
    k = np.arange(n) + 0.5
    phi, theta = np.arccos(1 - 2 * k / n), np.pi * (1 + 5 ** 0.5) * k
    sphere = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1) * 0.8 + [0.0, 0.0, 4.0]
    return np.concatenate([plane, sphere]).astype(np.float32)


def test_fusion_end_to_end_accuracy_is_the_surface_distance():
    from mvsnet_amd import evaluate as E, fusion as F
    s = FR.make_scene("sphere", V=5, H=40, W=48, low_prob_fraction=0.05, seed=7)
    plan = F.FusionPlan(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2)
    plan.enqueue()
    xyz, _, _ = plan.result()
    assert len(xyz) > 1000
    h = 0.004
    gt = _sphere_scene_gt(xyz, h)
    got = E.evaluate_point_clouds(plan.xyz[:len(xyz)], gt, max_dist=1.0, thresholds=(0.01,))
    sd = s["surface_distance"](xyz)
    assert got["accuracy_inlier_fraction"] == 1.0
    assert abs(got["accuracy"] - sd.mean()) <= h, (got["accuracy"], sd.mean())
    assert got["completeness_inlier_fraction"] > 0.2


def _write_ply(path, xyz):
    from mvsnet_amd import fusion as F
    F.write_ply(path, xyz, np.zeros((len(xyz), 3), np.uint8))


def test_cli_matches_library(tmp_path):
    from mvsnet_amd import evaluate as E
    pred, gt, md, th = _eval_case()
    _write_ply(str(tmp_path / "p.ply"), pred)
    _write_ply(str(tmp_path / "g.ply"), gt)
    out, dump = str(tmp_path / "m.json"), str(tmp_path / "dist")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "mvsnet_amd.evaluate", "--pred", str(tmp_path / "p.ply"),
                        "--gt", str(tmp_path / "g.ply"), "--max_dist", str(md), "--thresholds", ",".join(map(str, th)),
                        "--out", out, "--dump_distances", dump], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = r.stdout.strip().splitlines()[-1]
    plan = E.EvaluationPlan(pred, gt, max_dist=md, thresholds=th)
    plan.enqueue()
    lib = plan.result()
    assert json.loads(line) == json.loads(json.dumps(lib))
    assert open(out).read().strip() == line
    assert np.load(os.path.join(dump, "pred_to_gt.npy")).tobytes() == plan.distances[0].tobytes()
    assert np.load(os.path.join(dump, "gt_to_pred.npy")).tobytes() == plan.distances[1].tobytes()


def test_depthfusion_eval_gt_writes_library_metrics(tmp_path):
    from mvsnet_amd import evaluate as E, fusion as F, predictlib
    s = FR.make_scene("sphere", V=5, H=40, W=48, low_prob_fraction=0.05, image_scale=1, seed=7)
    dense = str(tmp_path / "dense")
    out = os.path.join(dense, "depths_mvsnet")
    os.makedirs(out)
    for i in range(5):
        predictlib.write_output_slice(out, s["depths"][i], s["probs"][i], s["images"][i][:, :, ::-1], s["cams"][i], i)
    idx, d, p, c, im = F.load_dense_folder(dense)
    xyz, _, _ = F.fuse_depth_maps(d, p, c, im, num_consistent=2)
    gt = _sphere_scene_gt(xyz, 0.01)
    _write_ply(str(tmp_path / "gt.ply"), gt)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "mvsnet_amd.depthfusion", "--dense_folder", dense,
                        "--fusion", "hip", "--num_consistent", "2", "--eval_gt", str(tmp_path / "gt.ply"),
                        "--eval_max_dist", "0.5", "--eval_thresholds", "0.01,0.05"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    found = [os.path.join(b, f) for b, _, fs in os.walk(os.path.join(dense, "points_mvsnet")) for f in fs if f == "metrics.json"]
    assert len(found) == 1 and os.path.isfile(os.path.join(os.path.dirname(found[0]), "final3d_model.ply"))
    lib = E.evaluate_point_clouds(xyz, gt, max_dist=0.5, thresholds=(0.01, 0.05))
    assert json.load(open(found[0])) == json.loads(json.dumps(lib))


def test_million_points_against_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    # a volume, not a surface: at 1M points on a surface the spacing is ~1e-3 of the largest coordinate, and near-ties
    # within the 1e-6 tolerance are more than 0.1 % of the queries
    gt = R.uniform(1_000_000, -1.0, 1.0, seed=31)
    pred = R.uniform(1_000_000, -1.0, 1.0, seed=32)
    md = 0.05
    d, idx, _ = _device_nn(pred, gt, md)
    tree = spatial.cKDTree(gt.astype(np.float64))
    dd, ii = tree.query(pred.astype(np.float64), k=2, workers=16)
    same_pos = (gt[ii[:, 0]] == gt[ii[:, 1]]).all(1)
    gap = np.where(same_pos, np.inf, dd[:, 1] - dd[:, 0])
    tol = _tolerance(pred, gt, dd[:, 0])
    clear = (np.abs(dd[:, 0] - md) > tol) & (gap > tol)
    assert clear.mean() >= 0.999
    assert (np.abs(d - dd[:, 0]) <= tol).all()
    assert np.array_equal(idx[clear], ii[clear, 0])
    assert np.isfinite(d).mean() > 0.999
