"""GPU tests of the ICP registration (mvs_nn_target_build_f32 / mvs_icp_step_f32 of csrc/pointcloud.hip through
mvsnet_amd.register) against the float64 reference of tests/registration_reference.py: one step (correspondences, then the
moments against math.fsum over the returned correspondences), independence of the processing order and of the grid,
reproducibility, recovery of known transforms, stages, the evaluation with align, and both command lines."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pointcloud_reference as R
from tests import registration_reference as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MD = G.MAX_CORR_DIST


@functools.lru_cache(maxsize=None)
def _cases():
    return G.cases()


@functools.lru_cache(maxsize=None)
def _reference(case, with_scale=False, tight=False):
    c = _cases()
    kw = dict(max_iterations=400, fitness_tol=1e-10, rmse_tol=1e-10) if tight else {}
    return G.icp(c[case], c["target"], MD, with_scale=with_scale, **kw)


@functools.lru_cache(maxsize=None)
def _case_b_bound():
    """10 x the distance between the reference's result on case B at tolerances 1e-6 and 1e-10: how far "converged" sits from
    the fixed point.  Measured with the module's stop rule on these seeds: 5.4e-5 rad and 3.0e-3 units (27 and 35 steps)."""
    rot, trans, _ = G.errors(_reference("B")["transform"], _reference("B", tight=True)["transform"])
    return 10 * rot, 10 * trans


def _step_kinds():
    c = _cases()
    uni = R.uniform(1500, 0.0, 100.0, seed=4)
    return {
        "case_B": (c["B"], c["target"], MD),
        "duplicates": (R.uniform(3000, 0.0, 100.0, seed=12), np.concatenate([uni, uni[::-1], uni]), MD),   # every target point three times
        "beyond": (R.uniform(2000, 200.0, 300.0, seed=10), R.uniform(500, 0.0, 10.0, seed=11), MD),          # count == 0
        "one_point": (R.uniform(2000, -1.0, 1.0, seed=13), np.array([[0.25, -0.5, 0.125]], np.float32), 3.0),
    }


def _step_transforms():
    traj = _reference("B")["trajectory"]
    return {"identity": np.eye(4), "T0": _cases()["T0"], "intermediate": traj[len(traj) // 2]}


def _device_step(plan, T, order="plan"):
    import torch
    n = plan.source.shape[0]
    dist = torch.full((n,), -1.0, dtype=torch.float32, device=plan.dev)
    index = torch.full((n,), -7, dtype=torch.int32, device=plan.dev)
    m = plan.step_host(T, order=order, dist=dist, index=index)
    return m, dist.cpu().numpy(), index.cpu().numpy()


def _check_moments(m, src, tgt, idx, T, cp, cq):
    """Each moment against math.fsum over the correspondences the device returned: (n + 16) 2^-52 sum |term| bounds a float64
    sum of n such terms in any order, with or without fused multiply-adds."""
    terms = G.moment_terms(src, tgt, idx, T, cp, cq)
    ref, mag = G.moments_from_terms(terms)
    n = len(terms)
    assert m[0] == n
    bound = (n + 16) * 2.0 ** -52 * mag
    print("moment errors / bound:", (np.abs(m - ref) / np.maximum(bound, 1e-300)).round(4).tolist())
    assert (np.abs(m - ref) <= bound).all(), (np.abs(m - ref) / np.maximum(bound, 1e-300)).tolist()
    if n == 0:
        assert not m.any()
    return ref, bound


@pytest.mark.parametrize("kind", ["case_B", "duplicates", "beyond", "one_point"])
def test_one_step_matches_the_reference(kind):
    from mvsnet_amd import register as Rg
    from tests.test_gpu_pointcloud_eval import _check_against_reference
    src, tgt, md = _step_kinds()[kind]
    plan = Rg.RegistrationPlan(src, tgt, max_corr_dist=md)
    assert np.abs(plan.cp - src.astype(np.float64).mean(0)).max() <= 1e-9 * 300
    assert np.abs(plan.cq - tgt.astype(np.float64).mean(0)).max() <= 1e-9 * 300
    for name, T in _step_transforms().items():
        m, d, idx = _device_step(plan, T)
        assert m.shape == (18,) and np.isfinite(m).all()
        # which neighbour: the rule of the nearest-neighbour tests, for the moved points
        _check_against_reference(R.transform(src, T), tgt, md, d, idx.astype(np.int64))
        # how it was summed
        _check_moments(m, src, tgt, idx, T, plan.cp, plan.cq)
        if kind == "beyond":
            assert m[0] == 0 and (idx == -1).all() and np.isinf(d).all()
        if kind == "case_B" and name == "T0":
            assert abs(m[0] / len(src) - 0.956) < 2e-3


def test_order_and_grid_change_no_correspondence():
    import torch
    from mvsnet_amd import register as Rg
    c = _cases()
    src, tgt = c["B"], c["target"]
    T = _step_transforms()["intermediate"]
    plan = Rg.RegistrationPlan(src, tgt, max_corr_dist=MD)
    order = plan.order.cpu().numpy()
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(len(src)))
    m0, d0, i0 = _device_step(plan, T, order=None)
    ref, bound = _check_moments(m0, src, tgt, i0, T, plan.cp, plan.cq)
    runs = [_device_step(plan, T, order="plan"),
            _device_step(plan, T, order=torch.arange(len(src) - 1, -1, -1, dtype=torch.int32, device=plan.dev))]
    for scale in (0.3, 4.0):
        other = Rg.RegistrationPlan(src, tgt, max_corr_dist=MD, cell=plan.grid["cell"] * scale)
        assert other.grid["dims"] != plan.grid["dims"]
        m, d, i = _device_step(other, T)
        runs.append((m, d, i))
        # the centres are the same numbers, so the same lanes sum the same terms: with the same order even the bits agree
        ms, _, _ = _device_step(other, T, order=plan.order)
        mp, _, _ = _device_step(plan, T, order=plan.order)
        assert ms.tobytes() == mp.tobytes()
    for m, d, i in runs:
        assert i.tobytes() == i0.tobytes() and d.tobytes() == d0.tobytes() and m[0] == m0[0]
        assert (np.abs(m - ref) <= bound).all()


def test_two_runs_give_the_same_bits():
    from mvsnet_amd import register as Rg
    c = _cases()
    plan = Rg.RegistrationPlan(c["B"], c["target"], max_corr_dist=MD, max_iterations=6)
    T = _step_transforms()["intermediate"]
    a, b = plan.step_host(T), plan.step_host(T)
    assert a.tobytes() == b.tobytes()
    r1, r2 = plan.run(), plan.run()
    assert np.array(r1["transform"]).tobytes() == np.array(r2["transform"]).tobytes() and r1["history"] == r2["history"]
    again = Rg.RegistrationPlan(c["B"], c["target"], max_corr_dist=MD, max_iterations=6).run()
    assert np.array(again["transform"]).tobytes() == np.array(r1["transform"]).tobytes()
    assert r1["iterations"] == 6 and r1["stopped"] == "max_iterations" and len(r1["history"]) == 6


def _result_shape_ok(r, n_iter_max):
    T = np.array(r["transform"])
    assert T.shape == (4, 4) and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert len(r["history"]) == r["iterations"] <= n_iter_max and r["history"][-1] == [r["fitness"], r["inlier_rmse"]]


def test_recovers_a_rigid_motion_case_a():
    """Bound: 10 x the error the float64 reference itself reaches on the same inputs (float32 rounding of the source sets
    that floor).  Reference on these seeds: 1.6e-10 rad, 6.4e-9 units, 10 steps, fitness 1, rmse 9.8e-7."""
    from mvsnet_amd import register as Rg
    c = _cases()
    ref_rot, ref_trans, _ = G.errors(_reference("A")["transform"], c["T0"])
    r = Rg.RegistrationPlan(c["A"], c["target"], max_corr_dist=MD).run()
    _result_shape_ok(r, 50)
    rot, trans, _ = G.errors(r["transform"], c["T0"])
    print("case A: device", rot, trans, r["iterations"], "reference", ref_rot, ref_trans, _reference("A")["iterations"])
    assert r["stopped"] == "converged" and r["fitness"] == 1.0
    assert rot <= 10 * ref_rot and trans <= 10 * ref_trans, (rot, trans, ref_rot, ref_trans)


def test_recovers_a_similarity_case_c():
    """As case A with scale 1.03 and with_scale.  Reference on these seeds: 4.5e-10 rad, 1.8e-8 units, |scale - 1| 1.6e-10,
    11 steps."""
    from mvsnet_amd import register as Rg
    c = _cases()
    ref_rot, ref_trans, ref_s = G.errors(_reference("C", with_scale=True)["transform"], c["T0s"])
    r = Rg.RegistrationPlan(c["C"], c["target"], max_corr_dist=MD, with_scale=True).run()
    _result_shape_ok(r, 50)
    rot, trans, s = G.errors(r["transform"], c["T0s"])
    print("case C: device", rot, trans, s - 1, r["iterations"], "reference", ref_rot, ref_trans, ref_s - 1)
    assert r["stopped"] == "converged" and r["fitness"] == 1.0
    assert rot <= 10 * ref_rot and trans <= 10 * ref_trans and abs(s - 1) <= 10 * abs(ref_s - 1), (rot, trans, s - 1)


def test_noisy_case_b_ends_where_the_reference_ends():
    """Reference on these seeds: 27 steps, fitness 0.9565, rmse 0.8417; bound _case_b_bound() = 5.4e-4 rad, 3.0e-2 units."""
    from mvsnet_amd import register as Rg
    c = _cases()
    ref = _reference("B")
    r = Rg.RegistrationPlan(c["B"], c["target"], max_corr_dist=MD).run()
    _result_shape_ok(r, 50)
    rot, trans, _ = G.errors(r["transform"], ref["transform"])
    print("case B: device", rot, trans, r["iterations"], r["fitness"], r["inlier_rmse"], "bound", _case_b_bound())
    assert r["stopped"] == "converged"
    assert rot <= _case_b_bound()[0] and trans <= _case_b_bound()[1], (rot, trans, _case_b_bound())
    assert abs(r["fitness"] - ref["fitness"]) < 2e-3 and abs(r["inlier_rmse"] - ref["inlier_rmse"]) < 5e-3


def test_stage_list_ends_within_the_single_stage_bounds():
    """[(4, 8, 30), (0, 2, 30)] on cases A and B.  The float64 reference with the same stages ends 1.6e-10 rad / 6.4e-9 from T0
    on A (bit for bit its single-stage result) and 2.2e-4 rad / 6.0e-3 from its single-stage result on B."""
    from mvsnet_amd import register as Rg
    c = _cases()
    stages = [(4, 8, 30), (0, 2, 30)]
    ref_rot, ref_trans, _ = G.errors(_reference("A")["transform"], c["T0"])
    a = Rg.register_point_clouds(c["A"], c["target"], stages=stages)
    assert [s["voxel"] for s in a["stages"]] == [4.0, 0.0] and a["stopped"] == "converged" == a["stages"][0]["stopped"]
    assert a["stages"][0]["source_points"] < len(c["A"]) and a["stages"][1]["source_points"] == len(c["A"])
    assert a["transform"] == a["stages"][-1]["transform"]
    rot, trans, _ = G.errors(a["transform"], c["T0"])
    print("stages A:", rot, trans, [s["iterations"] for s in a["stages"]])
    assert rot <= 10 * ref_rot and trans <= 10 * ref_trans, (rot, trans)
    b = Rg.register_point_clouds(c["B"], c["target"], stages=stages)
    rot, trans, _ = G.errors(b["transform"], _reference("B")["transform"])
    print("stages B:", rot, trans, [s["iterations"] for s in b["stages"]], "bound", _case_b_bound())
    assert b["stopped"] == "converged" and rot <= _case_b_bound()[0] and trans <= _case_b_bound()[1], (rot, trans)


def test_no_overlap_stops_and_returns_init():
    from mvsnet_amd import register as Rg
    src, tgt, md = _step_kinds()["beyond"]
    init = G.rigid(degrees=1.0, translation=(0.5, 0.25, -0.125))
    r = Rg.RegistrationPlan(src, tgt, max_corr_dist=md, init=init).run()
    assert r["stopped"] == "too_few_correspondences" and r["iterations"] == 1 and r["fitness"] == 0.0 and r["inlier_rmse"] is None
    assert np.array(r["transform"]).tobytes() == init.tobytes()
    m = Rg.register_point_clouds(src, tgt, stages=[(0, md, 5), (0, md / 2, 5)], init=init)
    assert m["stopped"] == "too_few_correspondences" and len(m["stages"]) == 1
    assert np.array(m["transform"]).tobytes() == init.tobytes()


def _prediction():
    """An independent noisy sample of the scene with 5 % outliers, and the same cloud displaced by T0^-1."""
    c = _cases()
    und = R.with_outliers(R.noisy(G.asymmetric_scene(7000, seed=32), 0.3, seed=33), 0.05, -60, 60, seed=34)
    return und, R.transform(und, np.linalg.inv(c["T0"]))


EVAL = dict(max_dist=5.0, thresholds=(0.5, 1.0, 2.0))


def test_evaluation_with_align_scores_the_displaced_cloud_as_the_undisplaced_one():
    """The float64 reference (its ICP with these stages and this crop, then its metrics) gives F-scores 0.2563 / 0.7414 /
    0.9729 for the realigned cloud, 0.2562 / 0.7403 / 0.9730 for the undisplaced one and 0.0617 / 0.3185 / 0.7878 without the
    alignment; its transform ends 4.1e-4 rad / 4.4e-3 units from T0."""
    from mvsnet_amd import evaluate as E
    c = _cases()
    und, disp = _prediction()
    box = [-70, -70, -40, 70, 70, 60]
    plain = E.evaluate_point_clouds(disp, c["target"], crop=box, **EVAL)
    assert "alignment" not in plain
    m = E.evaluate_point_clouds(disp, c["target"], crop=box, align={"stages": [(2, 5, 30), (0, 5, 50)]}, **EVAL)
    al = m["alignment"]
    assert al["stopped"] == "converged" and len(al["stages"]) == 2
    assert set(al["stages"][0]) == {"voxel", "max_corr_dist", "fitness", "inlier_rmse", "iterations", "stopped"}
    rot, trans, _ = G.errors(al["transform"], c["T0"])
    assert rot < 2e-3 and trans < 5e-2, (rot, trans)
    same = E.evaluate_point_clouds(disp, c["target"], crop=box, transform=al["transform"], **EVAL)
    for k in same:
        assert m[k] == same[k], k                                      # to the counts: every metric, both grids
    own = E.evaluate_point_clouds(und, c["target"], crop=box, **EVAL)
    print("fscore aligned", m["fscore"], "undisplaced", own["fscore"], "unaligned", plain["fscore"])
    assert max(abs(a - b) for a, b in zip(m["fscore"], own["fscore"])) <= 0.01
    assert plain["fscore"][1] < own["fscore"][1] - 0.1                  # the displacement did matter


def test_register_then_evaluate_equals_evaluate_with_align(tmp_path):
    from mvsnet_amd import fusion as F
    c = _cases()
    _, disp = _prediction()
    pred, gt = disp[::3], c["target"][::2]
    F.write_ply(str(tmp_path / "p.ply"), pred, np.zeros((len(pred), 3), np.uint8))
    F.write_ply(str(tmp_path / "g.ply"), gt, np.zeros((len(gt), 3), np.uint8))
    p, g, t = str(tmp_path / "p.ply"), str(tmp_path / "g.ply"), str(tmp_path / "T.txt")
    stages = "4:8:30,0:5:40"

    def run(args):
        r = subprocess.run([sys.executable, "-m"] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])
    rep = run(["mvsnet_amd.register", "--source", p, "--target", g, "--stages", stages, "--out", t, "--report",
               str(tmp_path / "R.json")])
    assert rep["stopped"] == "converged" and json.load(open(str(tmp_path / "R.json"))) == rep
    assert np.loadtxt(t).reshape(4, 4).tobytes() == np.array(rep["transform"]).tobytes()
    ev = ["mvsnet_amd.evaluate", "--pred", p, "--gt", g, "--max_dist", "5", "--thresholds", "0.5,1,2"]
    a = run(ev + ["--transform", t])
    b = run(ev + ["--align", "icp", "--align_stages", stages])
    assert b["alignment"]["transform"] == rep["transform"]
    assert [s["iterations"] for s in b["alignment"]["stages"]] == [s["iterations"] for s in rep["stages"]]
    assert {k: v for k, v in b.items() if k != "alignment"} == a
