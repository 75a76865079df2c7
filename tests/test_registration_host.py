"""CPU tests of the ICP registration (mvsnet_amd/register.py): the solve from moments, stage parsing, the transform file, the
argument checks of the mvs_nn_target / mvs_icp_step entry points (no GPU call), the command line without a GPU, and the
float64 reference loop of tests/registration_reference.py on the three cases the GPU tests use."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pointcloud_reference as R
from tests import registration_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exact_moments(p, q, T, cp, cq):
    idx = np.arange(len(p))
    return G.moments_from_terms(G.moment_terms(p, q, idx, T, cp, cq))[0]


def _cloud(n, seed):
    return (np.random.RandomState(seed).uniform(-50, 50, (n, 3))).astype(np.float32)


@pytest.mark.parametrize("scale", [1.0, 1.03, 0.4])
def test_solve_recovers_a_known_similarity_from_exact_correspondences(scale):
    from mvsnet_amd import register as Rg
    p = _cloud(500, 1)
    T0 = G.rigid(axis=(3, -1, 2), degrees=40.0, translation=(7.0, -3.0, 11.0), scale=scale)
    # float64 images of the float32 source: moment_terms casts the target to float32, so feed the terms directly
    p64 = p.astype(np.float64)
    q64 = p64 @ T0[:3, :3].T + T0[:3, 3]
    cp, cq = p64.mean(0), q64.mean(0)
    a, b = p64 - cp, q64 - cq
    m = np.zeros(18)
    m[0] = len(p)
    m[2:5], m[5:8] = a.sum(0), b.sum(0)
    m[8:17] = (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1)
    m[17] = (a * a).sum()
    T, why = Rg.solve_from_moments(m, cp, cq, with_scale=scale != 1.0)
    assert why is None and T.dtype == np.float64 and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    rot, trans, s = G.errors(T, T0)
    assert rot <= 1e-12 and trans <= 1e-12 and abs(s - 1.0) <= 1e-12, (rot, trans, s)
    # the centres only centre the sums: another pair gives the same transform
    cp2, cq2 = cp + [3.0, -2.0, 1.0], cq - [5.0, 0.5, 2.0]
    a, b = p64 - cp2, q64 - cq2
    m[2:5], m[5:8], m[8:17], m[17] = a.sum(0), b.sum(0), (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1), (a * a).sum()
    T2, _ = Rg.solve_from_moments(m, cp2, cq2, with_scale=scale != 1.0)
    assert np.abs(T2 - T).max() <= 1e-10
    # and the reference's statement of the solve agrees with the module's
    T3, _ = G.solve_from_moments(m, cp2, cq2, with_scale=scale != 1.0)
    assert np.array_equal(T3, T2)


def test_solve_of_mirrored_correspondences_is_a_proper_rotation():
    from mvsnet_amd import register as Rg
    p = _cloud(300, 2)
    q = p * np.array([1.0, 1.0, -1.0], np.float32)                 # a reflection: no rotation maps p onto q
    cp, cq = p.astype(np.float64).mean(0), q.astype(np.float64).mean(0)
    T, why = Rg.solve_from_moments(_exact_moments(p, q, np.eye(4), cp, cq), cp, cq)
    assert why is None
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) <= 1e-12 and np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-12


def test_solve_reports_too_few_and_degenerate():
    from mvsnet_amd import register as Rg
    p = _cloud(2, 3)
    cp = p.astype(np.float64).mean(0)
    assert Rg.solve_from_moments(_exact_moments(p, p, np.eye(4), cp, cp), cp, cp) == (None, "too_few_correspondences")
    assert Rg.solve_from_moments(np.zeros(18), cp, cp) == (None, "too_few_correspondences")
    line = (np.arange(20, dtype=np.float32)[:, None] * np.array([[1.0, 2.0, -0.5]], np.float32)).astype(np.float32)
    cl = line.astype(np.float64).mean(0)
    assert Rg.solve_from_moments(_exact_moments(line, line, np.eye(4), cl, cl), cl, cl) == (None, "degenerate")
    same = np.repeat(np.array([[1.0, 2.0, 3.0]], np.float32), 5, 0)
    cs = same.astype(np.float64).mean(0)
    assert Rg.solve_from_moments(_exact_moments(same, same, np.eye(4), cs, cs), cs, cs, with_scale=True) == (None, "degenerate")
    with pytest.raises(ValueError):
        Rg.solve_from_moments(np.zeros(17), cp, cp)


def test_stage_parsing():
    from mvsnet_amd import register as Rg
    assert Rg.parse_stages("4:8:30,2:4:30,0:2:30") == [(4.0, 8.0, 30), (2.0, 4.0, 30), (0.0, 2.0, 30)]
    assert Rg.parse_stages("0.5:1.25:7") == [(0.5, 1.25, 7)]
    assert Rg.check_stages([(4, 8, 30), (0, 2, 30)]) == [(4.0, 8.0, 30), (0.0, 2.0, 30)]
    for bad in ("", "4:8", "4:8:30:1", "a:8:30", "4:0:30", "-1:8:30", "4:8:0", "4:8:2.5", "4:inf:3"):
        with pytest.raises(ValueError):
            Rg.parse_stages(bad)
    with pytest.raises(ValueError):
        Rg.check_stages([])


def test_transform_file_round_trip_keeps_every_bit(tmp_path):
    from mvsnet_amd import evaluate as E
    from mvsnet_amd import register as Rg
    T = G.rigid(axis=(0.3, -2, 1), degrees=17.3, translation=(1 / 3, -2e-7, 1e9 / 7), scale=1.03)
    T[0, 1] = np.nextafter(T[0, 1], 1.0)
    path = str(tmp_path / "T.txt")
    Rg.write_transform(path, T)
    back = np.loadtxt(path, dtype=np.float64).reshape(4, 4)               # what evaluate --transform does
    assert back.tobytes() == T.tobytes() and Rg.read_transform(path).tobytes() == T.tobytes()
    assert np.array_equal(E.check_transform(back), T)                     # a scaled result is an accepted transform
    with pytest.raises(ValueError):
        Rg.write_transform(path, np.ones((4, 4)))


def test_entry_points_check_arguments_without_gpu(lib_built):
    import ctypes
    from mvsnet_amd import _lib
    h = _lib.load()
    BADARG, SHAPE, WORKSPACE = -1, -2, -3
    assert h.mvs_nn_target_workspace_bytes(200, 4, 4, 4) > 0
    assert h.mvs_nn_target_workspace_bytes(0, 4, 4, 4) == 0 and h.mvs_nn_target_workspace_bytes(200, 4, 0, 4) == 0
    assert h.mvs_nn_target_workspace_bytes(200, 1 << 10, 1 << 10, 1 << 10) == 0
    assert h.mvs_icp_step_workspace_bytes(100) > 0 and h.mvs_icp_step_workspace_bytes(0) == 0
    assert h.mvs_icp_step_workspace_bytes(2 ** 31 - 2) == h.mvs_icp_step_workspace_bytes(10 ** 7)   # a fixed grid of blocks
    nz = 4096                                  # never dereferenced: the checks return before any HIP call
    tws, sws = h.mvs_nn_target_workspace_bytes(200, 4, 4, 4), h.mvs_icp_step_workspace_bytes(100)

    def build(**kw):
        a = dict(t=nz, nt=200, ox=0.0, cell=1.0, gx=4, gy=4, gz=4, ws=nz, wsb=tws)
        a.update(kw)
        return h.mvs_nn_target_build_f32(a["t"], a["nt"], a["ox"], 0.0, 0.0, a["cell"], a["gx"], a["gy"], a["gz"], a["ws"],
                                         a["wsb"], None)
    assert build(t=None) == BADARG and build(ws=None) == BADARG and build(nt=0) == BADARG and build(nt=-3) == BADARG
    assert build(gx=0) == BADARG and build(gz=-1) == BADARG and build(cell=0.0) == BADARG and build(cell=float("nan")) == BADARG
    assert build(ox=float("inf")) == BADARG
    assert build(gx=1 << 10, gy=1 << 10, gz=1 << 10) == SHAPE
    assert build(wsb=tws - 1) == WORKSPACE

    eye = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    zero = (ctypes.c_double * 3)(0, 0, 0)

    def step(**kw):
        a = dict(s=nz, n=100, order=None, T=eye, cp=zero, cq=zero, cell=1.0, gx=4, gy=4, gz=4, nt=200, tw=nz, twb=tws, md=2.0,
                 mom=nz, dist=None, idx=None, ws=nz, wsb=sws)
        a.update(kw)
        return h.mvs_icp_step_f32(a["s"], a["n"], a["order"], a["T"], a["cp"], a["cq"], 0.0, 0.0, 0.0, a["cell"], a["gx"], a["gy"],
                                  a["gz"], a["nt"], a["tw"], a["twb"], a["md"], a["mom"], a["dist"], a["idx"], a["ws"], a["wsb"],
                                  None)
    assert step(s=None) == BADARG and step(T=None) == BADARG and step(cp=None) == BADARG and step(cq=None) == BADARG
    assert step(tw=None) == BADARG and step(mom=None) == BADARG and step(ws=None) == BADARG
    assert step(n=0) == BADARG and step(n=-7) == BADARG and step(nt=0) == BADARG and step(gy=0) == BADARG
    assert step(cell=-1.0) == BADARG and step(md=0.0) == BADARG and step(md=float("inf")) == BADARG and step(md=1e30) == BADARG
    bad = (ctypes.c_double * 12)(*([1.0] * 11 + [float("nan")]))
    assert step(T=bad) == BADARG and step(cp=(ctypes.c_double * 3)(0, float("inf"), 0)) == BADARG
    assert step(gx=1 << 10, gy=1 << 10, gz=1 << 10) == SHAPE
    assert step(twb=tws - 1) == WORKSPACE and step(wsb=sws - 1) == WORKSPACE


def test_plan_and_stage_arguments_are_checked_before_any_gpu_use():
    from mvsnet_amd import register as Rg
    p = _cloud(10, 4)
    for kw in (dict(max_corr_dist=0.0), dict(max_corr_dist=float("inf")), dict(max_corr_dist=1.0, max_iterations=0),
               dict(max_corr_dist=1.0, rmse_tol=-1.0), dict(max_corr_dist=1.0, init=np.ones((4, 4)))):
        with pytest.raises(ValueError):
            Rg.RegistrationPlan(p, p, **kw)
    with pytest.raises(ValueError):
        Rg.register_point_clouds(p, p, stages=[])
    with pytest.raises(ValueError):
        Rg.register_point_clouds(p, p, stages=[(0, 1, 5)], crop=[1, 0, 0, 0, 1, 1])


def test_cli_without_gpu_fails_clearly(tmp_path):
    from mvsnet_amd import fusion as F
    F.write_ply(str(tmp_path / "a.ply"), np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    base = [sys.executable, "-m", "mvsnet_amd.register", "--source", str(tmp_path / "a.ply"), "--target", str(tmp_path / "a.ply"),
            "--out", str(tmp_path / "T.txt")]
    r = subprocess.run(base + ["--stages", "0:1:5"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs a GPU" in r.stderr and "Traceback" not in r.stderr
    assert not os.path.exists(str(tmp_path / "T.txt"))
    r = subprocess.run(base + ["--stages", "0:1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "voxel:max_corr_dist:max_iterations" in r.stderr and "Traceback" not in r.stderr


def test_tree_correspondences_equal_the_brute_force():
    uni = R.uniform(1500, seed=4)
    dup = np.concatenate([uni, uni[::-1], uni, uni, uni])                  # five copies: more ties than the tree's candidates
    q = R.uniform(800, seed=12)
    for t, md in ((dup, 0.2), (G.asymmetric_scene(3000, seed=5), 5.0)):
        a, b = G.correspondences(q * (1 if t is dup else 50), t, md), G.tree_correspondences(q * (1 if t is dup else 50), t, md)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_reference_loop_reproduces_the_three_cases():
    """Figures of the reference on these seeds: A 10 steps, fitness 1, rmse 9.8e-7, 1.6e-10 rad / 6.4e-9 from T0; B 27 steps,
    fitness 0.9565, rmse 0.8417; C 11 steps, scale within 1.7e-10, 4.5e-10 rad / 1.8e-8."""
    c = G.cases()
    a = G.icp(c["A"], c["target"], G.MAX_CORR_DIST)
    rot, trans, _ = G.errors(a["transform"], c["T0"])
    assert a["stopped"] == "converged" and a["iterations"] <= 12 and a["fitness"] == 1.0 and a["inlier_rmse"] < 5e-6
    assert rot < 1e-8 and trans < 1e-7, (rot, trans)
    b = G.icp(c["B"], c["target"], G.MAX_CORR_DIST)
    rot, trans, _ = G.errors(b["transform"], c["T0"])
    assert b["stopped"] == "converged" and b["iterations"] <= 35
    assert abs(b["fitness"] - 0.956) < 2e-3 and abs(b["inlier_rmse"] - 0.84) < 0.01 and rot < 1e-3 and trans < 2e-2, (rot, trans)
    assert len(b["history"]) == b["iterations"] == len(b["trajectory"])
    s = G.icp(c["C"], c["target"], G.MAX_CORR_DIST, with_scale=True)
    rot, trans, scale = G.errors(s["transform"], c["T0s"])
    assert s["stopped"] == "converged" and s["fitness"] == 1.0 and abs(scale - 1.0) < 1e-8 and rot < 1e-8 and trans < 1e-6
    # without the scale the same source cannot reach T0s
    r = G.icp(c["C"], c["target"], G.MAX_CORR_DIST)
    assert r["inlier_rmse"] > 0.1
