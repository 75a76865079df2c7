"""CPU tests of the point-cloud rendering (mvsnet_amd/render.py): the numpy restatement of tests/render_reference.py on
hand-computed cases, the projection tables, the two-layer occlusion case, the depth PNG writer, the argument checks of the
mvs_render entry points (no GPU call) and the command line's parsing."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import render_reference as R
from tests._helpers import make_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 6, 8


def _hand_cam():
    """Identity pose, f = 2, principal point (4, 3): the point (x - 4, y - 3, 2) projects onto pixel (x, y) exactly, at depth 2."""
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[1, :3, :3] = [[2.0, 0, 4.0], [0, 2.0, 3.0], [0, 0, 1.0]]
    return cam[None]


def _at(x, y, z=2.0):
    return [(x - 4.0) * z / 2.0, (y - 3.0) * z / 2.0, z]


def test_one_point_per_hand_computed_pixel():
    inside = [(3, 2), (0, 2), (7, 2), (3, 0), (3, 5), (0, 0), (7, 5)]            # interior, each border, two corners
    outside = [(-1, 2), (8, 2), (3, -1), (3, 6)]                               # one pixel outside each border
    pts = [_at(x, y) for x, y in inside + outside]
    pts.append([0.0, 0.0, -2.0])                                               # behind the camera
    pts.append([0.0, 0.0, 0.0])                                                # w = 0 = min_depth exactly
    nan, inf = float("nan"), float("inf")
    pts += [[nan, 0, 2], [0, nan, 2], [0, 0, nan], [inf, 0, 2], [0, -inf, 2], [0, 0, inf], [1e38, 1e38, 1e-38], [1e30, -1e30, 2]]
    pts = np.array(pts, np.float32)
    depth, index = R.render(pts, _hand_cam(), H, W)
    want_d, want_i = np.zeros((1, H, W), np.float32), np.full((1, H, W), -1, np.int32)
    for i, (x, y) in enumerate(inside):
        want_d[0, y, x], want_i[0, y, x] = 2.0, i
    assert np.array_equal(depth, want_d) and np.array_equal(index, want_i)
    # w = min_depth exactly is culled, the next float32 above it is drawn
    two = np.array([_at(3, 2, 2.0), _at(5, 4, float(np.nextafter(np.float32(2), np.float32(3))))], np.float32)
    depth, index = R.render(two, _hand_cam(), H, W, min_depth=2.0)
    assert (index >= 0).sum() == 1 and index[0, 4, 5] == 1 and depth[0, 4, 5] > 2.0
    # the float64 twin agrees on cases this exact
    d64, i64 = R.render(pts, _hand_cam(), H, W, dtype=np.float64)
    assert np.array_equal(i64, want_i) and np.array_equal(d64, want_d)


def test_ties_go_to_the_smallest_index():
    a = _at(3, 2)
    depth, index = R.render(np.array([_at(1, 1), a, a], np.float32), _hand_cam(), H, W)
    assert index[0, 2, 3] == 1 and depth[0, 2, 3] == 2.0
    # two different points, equal float32 w, one pixel: (3.1, 2.2) and (2.9, 1.8) both round to (3, 2)
    pts = np.array([_at(1, 1), _at(3.1, 2.2), _at(2.9, 1.8)], np.float32)
    depth, index = R.render(pts, _hand_cam(), H, W)
    assert index[0, 2, 3] == 1 and (index >= 0).sum() == 2
    depth, index = R.render(pts[::-1].copy(), _hand_cam(), H, W)
    assert index[0, 2, 3] == 0
    # a nearer point beats a smaller index
    pts = np.array([_at(3, 2, 2.0), _at(3, 2, 1.0)], np.float32)
    depth, index = R.render(pts, _hand_cam(), H, W)
    assert index[0, 2, 3] == 1 and depth[0, 2, 3] == 1.0


def test_a_splat_at_a_corner_is_clipped_to_the_image():
    depth, index = R.render(np.array([_at(0, 0), _at(7, 5)], np.float32), _hand_cam(), H, W, splat=2)
    want = np.full((H, W), -1, np.int32)
    want[0:3, 0:3] = 0
    want[3:6, 5:8] = 1
    assert np.array_equal(index[0], want) and np.array_equal(depth[0] > 0, want >= 0)
    # a point outside the image still covers the pixels its splat reaches
    depth, index = R.render(np.array([_at(-1, 2)], np.float32), _hand_cam(), H, W, splat=1)
    assert sorted(zip(*np.nonzero(index[0] >= 0))) == [(1, 0), (2, 0), (3, 0)]


def test_projection_tables_equal_the_fusion_matrix_rounded_once():
    from mvsnet_amd import fusion as Fu
    from mvsnet_amd import render as Rn
    cams = R.scene("sphere")["cams"]
    t = Rn.projection_tables(cams)
    assert t.dtype == np.float32 and t.shape == (5 * 12,)
    for v in range(5):
        assert np.array_equal(t[12 * v:12 * v + 12], Fu.projection_matrix(cams[v]).astype(np.float32).reshape(-1))
    assert np.array_equal(t.reshape(5, 3, 4), R.projection_tables(cams))
    with pytest.raises(ValueError):
        Rn.projection_tables(np.zeros((2, 4, 4)))


def test_two_layer_case_and_its_occlusion_filter():
    pts, cams, front = R.two_layer()
    Hh, Ww = front.shape
    assert pts.dtype == np.float32 and len(pts) == Hh * Ww + int(front.sum())
    raw, raw_i = R.render(pts, cams, Hh, Ww)
    assert int((raw == 500).sum()) == 192 and int((raw == 800).sum()) == 576 and int((raw > 0).sum()) == Hh * Ww
    assert np.array_equal(raw[0] == 500, front)
    d, i = R.render(pts, cams, Hh, Ww, occlusion=(1, 0.1, 2))
    removed = (raw > 0) & (d == 0)
    assert np.array_equal(i < 0, removed) and np.array_equal(d[~removed], raw[~removed]) and np.array_equal(i[~removed], raw_i[~removed])
    assert not (d[0, 1:-1, 1:Ww // 2 - 1] == 800).any()                      # no back pixel is left in the interior of the left half
    assert (d[0][front] == 500).all()                                         # all 192 front pixels stay
    assert not removed[0, :, Ww // 2 + 1:].any()                              # nothing is removed beyond the front layer's reach
    assert int(removed.sum()) == R.TWO_LAYER_REMOVED == 203
    # the filter is a function of the raw map alone
    d2, i2 = R.occlusion_filter(raw, raw_i, 1, 0.1, 2)
    assert np.array_equal(d2, d) and np.array_equal(i2, i)


def test_depth_png_rounding_overflow_and_zeros(tmp_path):
    from mvsnet_amd import render as Rn
    from mvsnet_amd.mvs_data_generation import Cluster
    d = np.array([[0.0, 0.49, 0.5, 1.49], [1.5, 599.5, 65535.49, 65535.5], [70000.0, np.inf, np.nan, -3.0]], np.float32)
    want = np.array([[0, 0, 1, 1], [2, 600, 65535, 0], [0, 0, 0, 0]], np.uint16)
    got = Rn.depth_to_png16(d)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    # a session rendered by the reference: the files load through Cluster.load_depth
    session = make_session(str(tmp_path / "s"))
    views = Rn.session_views(session)
    assert [v[0] for v in views] == [0, 1, 2, 3] and all(v[2] == (48, 64) for v in views)
    assert views[1][1][0, 0, 3] == 50.0                                       # 0.05 m -> millimetres
    assert Rn.size_groups(views) == [((48, 64), [0, 1, 2, 3])]
    yy, xx = np.mgrid[0:48, 0:64]
    from tests import fusion_reference as F
    cloud = F._backproject(views[0][1], xx.reshape(-1), yy.reshape(-1), np.full(48 * 64, 600.0)).astype(np.float32)
    depth, _ = R.render(cloud, np.stack([v[1] for v in views]), 48, 64)
    os.makedirs(os.path.join(session, "depths"))
    for (i, _, _), dm in zip(views, depth):
        Rn.write_depth_png(os.path.join(session, "depths", "%d.png" % i), dm)
    c = Cluster(session, 0, [1, 2], 400.0, 900.0, 3)
    for i in range(4):
        back = c.load_depth(i)
        assert back is not None and back.dtype == np.uint16 and np.array_equal(back, Rn.depth_to_png16(depth[i]))
    assert (c.load_depth(0) == 600).all()


def test_force_rule_and_cli_parsing(tmp_path):
    from mvsnet_amd import render as Rn
    session = make_session(str(tmp_path / "s"))
    a = Rn.parse_args(["--cloud", "g.ply", "--session", session, "--occlusion", "2:0.05:3", "--splat", "1", "--min_depth", "10",
                       "--write_index", "--cloud_scale", "1000"])
    assert a.occlusion == (2, 0.05, 3) and a.splat == 1 and a.min_depth == 10.0 and a.write_index and a.cloud_scale == 1000.0
    assert a.dense_folder is None and a.transform is None and not a.force
    assert Rn.prepare_output(a) == os.path.join(session, "depths")
    os.makedirs(os.path.join(session, "depths"))
    with pytest.raises(SystemExit, match="--force"):
        Rn.prepare_output(a)
    a = Rn.parse_args(["--cloud", "g.ply", "--session", session, "--force"])
    assert a.occlusion is None and a.splat == 0 and a.min_depth == 0.0 and Rn.prepare_output(a) == os.path.join(session, "depths")
    a = Rn.parse_args(["--cloud", "g.ply", "--dense_folder", str(tmp_path / "d")])
    assert Rn.prepare_output(a) == os.path.join(str(tmp_path / "d"), "depths_mvsnet")
    assert Rn.parse_occlusion("1:0.1:2") == (1, 0.1, 2)
    for bad in ("1:0.1", "1:0.1:2:3", "a:0.1:2", "0:0.1:2", "1:0:2", "1:1:2", "1:0.1:0", "17:0.1:1", "1:nan:2"):
        with pytest.raises(ValueError):
            Rn.parse_occlusion(bad)
    for argv in (["--cloud", "g.ply"], ["--cloud", "g.ply", "--session", "a", "--dense_folder", "b"], ["--session", "a"],
                 ["--cloud", "g.ply", "--session", "a", "--occlusion", "1:2"], ["--cloud", "g.ply", "--session", "a", "--splat", "-1"],
                 ["--cloud", "g.ply", "--session", "a", "--min_depth", "-1"], ["--cloud", "g.ply", "--session", "a", "--cloud_scale", "0"]):
        with pytest.raises(SystemExit):
            Rn.parse_args(argv)
    assert Rn.occlusion_ratio(0.1) == float(np.float32(1.0 - 0.1))


def test_plan_arguments_are_checked_before_any_gpu_use():
    from mvsnet_amd import render as Rn
    p = np.zeros((4, 3), np.float32)
    cams = _hand_cam()
    for args, kw in (((p.astype(np.float64), cams, H, W), {}), ((p.reshape(3, 4), cams, H, W), {}), ((p[:0], cams, H, W), {}),
                     ((p, cams[0], H, W), {}), ((p, cams, 0, W), {}), ((p, cams, H, 2.5), {}),
                     ((p, cams, H, W), dict(splat=-1)), ((p, cams, H, W), dict(splat=33)), ((p, cams, H, W), dict(splat=1.5)),
                     ((p, cams, H, W), dict(min_depth=-1.0)), ((p, cams, H, W), dict(min_depth=float("nan"))),
                     ((p, cams, H, W), dict(occlusion=(0, 0.1, 1))), ((p, cams, H, W), dict(occlusion=(1, 1.0, 1))),
                     ((p, cams, H, W), dict(occlusion=(1, 0.1, 0))), ((p, cams, H, W), dict(occlusion=(1, 0.1))),
                     ((p, cams, H, W), dict(order="morton")), ((p, cams, H, W), dict(device="cpu"))):
        with pytest.raises(ValueError):
            Rn.RenderPlan(*args, **kw)


def test_entry_points_check_arguments_without_gpu(lib_built):
    from mvsnet_amd import _lib
    h = _lib.load()
    BADARG, SHAPE, WORKSPACE = -1, -2, -3
    wsb, wsb_occ = h.mvs_render_workspace_bytes(5, 40, 48, 0), h.mvs_render_workspace_bytes(5, 40, 48, 1)
    assert wsb >= 5 * 40 * 48 * 8 and wsb_occ >= wsb + 5 * 40 * 48 * 4
    assert h.mvs_render_workspace_bytes(0, 40, 48, 0) == 0 and h.mvs_render_workspace_bytes(5, -1, 48, 0) == 0
    assert h.mvs_render_workspace_bytes(5, 40, 0, 1) == 0 and h.mvs_render_workspace_bytes(1 << 12, 1 << 10, 1 << 10, 0) == 0
    assert h.mvs_render_workspace_bytes(1, 1, (1 << 24) + 1, 0) == 0 and h.mvs_render_workspace_bytes(1, 1, 1 << 24, 0) > 0
    nz = 4096                                  # never dereferenced: the checks return before any HIP call

    def call(**kw):
        a = dict(xyz=nz, n=100, order=None, proj=nz, V=5, H=40, W=48, splat=0, md=0.0, k=0, ratio=0.0, count=0, depth=nz, index=None,
                 ws=nz, wsb=wsb)
        a.update(kw)
        return h.mvs_render_points_f32(a["xyz"], a["n"], a["order"], a["proj"], a["V"], a["H"], a["W"], a["splat"], a["md"], a["k"],
                                       a["ratio"], a["count"], a["depth"], a["index"], a["ws"], a["wsb"], None)
    assert call(xyz=None) == BADARG and call(proj=None) == BADARG and call(depth=None) == BADARG and call(ws=None) == BADARG
    assert call(n=0) == BADARG and call(n=-5) == BADARG and call(V=0) == BADARG and call(H=0) == BADARG and call(W=-2) == BADARG
    assert call(splat=-1) == BADARG and call(splat=33) == BADARG
    assert call(md=-1.0) == BADARG and call(md=float("nan")) == BADARG and call(md=float("inf")) == BADARG
    occ = dict(k=1, ratio=0.9, count=2, wsb=wsb_occ)
    assert call(k=-1) == BADARG and call(**dict(occ, k=17)) == BADARG
    assert call(**dict(occ, ratio=0.0)) == BADARG and call(**dict(occ, ratio=1.0)) == BADARG
    assert call(**dict(occ, ratio=float("nan"))) == BADARG and call(**dict(occ, count=0)) == BADARG
    assert call(V=1 << 12, H=1 << 10, W=1 << 10) == SHAPE and call(V=1, H=1, W=(1 << 24) + 1) == SHAPE
    assert call(wsb=wsb - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
    assert call(**dict(occ, wsb=wsb)) == WORKSPACE and call(**dict(occ, wsb=wsb_occ - 1)) == WORKSPACE


def test_cli_without_gpu_fails_clearly(tmp_path):
    from mvsnet_amd import fusion as Fu
    session = make_session(str(tmp_path / "s"))
    Fu.write_ply(str(tmp_path / "a.ply"), np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    base = [sys.executable, "-m", "mvsnet_amd.render", "--cloud", str(tmp_path / "a.ply"), "--session", session]
    r = subprocess.run(base, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs a GPU" in r.stderr and "Traceback" not in r.stderr
    assert not os.path.exists(os.path.join(session, "depths"))
    r = subprocess.run(base + ["--occlusion", "1:0.1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "k:rel:count" in r.stderr and "Traceback" not in r.stderr
