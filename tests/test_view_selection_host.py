"""Host tests of the view selection (mvsnet_amd/select_views.py): the weight table, the float32 restatement of
tests/view_selection_reference.py against hand-computed pairs, its float64 twin and the continuous formula on the five-view
scene, the exact depth percentiles, the neighbour selection and the two files it writes.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

from mvsnet_amd import select_views as S
from tests import render_reference as R
from tests import view_selection_reference as VR
from tests._helpers import make_session

SIZES = ((40, 48), (37, 53))


def test_weight_table():
    t = S.weight_table()
    assert t.dtype == np.uint16 and t.shape == (8192,)
    assert np.array_equal(t, VR.weight_table())
    assert math.sin(math.radians(5.0)) * 8192 == pytest.approx(713.98, abs=0.01)
    assert int(t.max()) == 65535 and int(t.argmax()) == 713
    nz = np.nonzero(t)[0]
    assert nz[0] == 21 and nz[-1] == 6588 and len(nz) == 6588 - 21 + 1
    d = np.diff(t.astype(np.int64))
    assert (d[:713] >= 0).all() and (d[713:] <= 0).all() and t[712] < 65535


@pytest.mark.parametrize("theta0,sigma1,sigma2", [(10.0, 2.0, 5.0), (2.5, 0.5, 20.0), (20.0, 1.0, 3.0)])
def test_weight_table_with_other_parameters(theta0, sigma1, sigma2):
    t = S.weight_table(theta0, sigma1, sigma2)
    peak = int(math.floor(math.sin(math.radians(theta0)) * 8192))
    assert np.array_equal(t, VR.weight_table(theta0, sigma1, sigma2))
    top = np.nonzero(t == 65535)[0]                                            # wide sigmas round a run of bins to 65535
    assert t.max() == 65535 and top[0] <= peak <= top[-1] and len(top) == top[-1] - top[0] + 1
    d = np.diff(t.astype(np.int64))
    assert (d[:peak] >= 0).all() and (d[peak:] <= 0).all()
    with pytest.raises(ValueError):
        S.weight_table(theta0, 0.0, sigma2)


def _cam_at(centre):
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[0, :3, 3] = -np.asarray(centre, np.float64)
    cam[1, :3, :3] = np.eye(3)
    return cam


def test_hand_computed_pairs():
    t = S.weight_table()
    assert int(t[4915]) == 408
    a, b, obtuse = np.float32([5, 0, 0]), np.float32([4, 3, 0]), np.float32([-4, 3, 0])
    assert int(VR.pair_terms(a, b, t)) == 408                                   # dot 20, r 0.64, s 0.6, k 4915
    assert int(VR.pair_terms(a, obtuse, t)) == 0
    assert int(VR.pair_terms(np.float32([0, 0, 0]), b, t)) == 0                 # the point at c_a: 0 / 0
    cams = np.stack([_cam_at(a), _cam_at(b), _cam_at(obtuse)])
    assert np.array_equal(S.camera_centres(cams), np.stack([a, b, obtuse]))
    assert np.array_equal(VR.camera_centres(cams), S.camera_centres(cams))
    pts = np.float32([[0, 0, 0], [5, 0, 0]])
    vis = np.ones((2, 3), bool)
    score, shared = VR.pair_scores(pts, vis, cams, t)
    assert shared[0, 1] == shared[1, 0] == 2 and shared[0, 0] == 0              # the point at c_a counts as shared
    assert score[0, 1] == score[1, 0] == 408 and score[0, 2] == 0
    # second point (5,0,0): B = (-1,3,0), C = (-9,3,0): dot 18, r = 324 / 900 = 0.36, s = 0.8, k = 6553
    assert score[1, 2] == int(t[6553]) and shared[1, 2] == 2


@pytest.mark.parametrize("size", SIZES)
def test_scene_float64_twin_and_continuous_formula(size):
    pts, cams = R.scene_cloud()[0], VR.scene_cams(size)
    vis = VR.visibility(pts, cams, *size)
    assert np.array_equal(vis, VR.visibility(pts, cams, *size, dtype=np.float64))
    score, shared = VR.pair_scores(pts, vis, cams)
    cont = VR.continuous_scores(pts, vis, cams)
    iu = np.triu_indices(5, 1)
    err = np.abs(score / 65535.0 - cont)
    print("shared", shared[iu].min(), shared[iu].max(), "scores", (score[iu] / 65535.0).min(), (score[iu] / 65535.0).max(),
          "worst error per shared point %.3g" % (err[iu] / shared[iu]).max())
    assert (shared[iu] > 0).all() and (err <= 0.015 * shared).all()
    assert np.array_equal(score, score.T) and np.array_equal(shared, shared.T) and not np.diag(score).any()


def test_scene_literal_numbers():
    pts, cams = R.scene_cloud()[0], VR.scene_cams((40, 48))
    vis = VR.visibility(pts, cams, 40, 48)
    assert vis.sum(0).tolist() == [8809, 9012, 9072, 9019, 8829]
    lo, hi = VR.depth_ranges(pts, vis, cams)[2]
    assert lo == np.float32(3.2235289) and hi == np.float32(5.5)
    score, shared = VR.pair_scores(pts, vis, cams)
    iu = np.triu_indices(5, 1)
    assert 8000 <= shared[iu].min() and shared[iu].max() <= 8900
    assert 1366 <= (score[iu] / 65535.0).min() and (score[iu] / 65535.0).max() <= 8341
    mask = VR.pack_mask(vis)
    assert mask.shape == (9600, 1) and [int(((mask[:, 0] >> np.uint64(v)) & np.uint64(1)).sum()) for v in range(5)] == vis.sum(0).tolist()


def test_zbuffer_visibility_hides_the_plane_behind_the_sphere():
    pts, cams = R.scene_cloud()[0], VR.scene_cams((40, 48))
    front = VR.visibility(pts, cams, 40, 48)
    z = VR.zbuffer(pts, cams, 40, 48)
    vis = VR.visibility(pts, cams, 40, 48, zbuf=z)
    assert not (vis & ~front).any() and 0 < vis.sum() < front.sum()
    assert np.array_equal(vis, VR.visibility(pts, cams, 40, 48, zbuf=z, z_rel=0.01))
    assert VR.visibility(pts, cams, 40, 48, zbuf=z, z_rel=0.0).sum() <= vis.sum()
    assert S.z_tolerance(0.01) == float(np.float32(1.01))


@pytest.mark.parametrize("m", [0, 1, 2, 100])
def test_depth_range_equals_sorting(m):
    rs = np.random.RandomState(m)
    w = rs.uniform(1.0, 9.0, m).astype(np.float32)
    for lo, hi in ((1, 99), (0, 100), (50, 50), (25, 75)):
        got = VR.depth_range(w, lo, hi)
        if m == 0:
            assert got == (0, 0)
            continue
        s = np.sort(w)
        want = s[m * lo // 100], s[min(m - 1, m * hi // 100)]
        assert got == want
        assert VR.radix_select(w, m * lo // 100) == want[0] and VR.radix_select(w, min(m - 1, m * hi // 100)) == want[1]


def test_depth_range_with_ties_and_half_words():
    bits = lambda u: np.array(u, np.uint32).view(np.float32)
    cases = {"ties": np.float32([2.0] * 40 + [3.0] * 40 + [2.5] * 20),
             "low half only": bits([0x40000000 + k for k in range(100)]),
             "high half only": bits([0x40000000 + (k << 16) for k in range(100)]),
             "across a power of two": np.float32(np.linspace(1.5, 2.5, 100))}
    for name, w in cases.items():
        w = w[np.random.RandomState(1).permutation(len(w))]
        s = np.sort(w)
        for rank in (0, 1, 39, 40, 50, 98, 99):
            assert VR.radix_select(w, rank) == s[rank], (name, rank)
        assert VR.depth_range(w) == (s[1], s[99])


def test_selection():
    score = np.array([[0, 5, 9, 5, 0], [5, 0, 1, 2, 3], [9, 1, 0, 0, 7], [5, 2, 0, 0, 4], [0, 3, 7, 4, 0]], np.int64)
    shared = np.array([[0, 3, 3, 2, 9], [3, 0, 1, 1, 1], [3, 1, 0, 5, 2], [2, 1, 5, 0, 2], [9, 1, 2, 2, 0]], np.int64)
    assert S.select_neighbours(score, shared) == [[2, 1, 3], [0, 4, 3, 2], [0, 4, 1], [0, 4, 1], [2, 3, 1]]    # ties: 1 before 3
    assert S.select_neighbours(score, shared, num_views=2)[0] == [2, 1]
    assert S.select_neighbours(score, shared, min_shared=3)[0] == [2, 1]
    assert S.select_neighbours(score, shared, min_shared=2) == [[2, 1, 3], [0], [0, 4], [0, 4], [2, 3]]
    assert S.select_neighbours(score, shared, num_views=0) == [[], [], [], [], []]
    with pytest.raises(ValueError):
        S.select_neighbours(score, shared[:4])


def _session_result(session):
    from mvsnet_amd import render as Rn
    from tests import fusion_reference as F
    views = Rn.session_views(session)
    yy, xx = np.mgrid[0:48:1.0, 0:64:1.0]
    cloud = F._backproject(views[0][1], xx.reshape(-1), yy.reshape(-1), np.full(xx.size, 600.0)).astype(np.float32)
    cams = np.stack([v[1] for v in views])
    vis = VR.visibility(cloud, cams, 48, 64)
    score, shared = VR.pair_scores(cloud, vis, cams)
    return views, score, shared, VR.depth_ranges(cloud, vis, cams)


def test_covisibility_file_loads_through_the_generator(tmp_path):
    from mvsnet_amd.mvs_data_generation import make_generator
    session = make_session(str(tmp_path / "s"))
    os.remove(os.path.join(session, "covisibility.json"))
    views, score, shared, ranges = _session_result(session)
    indices = [v[0] for v in views]
    nb = S.select_neighbours(score, shared, num_views=2)
    assert all(len(x) == 2 for x in nb) and all(score[r, x[0]] >= score[r, x[1]] > 0 for r, x in enumerate(nb))
    out = os.path.join(session, "covisibility.json")
    S.write_covisibility(out, indices, nb, score, shared, ranges[:, 0], ranges[:, 1])
    data = json.load(open(out))
    assert sorted(data) == ["0", "1", "2", "3"] and sorted(data["0"]) == ["max_depth", "min_depth", "scores", "shared", "views"]
    assert data["0"]["scores"] == [score[0, b] / 65535.0 for b in nb[0]] and data["0"]["shared"] == [int(shared[0, b]) for b in nb[0]]
    gen = make_generator(session, view_num=3, image_width=64, image_height=64, depth_num=8, base_image_size=8)
    assert [c.ref_index for c in gen.clusters] == indices
    for c, r in zip(gen.clusters, range(4)):
        assert c.views == [indices[b] for b in nb[r]]
        assert np.float32(c.min_depth) == ranges[r, 0] and np.float32(c.max_depth) == ranges[r, 1]
        assert 590.0 < c.min_depth <= c.max_depth < 610.0


def test_pair_file_loads_through_the_pair_generator(tmp_path):
    from mvsnet_amd.mvs_data_generation import PairClusterGenerator
    score = np.array([[0, 65535, 3 * 65535], [65535, 0, 32768], [3 * 65535, 32768, 0]], np.int64)
    shared = np.where(score > 0, 7, 0)
    indices = [4, 7, 9]
    nb = S.select_neighbours(score, shared)
    assert S.pair_text(indices, nb, score) == "3\n4\n2 9 3.0000 7 1.0000\n7\n2 4 1.0000 9 0.5000\n9\n2 4 3.0000 7 0.5000\n"
    S.write_pair_txt(str(tmp_path / "pair.txt"), indices, nb, score)
    gen = PairClusterGenerator(str(tmp_path), view_num=3)
    assert [c.ref_index for c in gen.clusters] == indices
    assert [os.path.basename(p) for p in gen.clusters[0].paths[::2]] == ["00000004.jpg", "00000009.jpg", "00000007.jpg"]


def test_existing_output_is_refused_without_force(tmp_path):
    session = make_session(str(tmp_path / "s"))
    before = open(os.path.join(session, "covisibility.json")).read()
    args = ["--cloud", "c.ply", "--session", session]
    with pytest.raises(SystemExit, match="--force"):
        S.prepare_output(S.parse_args(args))
    with pytest.raises(SystemExit, match="--force"):
        S.main(args)
    assert open(os.path.join(session, "covisibility.json")).read() == before
    assert S.prepare_output(S.parse_args(args + ["--force"])) == os.path.join(session, "covisibility.json")
    assert S.prepare_output(S.parse_args(args + ["--format", "pair"])) == os.path.join(session, "pair.txt")
    a = S.parse_args(["--cloud", "c.ply", "--dense_folder", str(tmp_path), "--occlusion", "1:0.1:2", "--depth_percentiles", "5:95"])
    assert a.format == "pair" and a.occlusion == (1, 0.1, 2) and a.depth_percentiles == (5, 95)
    for bad in (["--depth_percentiles", "99:1"], ["--sigma1", "0"], ["--z_rel", "-1"], ["--occlusion", "1:2"]):
        with pytest.raises(SystemExit):
            S.parse_args(args + bad)
