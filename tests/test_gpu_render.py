"""GPU tests of the point-cloud rendering (mvs_render_points_f32 of csrc/render.hip through mvsnet_amd.render) against the
float32 restatement of tests/render_reference.py, byte for byte: a five-view cloud at two sizes and three splat radii, round
trips through one view, contention on one pixel, independence of the processing order and of the launch shape, culling, the
hidden-point filter, and the command line end to end."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_reference as F
from tests import render_reference as R
from tests._helpers import make_session

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"40x48": (40, 48), "37x53": (37, 53)}


def _cams(size):
    H, W = SIZES[size]
    return R.scale_cams(R.scene_cloud()[1], 40, 48, H, W)


@functools.lru_cache(maxsize=None)
def _reference(size, splat, twin=False, min_depth=0.0, occlusion=None, every=1):
    H, W = SIZES[size]
    return R.render(R.scene_cloud()[0][::every], _cams(size), H, W, splat=splat, min_depth=min_depth, occlusion=occlusion,
                    dtype=np.float64 if twin else np.float32)


def _device(points, cams, H, W, order="plan", **kw):
    from mvsnet_amd import render as Rn
    plan = Rn.RenderPlan(points, cams, H, W, **kw)
    d, i = plan.run(order=order)
    return d.cpu().numpy(), i.cpu().numpy()


def _assert_same(got, want):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[0].shape == want[0].shape
    nd, ni = int((got[0].view(np.int32) != want[0].view(np.int32)).sum()), int((got[1] != want[1]).sum())
    print("pixels that differ: depth %d, index %d of %d" % (nd, ni, want[1].size))
    assert nd == 0 and ni == 0


@pytest.mark.parametrize("splat", [0, 1, 2])
@pytest.mark.parametrize("size", list(SIZES))
def test_cloud_of_five_views_equals_the_float32_reference(size, splat):
    H, W = SIZES[size]
    cloud = R.scene_cloud()[0]
    assert cloud.shape == (9600, 3) and cloud.dtype == np.float32
    _assert_same(_device(cloud, _cams(size), H, W, splat=splat), _reference(size, splat))


@pytest.mark.parametrize("splat", [0, 1, 2])
def test_float32_and_float64_references_choose_the_same_points(splat):
    """On this cloud at 40 x 48 the two statements chose the same index at every one of the 9 600 pixels for all three radii;
    a change of scene that breaks this is to be noticed.  (At 37 x 53 the scaled principal point puts rows of points exactly
    on rounding boundaries, and the two differ on about 1.5 % of the pixels.)"""
    a, b = _reference("40x48", splat), _reference("40x48", splat, twin=True)
    assert a[1].size == 9600 and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["plane", "step", "sphere"])
def test_round_trip_through_one_view(kind):
    sc = R.scene(kind)
    # 16 x the float32 reference's own worst relative error against the scene's float64 depths, measured at 1.2e-7 on these
    # scenes (plane and step 1.18e-7, sphere 0.94e-7)
    bound = 16 * 1.2e-7
    for v in range(5):
        d64 = sc["depths"][v].astype(np.float64)
        pts, pix = R.backproject(sc["cams"][v], d64)
        depth, index = _device(pts.astype(np.float32), sc["cams"][v:v + 1], 40, 48)
        depth, index = depth.reshape(-1), index.reshape(-1)
        assert np.array_equal(index[pix], np.arange(len(pix)))                 # every pixel returns its own point
        empty = np.ones(40 * 48, bool)
        empty[pix] = False
        assert (index[empty] == -1).all() and (depth[empty] == 0).all()        # empty pixels stay empty
        err = np.abs(depth[pix].astype(np.float64) - d64.reshape(-1)[pix]) / d64.reshape(-1)[pix]
        print(kind, v, "worst relative depth error %.3g (bound %.3g)" % (err.max(), bound))
        assert err.max() <= bound


def _one_pixel_cam():
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[1, :3, :3] = [[2.0, 0, 4.0], [0, 2.0, 3.0], [0, 0, 1.0]]
    return cam[None]


def test_ten_thousand_points_on_one_pixel():
    rs = np.random.RandomState(5)
    z = np.float32(1.0) + np.arange(1, 9951, dtype=np.float32) * np.float32(1e-3)
    assert len(np.unique(z)) == 9950 and z.min() > 1.0
    z = np.concatenate([z, np.full(50, 1.0, np.float32)])[rs.permutation(10000)]
    pts = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
    first = int(np.nonzero(z == 1.0)[0].min())
    for order in (None, "plan"):
        depth, index = _device(pts, _one_pixel_cam(), 6, 8, order=order)
        assert (index >= 0).sum() == 1 and depth[0, 3, 4] == 1.0 and index[0, 3, 4] == first
    _assert_same((depth, index), R.render(pts, _one_pixel_cam(), 6, 8))


def test_a_cloud_concatenated_with_itself_keeps_the_first_copy():
    cloud = R.scene_cloud()[0]
    got = _device(np.concatenate([cloud, cloud]), _cams("40x48"), 40, 48, splat=1)
    assert (got[1] < len(cloud)).all()
    _assert_same(got, _reference("40x48", 1))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 9600])
def test_order_and_launch_shape_never_change_a_byte(n):
    import torch
    from mvsnet_amd import render as Rn
    cloud = R.scene_cloud()[0][:n]
    want = R.render(cloud, _cams("37x53"), 37, 53, splat=1)
    plan = Rn.RenderPlan(cloud, _cams("37x53"), 37, 53, splat=1)
    assert n == 1 or (plan.order is not None and sorted(plan.order.cpu().tolist()) == list(range(n)))
    rs = np.random.RandomState(n)
    orders = [None, "plan"] + [torch.as_tensor(rs.permutation(n).astype(np.int32)).to(plan.dev) for _ in range(2)]
    for o in orders + ["plan"]:                                                # the plan's order twice: two runs of one plan
        d, i = plan.run(order=o)
        _assert_same((d.cpu().numpy(), i.cpu().numpy()), want)
    plain = Rn.RenderPlan(cloud, _cams("37x53"), 37, 53, splat=1, order=None)
    assert plain.order is None
    d, i = plain.run()
    _assert_same((d.cpu().numpy(), i.cpu().numpy()), want)


def test_a_cloud_beyond_one_sweep_of_the_grid():
    """528 000 points: more than the 2048 x 256 lanes of the fixed grid, so lanes stride, and one chunk holds all views (a
    small cloud spreads the views over blockIdx.y).  Every copy of a point ties with the first, so the answer is the single
    cloud's."""
    cloud = R.scene_cloud()[0]
    big = np.tile(cloud, (55, 1))
    assert len(big) > 2048 * 256
    from mvsnet_amd import render as Rn
    for order in ("voxel", None):
        d, i = Rn.RenderPlan(big, _cams("40x48"), 40, 48, order=order).run()
        _assert_same((d.cpu().numpy(), i.cpu().numpy()), _reference("40x48", 0))


def test_culling():
    cloud = R.scene_cloud()[0]
    away = np.array(_cams("40x48")[:1])
    away[0, 0, :3, :] = np.diag([-1.0, 1.0, -1.0]) @ away[0, 0, :3, :]         # the camera turned away: every w < 0
    depth, index = _device(cloud, away, 40, 48, splat=2)
    assert (depth == 0).all() and (index == -1).all()
    # non-finite and huge coordinates cover nothing and disturb nothing
    nan, inf = float("nan"), float("inf")
    junk = np.array([[nan, 0, 4], [0, inf, 4], [0, 0, -inf], [1e38, 1e38, 4.0], [1e30, -1e30, 4.0], [nan, nan, nan]], np.float32)
    mixed = np.concatenate([junk, cloud])
    want = R.render(mixed, _cams("40x48"), 40, 48, splat=1)
    assert want[1].min() == -1 or want[1][want[1] >= 0].min() >= len(junk)
    _assert_same(_device(mixed, _cams("40x48"), 40, 48, splat=1), want)
    _assert_same(_device(junk, _cams("40x48"), 40, 48, splat=1, order=None), R.render(junk, _cams("40x48"), 40, 48, splat=1))
    # min_depth between the sphere (depth < 4.0 in every view) and the plane (> 4.9) removes exactly the sphere's pixels
    got = _device(cloud, _cams("40x48"), 40, 48, min_depth=4.5)
    want, raw = _reference("40x48", 0, min_depth=4.5), _reference("40x48", 0)
    _assert_same(got, want)
    sphere = (raw[0] > 0) & (raw[0] <= 4.5)
    assert sphere.any() and np.array_equal(got[0] != raw[0], sphere) and not ((got[0] > 0) & (got[0] <= 4.5)).any()


def test_two_layer_case_with_the_occlusion_filter():
    pts, cams, front = R.two_layer()
    raw = _device(pts, cams, 24, 32)
    _assert_same(raw, R.render(pts, cams, 24, 32))
    got = _device(pts, cams, 24, 32, occlusion=(1, 0.1, 2))
    _assert_same(got, R.render(pts, cams, 24, 32, occlusion=(1, 0.1, 2)))
    removed = (raw[0] > 0) & (got[0] == 0)
    assert not (got[0][0, 1:-1, 1:15] == 800).any() and (got[0][0][front] == 500).all() and not removed[0, :, 17:].any()
    assert int(removed.sum()) == R.TWO_LAYER_REMOVED


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("size", list(SIZES))
def test_occlusion_filter_on_a_thinned_cloud(size, k):
    H, W = SIZES[size]
    cloud = R.scene_cloud()[0][::2]
    want = _reference(size, 0, occlusion=(k, 0.1, 2), every=2)
    raw = _reference(size, 0, every=2)
    print("pixels the filter removes:", int(((raw[0] > 0) & (want[0] == 0)).sum()))
    _assert_same(_device(cloud, _cams(size), H, W, occlusion=(k, 0.1, 2)), want)


def test_occlusion_off_and_a_filter_that_removes_nothing():
    cloud = R.scene_cloud()[0][::2]
    want = _reference("37x53", 0, every=2)
    _assert_same(_device(cloud, _cams("37x53"), 37, 53, occlusion=None), want)
    # eight neighbours can never be nine: the filter's path, the raw map's bytes
    _assert_same(_device(cloud, _cams("37x53"), 37, 53, occlusion=(1, 0.1, 9)), want)


def test_index_null_colors_and_a_side_stream():
    import torch
    from mvsnet_amd import render as Rn
    cloud = R.scene_cloud()[0]
    want = _reference("37x53", 1)
    plan = Rn.RenderPlan(cloud, _cams("37x53"), 37, 53, splat=1)
    plan.index.fill_(-7)
    plan.depth.fill_(-1.0)
    plan.enqueue(index=False)                                                  # index passed as NULL: depth unchanged
    assert np.array_equal(plan.depth.cpu().numpy().view(np.int32), want[0].view(np.int32))
    assert (plan.index.cpu().numpy() == -7).all()
    d, i = plan.run()
    _assert_same((d.cpu().numpy(), i.cpu().numpy()), want)
    rgb = np.random.RandomState(3).randint(1, 256, (len(cloud), 3)).astype(np.uint8)
    col = plan.colors(rgb).cpu().numpy()
    ref = np.where((want[1] >= 0)[..., None], rgb[np.maximum(want[1], 0)], 0).astype(np.uint8)
    assert col.shape == (5, 37, 53, 3) and col.dtype == np.uint8 and np.array_equal(col, ref)
    plan.depth.fill_(-1.0)
    plan.index.fill_(-7)
    side = torch.cuda.Stream(device=plan.dev)
    side.wait_stream(torch.cuda.current_stream(plan.dev))
    with torch.cuda.stream(side):
        plan.enqueue()
    side.synchronize()
    _assert_same((plan.depth.cpu().numpy(), plan.index.cpu().numpy()), want)
    one = Rn.render_depth_maps(cloud, _cams("37x53"), 37, 53, splat=1)
    _assert_same(one, want)


def test_command_line_renders_a_session_that_the_test_mode_reads(tmp_path):
    from mvsnet_amd import fusion as Fu
    from mvsnet_amd import render as Rn
    from mvsnet_amd.mvs_data_generation import make_generator
    session = make_session(str(tmp_path / "s"))
    views = Rn.session_views(session)
    yy, xx = np.mgrid[0:48:0.5, 0:64:0.5]                                      # a plane at 600 mm, four points per pixel of view 0
    cloud = F._backproject(views[0][1], xx.reshape(-1), yy.reshape(-1), np.full(xx.size, 600.0)).astype(np.float32)
    ply = str(tmp_path / "g.ply")
    Fu.write_ply(ply, cloud, np.zeros((len(cloud), 3), np.uint8))
    cmd = [sys.executable, "-m", "mvsnet_amd.render", "--cloud", ply, "--session", session, "--write_index"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert report["points"] == len(cloud) and report["views"] == 4
    want_d, want_i = R.render(cloud, np.stack([v[1] for v in views]), 48, 64)
    from PIL import Image
    for i in range(4):
        png = np.asarray(Image.open(os.path.join(session, "depths", "%d.png" % i)))
        assert png.dtype == np.uint16 and np.array_equal(png, Rn.depth_to_png16(want_d[i]))
        assert np.array_equal(np.load(os.path.join(session, "depths", "%d_index.npy" % i)), want_i[i])
    assert (np.asarray(Image.open(os.path.join(session, "depths", "0.png"))) == 600).all()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)      # depths/ exists now
    assert r.returncode != 0 and "--force" in r.stderr and "Traceback" not in r.stderr
    gen = make_generator(session, view_num=3, image_width=64, image_height=64, depth_num=8, base_image_size=8, mode="test",
                         output_scale=0.25)
    depth = gen.prepare(gen.clusters[0])[5]
    assert depth.shape == (64, 64, 1) and (depth > 0).any() and set(np.unique(depth[depth > 0]).astype(int)) == {600}
