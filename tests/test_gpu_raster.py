"""GPU tests of the triangle rasteriser (mvs_raster_mesh_f32 and mvs_raster_interpolate_f32 of csrc/raster.hip through
mvsnet_amd.render_mesh) against the restatement of tests/raster_reference.py, byte for byte: the TSDF scene meshes in five
views at two sizes, watertight and sub-pixel cases, the large path with its queue and the overflow fallback, independence of
the processing order, dropped faces, ties, contention on one pixel, culling, attribute interpolation, argument errors and the
command line end to end."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import raster_reference as RR
from tests import render_reference as R
from tests._helpers import make_session

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"40x48": (40, 48), "37x53": (37, 53)}
GUARD_WORDS = 64


@functools.lru_cache(maxsize=None)
def _scene_reference(kind, size):
    H, W = SIZES[size]
    verts, _, faces, cams = RR.scene_mesh(kind)
    cams = R.scale_cams(cams, 40, 48, H, W)
    return cams, RR.render(verts, faces, cams, H, W)


@functools.lru_cache(maxsize=None)
def _mixed():
    verts, faces = RR.mixed_mesh()
    return verts, faces, RR.render(verts, faces, RR.pixel_cam(40, 48), 40, 48)


def _device(verts, faces, cams, H, W, order="plan", **kw):
    from mvsnet_amd import render_mesh as RM
    plan = RM.RasterPlan(verts, faces, cams, H, W, **kw)
    d, i = plan.run(order=order)
    return d.cpu().numpy(), i.cpu().numpy()


def _assert_same(got, want):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[0].shape == want[0].shape
    nd, ni = int((got[0].view(np.int32) != want[0].view(np.int32)).sum()), int((got[1] != want[1]).sum())
    print("pixels that differ: depth %d, index %d of %d" % (nd, ni, want[1].size))
    assert nd == 0 and ni == 0


def _queued(plan):
    """The queue counter as the last run left it: the (face, view) pairs that asked for the large path."""
    return int(plan.workspace[:8].cpu().numpy().view(np.uint64)[0])


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("kind", ["plane", "step", "sphere"])
def test_scene_mesh_in_five_views_equals_the_reference(kind, size):
    H, W = SIZES[size]
    verts, _, faces, _ = RR.scene_mesh(kind)
    assert 7000 <= len(faces) <= 8000
    cams, want = _scene_reference(kind, size)
    assert (want[1] >= 0).mean() > 0.1
    _assert_same(_device(verts, faces, cams, H, W), want)


def test_vertex_aligned_grid():
    verts, faces = RR.aligned_grid()
    want = RR.render(verts, faces, RR.pixel_cam(40, 48), 40, 48)
    assert (want[2][0, 1:33, 1:33] == 1).all() and want[2].sum() == 32 * 32
    for f in (faces, np.ascontiguousarray(faces[:, ::-1])):
        _assert_same(_device(verts, f, RR.pixel_cam(40, 48), 40, 48), RR.render(verts, f, RR.pixel_cam(40, 48), 40, 48))


def test_sub_pixel_triangles():
    verts, faces = RR.subpixel_soup()
    want = RR.render(verts, faces, RR.pixel_cam(40, 48), 40, 48)
    hit = len(np.unique(want[1])) - 1
    assert 50 < hit < len(faces) // 4                                           # most cover no pixel, some cover one
    _assert_same(_device(verts, faces, RR.pixel_cam(40, 48), 40, 48), want)


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (64, 3), (65, 9)])
def test_off_screen_quad(size):
    H, W = size
    verts, faces = RR.offscreen_quad()
    want = RR.render(verts, faces, RR.pixel_cam(H, W), H, W)
    assert (want[2] == 1).all() and (want[0] == 2.0).all()
    for lp in (0, 1 << 30):
        _assert_same(_device(verts, faces, RR.pixel_cam(H, W), H, W, large_pixels=lp), want)


def test_large_path_queue_and_overflow_never_change_a_byte():
    from mvsnet_amd import render_mesh as RM
    verts, faces, want = _mixed()
    cam = RR.pixel_cam(40, 48)
    s = RR.face_setup(*RR.project_vertices(R.projection_tables(cam)[0], verts), faces, 40, 48)
    boxes = ((s["x1"] - s["x0"] + 1) * (s["y1"] - s["y0"] + 1))[s["valid"]]
    assert (boxes > RM.LARGE_PIXELS).sum() == 2 and (boxes <= RM.LARGE_PIXELS).sum() > 200
    ample = len(faces)
    plan = RM.RasterPlan(verts, faces, cam, 40, 48, queue_capacity=ample)
    for lp in (0, RM.LARGE_PIXELS, 1 << 30):
        for qc in (0, 1, ample):
            d, i = plan.run(large_pixels=lp, queue_capacity=qc)
            _assert_same((d.cpu().numpy(), i.cpu().numpy()), want)
            if qc:                                                             # every pair over the threshold asked for a slot
                assert _queued(plan) == int((boxes > lp).sum())
    d, i = RM.RasterPlan(verts, faces, cam, 40, 48).run()                      # the defaults
    _assert_same((d.cpu().numpy(), i.cpu().numpy()), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 3130])
def test_order_and_launch_shape_never_change_a_byte(n):
    import torch
    from mvsnet_amd import render_mesh as RM
    verts, faces, _ = _mixed()
    faces = np.ascontiguousarray(faces[len(faces) - n:])                       # the last n: the quad and its neighbours
    cams = R.scale_cams(np.repeat(RR.pixel_cam(40, 48), 3, 0), 40, 48, 37, 53)
    want = RR.render(verts, faces, cams, 37, 53)
    plan = RM.RasterPlan(verts, faces, cams, 37, 53)
    assert n == 1 or (plan.order is not None and sorted(plan.order.cpu().tolist()) == list(range(n)))
    rs = np.random.RandomState(n)
    orders = [None, "plan"] + [torch.as_tensor(rs.permutation(n).astype(np.int32)).to(plan.dev) for _ in range(2)]
    for o in orders + ["plan"]:                                                # the plan's order twice: two runs of one plan
        d, i = plan.run(order=o)
        _assert_same((d.cpu().numpy(), i.cpu().numpy()), want)
    plain = RM.RasterPlan(verts, faces, cams, 37, 53, order=None)
    assert plain.order is None
    plain.depth.fill_(-1.0)
    plain.index.fill_(-7)
    side = torch.cuda.Stream(device=plain.dev)
    side.wait_stream(torch.cuda.current_stream(plain.dev))
    with torch.cuda.stream(side):
        plain.enqueue()
    side.synchronize()
    _assert_same((plain.depth.cpu().numpy(), plain.index.cpu().numpy()), want)


def test_a_mesh_beyond_one_sweep_of_the_grid():
    """550 000 faces: more than the 2048 x 256 lanes of the fixed grid, so lanes stride and one chunk holds all views.  Every
    copy of a face ties with the first, so the answer is the single mesh's."""
    verts, _, faces, _ = RR.scene_mesh("sphere")
    cams, want = _scene_reference("sphere", "40x48")
    big = np.tile(faces, (72, 1))
    assert len(big) > 2048 * 256
    _assert_same(_device(verts, big, cams, 40, 48), want[:2])


def _raw(verts, faces, cam, H, W, *, min_depth=0.0, cull=0, lp=256, qc=16, M=None, F=None, order=None, override=None):
    """Calls mvs_raster_mesh_f32 on buffers with guard words on both sides -> (rc, depth, index, guards intact)."""
    import torch
    from mvsnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    g = GUARD_WORDS

    def padded(a):
        a = np.ascontiguousarray(a)
        raw = np.full(a.size + 2 * g, 0x5A5A5A5A, np.uint32)
        raw[g:g + a.size] = a.reshape(-1).view(np.uint32)
        return torch.as_tensor(raw.view(np.int32)).to(dev)

    pix = H * W
    wsb = lib.mvs_raster_workspace_bytes(1, H, W, qc)
    tv, tf = padded(np.asarray(verts, np.float32)), padded(np.asarray(faces, np.int32))
    tp = padded(R.projection_tables(cam).reshape(-1))
    td, ti = padded(np.full(pix, -1.0, np.float32)), padded(np.full(pix, -7, np.int32))
    tw = padded(np.zeros(wsb // 4, np.int32))
    to = padded(np.asarray(order, np.int32)) if order is not None else None
    bufs = [tv, tf, tp, td, ti, tw] + ([to] if to is not None else [])
    before = [b.cpu().numpy().copy() for b in bufs]
    at = lambda t: t.data_ptr() + 4 * g
    a = dict(vertices=at(tv), M=len(verts) if M is None else M, faces=at(tf), F=len(faces) if F is None else F,
             order=at(to) if to is not None else None, proj=at(tp), V=1, H=H, W=W, md=min_depth, cull=cull, lp=lp, qc=qc,
             depth=at(td), index=at(ti), ws=at(tw), wsb=wsb)
    a.update(override or {})
    rc = lib.mvs_raster_mesh_f32(a["vertices"], a["M"], a["faces"], a["F"], a["order"], a["proj"], a["V"], a["H"], a["W"], a["md"],
                                 a["cull"], a["lp"], a["qc"], a["depth"], a["index"], a["ws"], a["wsb"], _lib.stream_ptr())
    torch.cuda.synchronize()
    after = [b.cpu().numpy() for b in bufs]
    intact = all(np.array_equal(x[:g], y[:g]) and np.array_equal(x[-g:], y[-g:]) for x, y in zip(before, after))
    inputs_same = all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3]))
    depth = after[3][g:-g].view(np.float32).reshape(1, H, W)
    return rc, depth, after[4][g:-g].reshape(1, H, W), intact and inputs_same


def _dropped_case():
    """Four good triangles (faces 0..3) and, after each, faces that must be dropped -> (verts, faces, good face ids)."""
    nan, inf = float("nan"), float("inf")
    good = RR.soup([[[2, 2], [12, 3], [4, 11]], [[20, 4], [40, 6], [30, 20]], [[5, 22], [18, 24], [9, 36]], [[26, 25], [44, 28], [33, 37]]],
                   [2.0, 2.5, 3.0, 3.5])
    tri = np.array([[10.0, 10.0], [30.0, 12.0], [18.0, 30.0]])                 # would cover the middle of the image, in front
    P = lambda z=1.5: RR.at_pixel(tri[:, 0], tri[:, 1], z)
    bad = []
    line = RR.at_pixel([8, 16, 24], [8, 16, 24], 1.5)                          # zero area: three corners on a line
    bad.append(line)
    rep = P(); rep[2] = rep[0]; bad.append(rep)                                # a repeated corner (another zero area)
    for k, val in ((0, nan), (1, inf), (2, -inf)):
        p = P(); p[k, k] = val; bad.append(p)
    p = P(); p[0] = [0.0, 0.0, -1.0]; bad.append(p)                            # w < 0
    p = P(); p[1] = [0.0, 0.0, 0.0]; bad.append(p)                             # w = 0
    p = P(0.9); bad.append(p)                                                  # 0 < w <= min_depth = 1
    p = P(); p[2] = [1.5 * 2.0 ** 20 + 1e5, 0.0, 1.5]; bad.append(p)           # x = 2^20 + 6.7e4 pixels: beyond 2^28 / 256
    verts = np.concatenate([good[0]] + [b.astype(np.float32) for b in bad])
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    idx = np.array([[0, 1, -1], [len(verts), 1, 2], [3, 4, 2 ** 31 - 1]], np.int32)        # vertex indices outside 0..M-1
    faces = np.concatenate([faces, idx])
    return verts, faces, [0, 1, 2, 3]


def test_dropped_faces_draw_nothing_and_guards_stay_intact():
    verts, faces, good = _dropped_case()
    cam = RR.pixel_cam(40, 48)
    want = RR.render(verts, faces, cam, 40, 48, min_depth=1.0)
    only_good = RR.render(verts, faces[good], cam, 40, 48, min_depth=1.0)
    assert np.array_equal(want[0], only_good[0]) and np.array_equal(want[1], only_good[1]) and (want[1] >= 0).sum() > 300
    for lp in (0, 256):
        rc, depth, index, intact = _raw(verts, faces, cam, 40, 48, min_depth=1.0, lp=lp)
        assert rc == 0 and intact
        _assert_same((depth, index), want)
    # without min_depth the face at depth 0.9 is drawn, in front of the others
    rc, depth, index, intact = _raw(verts, faces, cam, 40, 48)
    assert rc == 0 and intact and (index == len(good) + 7).sum() > 100
    _assert_same((depth, index), RR.render(verts, faces, cam, 40, 48))
    # an order that is no permutation: its bad entries are left out, nothing is read through them
    order = np.arange(len(faces), dtype=np.int32)
    order[5], order[6] = -1, len(faces)
    rc, depth, index, intact = _raw(verts, faces, cam, 40, 48, min_depth=1.0, order=order)
    assert rc == 0 and intact
    _assert_same((depth, index), want)


def test_a_duplicated_face_resolves_to_the_smallest_index():
    verts, faces, want = _mixed()
    got = _device(verts, np.concatenate([faces, faces]), RR.pixel_cam(40, 48), 40, 48)
    assert (got[1] < len(faces)).all()
    _assert_same(got, want)


def test_four_thousand_faces_on_one_pixel():
    verts, faces, z = RR.one_pixel_stack()
    cam = RR.pixel_cam(6, 8)
    want = RR.render(verts, faces, cam, 6, 8)
    first = int(np.nonzero(z == 1.0)[0].min())
    assert want[2][0, 3, 4] == 4096 and want[2].sum() == 4096 and want[1][0, 3, 4] == first and want[0][0, 3, 4] == 1.0
    for order in (None, "plan"):
        for lp in (0, 256):
            _assert_same(_device(verts, faces, cam, 6, 8, order=order, large_pixels=lp), want)


def test_culling():
    cam = RR.pixel_cam(40, 48)
    verts, faces = RR.soup([[[5, 5], [30, 8], [12, 30]]], [2.0])
    s = RR.face_setup(*RR.project_vertices(R.projection_tables(cam)[0], verts), faces, 40, 48)
    assert s["area2"][0] > 0                                                    # screen-positive: its normal points away
    for f, positive in ((faces, True), (np.ascontiguousarray(faces[:, ::-1]), False)):
        for cull in (None, "back", "front"):
            got = _device(verts, f, cam, 40, 48, cull=cull)
            drawn = cull is None or (cull == "back") != positive
            assert bool((got[1] >= 0).any()) == drawn
            _assert_same(got, RR.render(verts, f, cam, 40, 48, cull=cull))
    sv, sf = RR.uv_sphere()
    cams = R.scene("sphere")["cams"]
    both, back = _device(sv, sf, cams, 40, 48), _device(sv, sf, cams, 40, 48, cull="back")
    assert np.array_equal(both[0].view(np.int32), back[0].view(np.int32)) and (both[0] > 0).sum() > 1000
    _assert_same(back, RR.render(sv, sf, cams, 40, 48, cull="back"))
    _assert_same(_device(sv, sf, cams, 40, 48, cull="front"), RR.render(sv, sf, cams, 40, 48, cull="front"))


def test_interpolation_of_constants_world_positions_and_colours():
    from mvsnet_amd import render_mesh as RM
    verts, rgb, faces, _ = RR.scene_mesh("step")
    cams, want = _scene_reference("step", "37x53")
    H, W = SIZES["37x53"]
    plan = RM.RasterPlan(verts, faces, cams, H, W)
    depth, index = (x.cpu().numpy() for x in plan.run())
    _assert_same((depth, index), want)
    covered = index >= 0
    one = plan.interpolate(np.ones((len(verts), 1), np.float32)).cpu().numpy()
    assert one.shape == (5, H, W, 1) and (one[covered] == 1.0).all() and (one[~covered] == 0.0).all()
    # world positions as attributes (eight channels: the positions, their negatives, two constants) project back onto their
    # own pixel.  The bound is 4 x the reference's own worst distance, which is the 1/512 pixel of the snap seen through
    # the face's slope
    attr = np.concatenate([verts, -verts, np.full((len(verts), 2), 3.0, np.float32)], 1)
    ref = RR.interpolate(verts, faces, cams, H, W, index, attr)
    got = plan.interpolate(attr).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), ref.view(np.int32))

    def worst(x):
        P = R.projection_tables(cams).astype(np.float64)
        X = np.concatenate([x[..., :3].astype(np.float64), np.ones(x.shape[:3] + (1,))], -1)
        uvw = np.einsum("vrk,vhwk->vhwr", P, X)
        yy, xx = np.mgrid[0:H, 0:W]
        with np.errstate(all="ignore"):
            d = np.hypot(uvw[..., 0] / uvw[..., 2] - xx, uvw[..., 1] / uvw[..., 2] - yy)
        return float(d[covered].max())
    bound = 4 * worst(ref)
    print("worst distance of a projected position from its pixel: device %.3g, reference %.3g" % (worst(got), worst(ref)))
    assert worst(got) <= bound < 0.1
    col = plan.colors(rgb).cpu().numpy()
    assert col.shape == (5, H, W, 3) and col.dtype == np.uint8 and col[covered].any()
    assert np.array_equal(col, RR.colors(verts, faces, cams, H, W, index, rgb))
    for bad in (attr[:-1], np.ones((len(verts), 9), np.float32), attr.astype(np.float64), np.ones(len(verts), np.float32)):
        with pytest.raises(ValueError):
            plan.interpolate(bad)


def test_argument_errors_leave_the_outputs_untouched():
    verts, faces = RR.aligned_grid(3)
    cam = RR.pixel_cam(6, 8)
    rc, depth, index, intact = _raw(verts, faces, cam, 6, 8)
    assert rc == 0 and intact and (index >= 0).any()
    for kw in (dict(vertices=None), dict(faces=None), dict(proj=None), dict(depth=None), dict(ws=None), dict(M=0), dict(F=0), dict(V=0),
               dict(H=0), dict(W=-1), dict(md=-1.0), dict(md=float("nan")), dict(md=float("inf")), dict(cull=2), dict(cull=-2),
               dict(lp=-1), dict(qc=-1), dict(H=(1 << 20) + 1), dict(V=1 << 12, H=1 << 10, W=1 << 10), dict(wsb=64), dict(qc=4096)):
        rc, depth, index, intact = _raw(verts, faces, cam, 6, 8, override=kw)
        assert rc in (-1, -2, -3) and intact, kw
        assert (depth == -1.0).all() and (index == -7).all(), kw


def test_interpolate_argument_errors_leave_the_output_untouched():
    import torch
    from mvsnet_amd import _lib
    from mvsnet_amd import render_mesh as RM
    verts, faces = RR.aligned_grid(3)
    plan = RM.RasterPlan(verts, faces, RR.pixel_cam(6, 8), 6, 8)
    plan.run()
    attr = torch.ones((len(verts), 2), dtype=torch.float32, device=plan.dev)
    out = torch.full((1, 6, 8, 2), -3.0, dtype=torch.float32, device=plan.dev)
    lib = _lib.load()

    def call(**kw):
        a = dict(vertices=_lib.ptr(plan.vertices), M=plan.M, faces=_lib.ptr(plan.faces), F=plan.F, proj=_lib.ptr(plan.proj), V=1, H=6,
                 W=8, md=0.0, index=_lib.ptr(plan.index), attr=_lib.ptr(attr), C=2, out=_lib.ptr(out))
        a.update(kw)
        rc = lib.mvs_raster_interpolate_f32(a["vertices"], a["M"], a["faces"], a["F"], a["proj"], a["V"], a["H"], a["W"], a["md"],
                                            a["index"], a["attr"], a["C"], a["out"], _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    for kw in (dict(vertices=None), dict(faces=None), dict(proj=None), dict(index=None), dict(attr=None), dict(M=0), dict(F=0), dict(V=0),
               dict(H=0), dict(W=-1), dict(md=-1.0), dict(md=float("nan")), dict(C=0), dict(C=9), dict(H=(1 << 20) + 1),
               dict(V=1 << 12, H=1 << 10, W=1 << 10)):
        assert call(**kw) in (-1, -2) and bool((out == -3.0).all()), kw
    assert call(out=None) == -1
    assert call() == 0
    covered = (plan.index >= 0).cpu().numpy()
    got = out.cpu().numpy()
    assert covered.any() and (got[covered] == 1.0).all() and (got[~covered] == 0.0).all()


def _write_mesh(path, verts, rgb, faces):
    from mvsnet_amd import mesh as Me
    Me.write_mesh_ply(path, verts, rgb, faces)


def test_command_line_draws_a_session(tmp_path):
    from PIL import Image
    from mvsnet_amd import render as Rn
    session = make_session(str(tmp_path / "s"))
    views = Rn.session_views(session)
    cams = np.stack([v[1] for v in views])
    # a wall at 600 mm that overfills view 0, in metres: --mesh_scale 1000 brings it to the session's millimetres
    from tests import fusion_reference as F
    corners = F._backproject(views[0][1], np.array([-40.0, 120, 120, -40]), np.array([-30.0, -30, 90, 90]), np.full(4, 600.0))
    verts, faces = (corners / 1000.0).astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    rgb = np.array([[250, 10, 10], [10, 250, 10], [10, 10, 250], [200, 200, 200]], np.uint8)
    ply = str(tmp_path / "m.ply")
    _write_mesh(ply, verts, rgb, faces)
    cmd = [sys.executable, "-m", "mvsnet_amd.render_mesh", "--mesh", ply, "--mesh_scale", "1000", "--session", session, "--write_index",
           "--write_color"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert report["faces"] == 2 and report["vertices"] == 4 and report["views"] == 4
    scaled = (verts.astype(np.float64) * 1000.0).astype(np.float32)
    want_d, want_i, _ = RR.render(scaled, faces, cams, 48, 64)
    want_c = RR.colors(scaled, faces, cams, 48, 64, want_i, rgb)
    assert report["covered_pixels"] == int((want_i >= 0).sum())
    for i in range(4):
        png = np.asarray(Image.open(os.path.join(session, "depths", "%d.png" % i)))
        assert png.dtype == np.uint16 and np.array_equal(png, Rn.depth_to_png16(want_d[i]))
        assert np.array_equal(np.load(os.path.join(session, "depths", "%d_index.npy" % i)), want_i[i])
        assert np.array_equal(np.asarray(Image.open(os.path.join(session, "depths", "%d_color.png" % i))), want_c[i])
    assert (np.asarray(Image.open(os.path.join(session, "depths", "0.png"))) == 600).all()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)      # depths/ exists now
    assert r.returncode != 0 and "--force" in r.stderr and "Traceback" not in r.stderr


def test_command_line_draws_a_dense_folder(tmp_path):
    from mvsnet_amd import preprocess as pp
    verts, rgb, faces, cams = RR.scene_mesh("plane")
    sc = R.scene("plane")
    out = str(tmp_path / "dense" / "depths_mvsnet")
    os.makedirs(out)
    for i in range(3):
        pp.write_pfm(os.path.join(out, "%d_init.pfm" % (i + 4)), sc["depths"][i])
        pp.write_cam(os.path.join(out, "%d.txt" % (i + 4)), sc["cams"][i].copy())
    ply = str(tmp_path / "m.ply")
    _write_mesh(ply, verts, rgb, faces)
    cmd = [sys.executable, "-m", "mvsnet_amd.render_mesh", "--mesh", ply, "--dense_folder", str(tmp_path / "dense"), "--suffix", "mesh",
           "--cull", "back"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.loads(r.stdout.strip().splitlines()[-1])
    assert report["faces"] == len(faces) and report["groups"] == [{"height": 40, "width": 48, "views": [4, 5, 6]}]
    loaded = np.stack([pp.load_cam(os.path.join(out, "%d.txt" % (i + 4))) for i in range(3)])
    want = RR.render(verts, faces, loaded, 40, 48, cull="back")
    for i in range(3):
        got = pp.load_pfm(os.path.join(out, "%d_mesh.pfm" % (i + 4)))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want[0][i].view(np.int32))
    assert (want[0] > 0).mean() > 0.25
