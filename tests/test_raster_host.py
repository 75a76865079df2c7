"""CPU tests of the triangle rasteriser (mvsnet_amd/render_mesh.py): the numpy restatement of tests/raster_reference.py on
cases with known answers (watertight coverage, a closed sphere, an analytic plane, the TSDF scene meshes), the option and
argument checks of the module and of the mvs_raster entry points (no GPU call), and the depth file writers behind the
command line."""
import os

import numpy as np
import pytest

from tests import mesh_reference as MR
from tests import raster_reference as RR
from tests import render_reference as R
from tests._helpers import make_session

H, W = 40, 48


def test_vertex_aligned_grid_is_covered_exactly_once():
    verts, faces = RR.aligned_grid(n=9, step=4)
    depth, index, count = RR.render(verts, faces, RR.pixel_cam(H, W), H, W, check=True)      # check: e_a + e_b + e_c == |area2|
    want = np.zeros((H, W), np.int64)
    want[1:33, 1:33] = 1                                                        # the half-open square (0, 32]^2
    assert np.array_equal(count[0], want)
    assert np.array_equal(index[0] >= 0, want == 1) and (depth[0][want == 1] == 2.0).all() and (depth[0][want == 0] == 0).all()
    # the same mesh with every face turned over: the same pixels, once each
    _, _, flipped = RR.render(verts, faces[:, ::-1], RR.pixel_cam(H, W), H, W, check=True)
    assert np.array_equal(flipped[0], want)


def test_closed_sphere_is_covered_twice_and_culling_keeps_the_front():
    verts, faces = RR.uv_sphere()
    assert MR.signed_volume(verts, faces) > 0                                   # wound outward
    topo = MR.mesh_topology(faces)
    assert topo["manifold"] and topo["oriented"]
    cams = R.scene("sphere")["cams"]
    depth, index, count = RR.render(verts, faces, cams, H, W, check=True)
    assert set(np.unique(count)) == {0, 2} and (count == 2).sum() > 1000
    back, _, back_count = RR.render(verts, faces, cams, H, W, cull="back")
    assert np.array_equal(back.view(np.int32), depth.view(np.int32)) and set(np.unique(back_count)) == {0, 1}
    front, _, front_count = RR.render(verts, faces, cams, H, W, cull="front")
    assert np.array_equal(front_count, back_count) and (front[count == 2] > depth[count == 2]).all()


def test_constant_attribute_comes_back_as_exactly_one():
    verts, _, faces, cams = RR.scene_mesh("sphere")
    depth, index, _ = RR.render(verts, faces, cams, H, W)
    one = RR.interpolate(verts, faces, cams, H, W, index, np.ones((len(verts), 2), np.float32))
    assert one.shape == (5, H, W, 2) and one.dtype == np.float32
    assert (one[index >= 0] == 1.0).all() and (one[index < 0] == 0.0).all() and (index >= 0).sum() > 1000
    # an index that names no face, or a face that is dropped in the view, gives 0
    bad = np.full_like(index, len(faces))
    assert (RR.interpolate(verts, faces, cams, H, W, bad, np.ones((len(verts), 1), np.float32)) == 0).all()


def test_tilted_analytic_plane():
    """z = 3 + 0.3 x seen with f = 50: the snap moves a vertex by at most 1/512 pixel, so the relative depth error is about
    slope / (512 f) = 1.17e-5.  The reference measured 1.235e-5 on this plane; the bound is 4 x that, the margin being for
    other planes of the same slope."""
    f = 50.0
    cam = R.identity_cam(H, W, f)
    n = 13
    X, Y = np.meshgrid(np.linspace(-2.2, 2.2, n), np.linspace(-1.9, 1.9, n))
    verts = np.stack([X.ravel(), Y.ravel(), 3 + 0.3 * X.ravel()], 1).astype(np.float32)
    quads = [(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i) for j in range(n - 1) for i in range(n - 1)]
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    depth, _, count = RR.render(verts, faces, cam[None], H, W)
    assert (count == 1).all()
    want = 3.0 / (1.0 - 0.3 * (np.arange(W)[None, :] - cam[1, 0, 2]) / f) + np.zeros((H, 1))
    err = float((np.abs(depth[0].astype(np.float64) - want) / want).max())
    print("worst relative depth error %.4g" % err)
    assert err <= 4 * 1.235e-5


# median relative difference between the rasterised TSDF mesh and the scene's own depth maps on the covered pixels, as the
# reference measured it (the TSDF mesh's error, not the rasteriser's; worst pixels 3.4e-4 and, at the step, 2.5e-2)
SCENE_MEDIAN = {"plane": 9.906e-5, "step": 1.435e-4}


@pytest.mark.parametrize("kind", ["plane", "step"])
def test_scene_mesh_agrees_with_the_scene_depth_maps(kind):
    verts, _, faces, cams = RR.scene_mesh(kind)
    depth, index, _ = RR.render(verts, faces, cams, H, W)
    ref = MR.scene(kind)["depths"].astype(np.float64)
    both = (depth > 0) & (ref > 0)
    assert both.mean() > 0.25
    rel = np.abs(depth.astype(np.float64) - ref)[both] / ref[both]
    print(kind, "median %.4g worst %.4g" % (np.median(rel), rel.max()))
    assert np.median(rel) <= 2 * SCENE_MEDIAN[kind]


def test_options_and_plan_arguments_are_checked_before_any_gpu_use():
    from mvsnet_amd import render_mesh as RM
    assert RM.check_options() == (0.0, 0, RM.LARGE_PIXELS, RM.QUEUE_CAPACITY)
    assert RM.check_options(2.5, "back", 0, 0) == (2.5, 1, 0, 0) and RM.check_options(cull="front")[1] == -1
    for kw in (dict(min_depth=-1.0), dict(min_depth=float("nan")), dict(min_depth=float("inf")), dict(min_depth=1e39),
               dict(cull="left"), dict(cull=1), dict(large_pixels=-1), dict(large_pixels=1.5), dict(large_pixels=True),
               dict(queue_capacity=-1), dict(queue_capacity=2 ** 31), dict(queue_capacity=None)):
        with pytest.raises(ValueError):
            RM.check_options(**kw)
    v, f = RR.aligned_grid(3)
    cams = RR.pixel_cam(H, W)
    for args, kw in (((v.astype(np.float64), f, cams, H, W), {}), ((v, f.astype(np.int64), cams, H, W), {}),
                     ((v.reshape(-1, 9), f, cams, H, W), {}), ((v, f.reshape(-1, 2), cams, H, W), {}), ((v[:0], f, cams, H, W), {}),
                     ((v, f[:0], cams, H, W), {}), ((v, f, cams[0], H, W), {}), ((v, f, cams, 0, W), {}), ((v, f, cams, H, 2.5), {}),
                     ((v, f, cams, H, (1 << 20) + 1), {}), ((v, f, cams, H, W), dict(min_depth=-1.0)),
                     ((v, f, cams, H, W), dict(cull="both")), ((v, f, cams, H, W), dict(large_pixels=-1)),
                     ((v, f, cams, H, W), dict(queue_capacity=-3)), ((v, f, cams, H, W), dict(order="morton")),
                     ((v, f, cams, H, W), dict(device="cpu"))):
        with pytest.raises(ValueError):
            RM.RasterPlan(*args, **kw)


def test_entry_points_check_arguments_without_gpu(lib_built):
    from mvsnet_amd import _lib
    h = _lib.load()
    BADARG, SHAPE, WORKSPACE = -1, -2, -3
    wsb0, wsb = h.mvs_raster_workspace_bytes(5, 40, 48, 0), h.mvs_raster_workspace_bytes(5, 40, 48, 100)
    assert wsb0 >= 5 * 40 * 48 * 8 + 8 and wsb >= wsb0 + 800
    for bad in ((0, 40, 48, 0), (5, -1, 48, 0), (5, 40, 0, 0), (5, 40, 48, -1), (1 << 12, 1 << 10, 1 << 10, 0), (1, 1, (1 << 20) + 1, 0)):
        assert h.mvs_raster_workspace_bytes(*bad) == 0
    assert h.mvs_raster_workspace_bytes(1, 1, 1 << 20, 0) > 0
    nz = 4096                                  # never dereferenced: the checks return before any HIP call

    def mesh(**kw):
        a = dict(vertices=nz, M=10, faces=nz, F=10, order=None, proj=nz, V=5, H=40, W=48, md=0.0, cull=0, lp=256, qc=100, depth=nz,
                 index=None, ws=nz, wsb=wsb)
        a.update(kw)
        return h.mvs_raster_mesh_f32(a["vertices"], a["M"], a["faces"], a["F"], a["order"], a["proj"], a["V"], a["H"], a["W"], a["md"],
                                     a["cull"], a["lp"], a["qc"], a["depth"], a["index"], a["ws"], a["wsb"], None)
    for kw in (dict(vertices=None), dict(faces=None), dict(proj=None), dict(depth=None), dict(ws=None), dict(M=0), dict(F=0), dict(F=-4),
               dict(V=0), dict(H=0), dict(W=-2), dict(md=-1.0), dict(md=float("nan")), dict(md=float("inf")), dict(cull=2),
               dict(cull=-2), dict(lp=-1), dict(qc=-1)):
        assert mesh(**kw) == BADARG, kw
    assert mesh(V=1 << 12, H=1 << 10, W=1 << 10) == SHAPE and mesh(V=1, H=1, W=(1 << 20) + 1) == SHAPE
    assert mesh(wsb=wsb - 1) == WORKSPACE and mesh(wsb=0) == WORKSPACE and mesh(qc=200) == WORKSPACE and mesh(qc=0, wsb=wsb0 - 1) == WORKSPACE

    def interp(**kw):
        a = dict(vertices=nz, M=10, faces=nz, F=10, proj=nz, V=5, H=40, W=48, md=0.0, index=nz, attr=nz, C=3, out=nz)
        a.update(kw)
        return h.mvs_raster_interpolate_f32(a["vertices"], a["M"], a["faces"], a["F"], a["proj"], a["V"], a["H"], a["W"], a["md"],
                                            a["index"], a["attr"], a["C"], a["out"], None)
    for kw in (dict(vertices=None), dict(faces=None), dict(proj=None), dict(index=None), dict(attr=None), dict(out=None), dict(M=0),
               dict(F=0), dict(V=0), dict(H=0), dict(W=0), dict(md=-1.0), dict(md=float("nan")), dict(C=0), dict(C=9)):
        assert interp(**kw) == BADARG, kw
    assert interp(V=1 << 12, H=1 << 10, W=1 << 10) == SHAPE and interp(V=1, H=(1 << 20) + 1, W=1) == SHAPE


def test_cli_parsing_force_rule_and_depth_file_writers(tmp_path):
    from PIL import Image
    from mvsnet_amd import render as Rn
    from mvsnet_amd import render_mesh as RM
    from mvsnet_amd.preprocess import load_pfm
    session = make_session(str(tmp_path / "s"))
    a = RM.parse_args(["--mesh", "m.ply", "--session", session, "--cull", "back", "--min_depth", "10", "--write_index", "--write_color",
                       "--mesh_scale", "1000"])
    assert a.cull == "back" and a.min_depth == 10.0 and a.write_index and a.write_color and a.mesh_scale == 1000.0
    assert a.dense_folder is None and a.transform is None and not a.force and a.suffix == "gt"
    out = RM.prepare_output(a)
    assert out == os.path.join(session, "depths") and RM.output_stem(a, out, 3) == os.path.join(out, "3")
    depth = np.array([[0.0, 0.49, 0.5, 1.49], [1.5, 599.5, 65535.49, 65535.5]], np.float32)
    index = np.arange(8, dtype=np.int32).reshape(2, 4) - 1
    color = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    os.makedirs(out)
    RM.write_view(a, RM.output_stem(a, out, 3), depth, index, color)
    assert sorted(os.listdir(out)) == ["3.png", "3_color.png", "3_index.npy"]
    png = np.asarray(Image.open(os.path.join(out, "3.png")))
    assert png.dtype == np.uint16 and np.array_equal(png, Rn.depth_to_png16(depth)) and png[1, 1] == 600
    assert np.array_equal(np.load(os.path.join(out, "3_index.npy")), index)
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "3_color.png"))), color)
    with pytest.raises(SystemExit, match="--force"):                           # depths/ exists now
        RM.prepare_output(a)
    a = RM.parse_args(["--mesh", "m.ply", "--session", session, "--force"])
    assert a.cull is None and a.min_depth == 0.0 and RM.prepare_output(a) == out
    dense = str(tmp_path / "d")
    a = RM.parse_args(["--mesh", "m.ply", "--dense_folder", dense, "--suffix", "mesh"])
    out = RM.prepare_output(a)
    assert out == os.path.join(dense, "depths_mvsnet") and RM.output_stem(a, out, 7) == os.path.join(out, "7_mesh")
    os.makedirs(out)
    RM.write_view(a, RM.output_stem(a, out, 7), depth)
    assert os.listdir(out) == ["7_mesh.pfm"] and np.array_equal(load_pfm(os.path.join(out, "7_mesh.pfm")), depth)
    for argv in (["--mesh", "m.ply"], ["--mesh", "m.ply", "--session", "a", "--dense_folder", "b"], ["--session", "a"],
                 ["--mesh", "m.ply", "--session", "a", "--cull", "both"], ["--mesh", "m.ply", "--session", "a", "--min_depth", "-1"],
                 ["--mesh", "m.ply", "--session", "a", "--mesh_scale", "0"], ["--mesh", "m.ply", "--dense_folder", "a", "--suffix", "init"],
                 ["--mesh", "m.ply", "--dense_folder", "a", "--suffix", "x/y"]):
        with pytest.raises(SystemExit):
            RM.parse_args(argv)
