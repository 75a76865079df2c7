"""Host tests of the TSDF fusion and surface-nets semantics (tests/mesh_reference.py, the numpy restatement that the GPU must
equal) and of the host side of mvsnet_amd.mesh: topology and accuracy on an analytic sphere and on the ray-cast scenes, hand
cases, the effect of the consistency masks, PLY round trip, volume choice and argument checks.  No GPU is needed."""
import ctypes
import importlib
import os
import pkgutil

import numpy as np
import pytest

from tests import fusion_reference as F
from tests import mesh_reference as M


# ------------------------------------------------------------------------------------------------ analytic sphere

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_analytic_sphere_is_a_closed_outward_surface(dtype):
    m = M.extract(M.analytic_sphere(dtype))
    topo = M.mesh_topology(m["faces"])
    assert len(m["vertices"]) == 1212 and len(m["faces"]) == 2420
    assert topo["manifold"] and topo["oriented"]
    assert topo["V"] == 1212 and topo["V"] - topo["E"] + topo["F"] == 2
    vol = M.signed_volume(m["vertices"], m["faces"])
    sphere = 4.0 / 3.0 * np.pi * M.SPHERE_RADIUS ** 3
    worst = np.abs(np.linalg.norm(m["vertices"].astype(np.float64), axis=1) - M.SPHERE_RADIUS).max() / M.SPHERE_VOXEL
    print("signed volume %.6f (sphere %.6f), worst |r - 0.8| = %.5f voxels" % (vol, sphere, worst))
    # measured: volume 2.106666 against 2.144661 (a deficit of 0.037995: vertices are means of chord points, which lie
    # inside), worst distance 0.044982 voxels; the bounds are twice the measured values
    assert vol > 0 and abs(vol - sphere) <= 2 * 0.037995
    assert worst <= 2 * 0.044982


def test_float32_and_float64_sphere_agree_on_cells_and_faces():
    a, b = M.extract(M.analytic_sphere(np.float32)), M.extract(M.analytic_sphere(np.float64))
    assert np.array_equal(a["active"], b["active"]) and np.array_equal(a["faces"], b["faces"])
    assert np.abs(a["vertices"].astype(np.float64) - b["vertices"]).max() < 1e-5


# ------------------------------------------------------------------------------------------------ hand cases

def _block(dims, inside=(), value=-1.0):
    vol = M.new_volume((0, 0, 0), 1.0, dims, 4.0, colour=True)
    vol["sum"][...] = 1.0
    vol["count"][...] = 1
    for (i, j, k) in inside:
        vol["sum"][k, j, i] = value
    return vol


def test_one_face_giving_edge_of_a_block_of_two_cells_a_side():
    """Node q = (0, 1, 1) alone is inside a 3 x 3 x 3 volume: only its edge towards +x has four cells around it."""
    m = M.extract(_block((3, 3, 3), [(0, 1, 1)]))
    assert np.nonzero(m["active"])[0].tolist() == [0, 2, 4, 6]
    assert m["faces"].tolist() == [[0, 1, 3], [0, 3, 2]]                      # q is inside: (c0, c1, c2), (c0, c2, c3)
    third = np.float32(1.0) / np.float32(3.0)
    # cell (0,0,0) sees q at its corner (0,1,1): crossings (0.5,1,1), (0,0.5,1), (0,1,0.5)
    np.testing.assert_allclose(m["vertices"][0], [0.5 * third, 2.5 * third, 2.5 * third], rtol=0, atol=2e-7)
    np.testing.assert_allclose(m["vertices"][3], [0.5 * third, 1 + 0.5 * third, 1 + 0.5 * third], rtol=0, atol=2e-7)
    # the same edge seen from the outside end: q outside, its neighbour inside -> the other winding
    vol = _block((3, 3, 3), [(i, j, k) for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (0, 1, 1)])
    m2 = M.extract(vol)
    assert m2["faces"].tolist() == [[0, 3, 1], [0, 2, 3]]
    n = np.cross(m["vertices"][1] - m["vertices"][0], m["vertices"][3] - m["vertices"][0])
    assert n[0] > 0 and abs(n[1]) < 1e-6 and abs(n[2]) < 1e-6                  # from inside (q) towards +x, outside


def test_a_node_with_value_zero_is_outside():
    m = M.extract(_block((3, 3, 3), [(0, 1, 1)], value=0.0))
    assert len(m["vertices"]) == 0 and len(m["faces"]) == 0 and not m["active"].any()
    m = M.extract(_block((3, 3, 3), [(0, 1, 1)], value=-0.0))
    assert len(m["vertices"]) == 0
    # next to an inside node the zero node is the outside end: tau = f_A / (f_A - 0) = 1
    vol = _block((2, 2, 2), [(0, 0, 0)])
    for (i, j, k) in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        vol["sum"][k, j, i] = 0.0
    m = M.extract(vol)
    np.testing.assert_allclose(m["vertices"], [[1 / 3.0, 1 / 3.0, 1 / 3.0]], rtol=0, atol=1e-7)


def test_an_unobserved_corner_kills_its_cell_and_the_faces_round_it():
    vol = _block((3, 3, 3), [(0, 1, 1)])
    vol["count"][0, 0, 1] = 0                                                  # node (1, 0, 0), a corner of cell (0, 0, 0) only
    m = M.extract(vol)
    assert np.nonzero(m["active"])[0].tolist() == [2, 4, 6] and len(m["faces"]) == 0
    vol["count"][0, 0, 1] = 2                                                  # observed twice: enough for min_count 2 only
    assert len(M.extract(vol, min_count=2)["faces"]) == 0                      # every other node has count 1
    vol["count"][...] = 2
    assert len(M.extract(vol, min_count=2)["faces"]) == 2 and len(M.extract(vol, min_count=3)["faces"]) == 0


@pytest.mark.parametrize("dims", [(1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1)])
def test_an_axis_of_one_node_gives_no_cells(dims):
    vol = _block(dims, [(0, 0, 0)])
    m = M.extract(vol)
    assert m["vertices"].shape == (0, 3) and m["colours"].shape == (0, 3) and m["faces"].shape == (0, 3) and m["active"].size == 0


def test_colour_rounds_half_up_over_the_eight_corners():
    vol = _block((2, 2, 2), [(0, 0, 0)])
    vol["rgb_sum"][0, 0, 0] = [3, 5, 255]
    vol["rgb_count"][0, 0, 0] = 1
    vol["rgb_sum"][1, 1, 1] = [0, 0, 255]
    vol["rgb_count"][1, 1, 1] = 1
    # R = (3, 5, 510), n = 2 -> (6 + 2) // 4, (10 + 2) // 4, (1020 + 2) // 4
    assert M.extract(vol)["colours"].tolist() == [[2, 3, 255]]
    vol["rgb_count"][...] = 0
    vol["rgb_sum"][...] = 0
    assert M.extract(vol)["colours"].tolist() == [[0, 0, 0]]


def test_integration_by_hand():
    """One camera at the origin looking along +Z, f = 2, a 4 x 4 map of depth 2: nodes on the optical axis."""
    cam = np.zeros((1, 2, 4, 4))
    cam[0, 0] = np.eye(4)
    cam[0, 1, :3, :3] = [[2.0, 0, 1.5], [0, 2.0, 1.5], [0, 0, 1.0]]
    depth, prob = np.full((1, 4, 4), 2.0, np.float32), np.ones((1, 4, 4), np.float32)
    img = np.zeros((1, 8, 8, 3), np.uint8)
    img[0, 5, 5] = [10, 20, 30]                                                # pixel (2, 2) -> ((2 * 2 + 1) * 8) // 8 = 5
    vol = M.new_volume((0.25, 0.25, 1.0), 0.5, (1, 1, 5), 0.5, colour=True)    # z = 1, 1.5, 2, 2.5, 3; pixel (0.5/z*2+1.5+.5)
    M.integrate(vol, depth, prob, cam, img)
    # sdf = 1, 0.5, 0, -0.5, -1: t = min(sdf / 0.5, 1) = 1, 1, 0, -1 and the last is dropped (sdf < -trunc)
    assert vol["sum"].reshape(-1).tolist() == [1.0, 1.0, 0.0, -1.0, 0.0] and vol["count"].reshape(-1).tolist() == [1, 1, 1, 1, 0]
    # colour only where sdf <= trunc; u/w + 0.5 = 0.5/z + 2: pixel 2 for every z >= 1
    assert vol["rgb_count"].reshape(-1).tolist() == [0, 1, 1, 1, 0] and vol["rgb_sum"][2, 0, 0].tolist() == [10, 20, 30]
    # a second call continues the sums; a pixel below the probability threshold, NaN, inf or negative adds nothing
    for bad in (np.nan, np.inf, -2.0, 0.0):
        d2 = depth.copy()
        d2[0, 2, 2] = bad
        before = vol["sum"].copy()
        M.integrate(vol, d2, prob, cam, img)
        assert np.array_equal(vol["sum"], before)
    M.integrate(vol, depth, prob * 0.5, cam, img)
    assert np.array_equal(vol["sum"], before)
    M.integrate(vol, depth, prob, cam, img)
    assert vol["sum"].reshape(-1).tolist() == [2.0, 2.0, 0.0, -2.0, 0.0] and vol["count"].reshape(-1).tolist() == [2, 2, 2, 2, 0]


# ------------------------------------------------------------------------------------------------ scenes

SCENE_COUNTS = {"plane": (3713, 7176), "sphere": (4274, 7648), "step": (3948, 7544)}


@pytest.mark.parametrize("kind", ["plane", "sphere", "step"])
def test_scene_meshes(kind):
    a, b = M.scene_mesh(kind), M.scene_mesh(kind, twin=True)
    assert (len(a["vertices"]), len(a["faces"])) == SCENE_COUNTS[kind]
    assert np.array_equal(a["active"], b["active"]) and np.array_equal(a["faces"], b["faces"])
    assert a["vertices"].dtype == np.float32 and a["faces"].dtype == np.int32 and a["faces"].min() >= 0
    assert a["faces"].max() < len(a["vertices"])
    dist = M.scene(kind)["surface_distance"](a["vertices"]) / M.SCENE_VOXEL
    print(kind, "vertex distance in voxels: median %.4f p95 %.4f worst %.4f" % (np.median(dist), np.percentile(dist, 95), dist.max()))
    if kind == "plane":
        assert dist.max() <= 2 * 0.028105                  # measured 0.028105
        # the winding faces the cameras, which look along +Z: normals point towards -Z
        v, f = a["vertices"].astype(np.float64), a["faces"]
        nz = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])[:, 2]
        assert (nz < 0).all()
    if kind == "sphere":
        # measured median 0.035381, p95 0.456214, worst 1.455996 (the worst is at the occlusion edge, where the sphere's
        # silhouette and the plane behind it share a truncation band)
        assert np.median(dist) <= 2 * 0.035381 and np.percentile(dist, 95) <= 2 * 0.456214 and dist.max() <= 2 * 1.455996
    # the step: byte checks only (the TSDF bridges the step)


def test_scene_colours_come_from_the_images():
    a = M.scene_mesh("plane", colour=True)
    assert np.array_equal(a["vertices"], M.scene_mesh("plane")["vertices"])
    assert a["colours"].std() > 5 and 100 < a["colours"].mean() < 156          # means of random bytes


def test_two_calls_equal_one_call():
    sc = M.scene("sphere")
    vol = M.new_volume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, M.SCENE_TRUNC, colour=True)
    M.integrate(vol, sc["depths"][:3], sc["probs"][:3], sc["cams"][:3], sc["images"][:3])
    M.integrate(vol, sc["depths"][3:], sc["probs"][3:], sc["cams"][3:], sc["images"][3:])
    one = M.scene_volume("sphere", colour=True)
    for key in ("sum", "count", "rgb_sum", "rgb_count"):
        assert np.array_equal(vol[key], one[key]), key


# ------------------------------------------------------------------------------------------------ the filter matters

def _far_vertices(kind, masked):
    sc = M.scene(kind, noisy=True)
    depths = sc["depths"]
    if masked:
        keep = F.reference_fusion(sc["depths"], sc["probs"], sc["cams"], num_consistent=3, dedupe=False)["keep"]
        depths = np.where(keep, depths, np.float32(0))
    vol = M.new_volume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, M.SCENE_TRUNC)
    m = M.extract(M.integrate(vol, depths, sc["probs"], sc["cams"]))
    used = np.unique(m["faces"])
    dist = sc["surface_distance"](m["vertices"][used]) / M.SCENE_VOXEL
    return int((dist > 2).sum()), float(dist.max())


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_consistency_masks_remove_the_outliers_the_probability_filter_lets_through(kind):
    """5 % of view 2's depths are corrupt at full probability.  Measured: unmasked 34 (plane) and 66 (sphere) face-referenced
    vertices farther than 2 voxels from the surface, worst 36 and 8.8 voxels; masked none, worst 0.06 and 0.86."""
    far, worst = _far_vertices(kind, masked=False)
    far_m, worst_m = _far_vertices(kind, masked=True)
    print(kind, "unmasked: %d far, worst %.3f; masked: %d far, worst %.3f" % (far, worst, far_m, worst_m))
    assert far > 0 and far_m == 0


# ------------------------------------------------------------------------------------------------ host side of the module

def test_ply_round_trip_and_evaluation_reader(tmp_path):
    from mvsnet_amd import evaluate, mesh
    m = M.scene_mesh("plane", colour=True)
    path = str(tmp_path / "mesh.ply")
    mesh.write_mesh_ply(path, m["vertices"], m["colours"], m["faces"])
    v, c, f = mesh.read_mesh_ply(path)
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    assert np.array_equal(v, m["vertices"]) and np.array_equal(c, m["colours"]) and np.array_equal(f, m["faces"])
    size = os.path.getsize(path)
    assert size == len(mesh.MESH_PLY_HEADER % (len(v), len(f))) + 15 * len(v) + 13 * len(f)
    pts, cols = evaluate.read_ply_points(path)                                  # a mesh evaluates as a cloud
    assert np.array_equal(np.asarray(pts, np.float32), m["vertices"])
    empty = str(tmp_path / "empty.ply")
    mesh.write_mesh_ply(empty, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert [len(a) for a in mesh.read_mesh_ply(empty)] == [0, 0, 0]
    with pytest.raises(ValueError):
        mesh.write_mesh_ply(path, m["vertices"][:10], m["colours"][:10], m["faces"])
    with pytest.raises(ValueError):
        mesh.write_mesh_ply(path, m["vertices"], m["colours"][:10], m["faces"])
    with open(path, "ab") as fh:
        fh.write(b"x")
    with pytest.raises(ValueError):
        mesh.read_mesh_ply(path)


def test_choose_volume():
    from mvsnet_amd import mesh
    o, s, d = mesh.choose_volume([0, 0, 0], [1, 2, 3], resolution=31)
    assert o.dtype == np.float64 and o.tolist() == [0, 0, 0] and s == pytest.approx(0.1) and d == (11, 21, 31)
    o, s, d = mesh.choose_volume([0, 0, 0], [1, 2, 3], voxel=0.1, margin_voxels=5)
    assert o.tolist() == [-0.5, -0.5, -0.5] and s == 0.1 and d == (21, 31, 41)
    o, s, d = mesh.choose_volume([0, 0, 0], [1, 2, 3], resolution=41, margin_voxels=5)
    assert s == pytest.approx(0.1) and d == (21, 31, 41) and np.allclose(o, -0.5)
    o, s, d = mesh.choose_volume([1, 1, 1], [1, 1, 3], voxel=0.5, margin=0.25)
    assert o.tolist() == [0.75, 0.75, 0.75] and d == (2, 2, 6)
    # the volume covers the widened box
    for hi in ([1, 2, 3], [0.95, 2.04, 2.96]):
        o, s, d = mesh.choose_volume([0, 0, 0], hi, voxel=0.1, margin=0.07)
        assert (o + s * (np.array(d) - 1) >= np.array(hi) + 0.07 - 1e-9).all()
    for bad in (dict(lo=[0, 0, 0], hi=[1, 1, -1]), dict(lo=[0, 0], hi=[1, 1, 1]), dict(lo=[0, 0, 0], hi=[1, 1, np.inf]),
                dict(lo=[0, 0, 0], hi=[1, 1, 1], voxel=0), dict(lo=[0, 0, 0], hi=[1, 1, 1], voxel=-1.0),
                dict(lo=[0, 0, 0], hi=[1, 1, 1], resolution=1), dict(lo=[0, 0, 0], hi=[1, 1, 1], margin=-1),
                dict(lo=[0, 0, 0], hi=[1, 1, 1], resolution=8, margin_voxels=4), dict(lo=[0, 0, 0], hi=[0, 0, 0]),
                dict(lo=[0, 0, 0], hi=[1, 1, 1], voxel=1e-4)):
        with pytest.raises(ValueError):
            mesh.choose_volume(**bad)


def test_argument_checks_come_before_any_gpu_work(tmp_path):
    from mvsnet_amd import mesh
    good = dict(origin=(0, 0, 0), voxel=0.1, dims=(4, 4, 4), trunc=0.4)
    o, s, d, t = mesh.check_volume(**good)
    assert o.dtype == np.float32 and d == (4, 4, 4) and s == float(np.float32(0.1)) and t == float(np.float32(0.4))
    for key, bad in (("origin", (0, 0)), ("origin", (0, np.nan, 0)), ("origin", (0, 0, 1e39)), ("voxel", 0), ("voxel", -1),
                     ("voxel", np.inf), ("voxel", np.nan), ("trunc", 0), ("trunc", np.nan), ("dims", (4, 4)), ("dims", (4, 0, 4)),
                     ("dims", (4, 4.5, 4)), ("dims", 7), ("dims", (2048, 2048, 512)), ("dims", (True, 4, 4))):
        with pytest.raises(ValueError):
            mesh.check_volume(**dict(good, **{key: bad}))
        with pytest.raises(ValueError):
            mesh.TsdfVolume(**dict(good, **{key: bad}))                        # a ValueError with or without a GPU
    assert mesh.check_volume((0, 0, 0), 1.0, (2047, 1024, 1024), 1.0)[2] == (2047, 1024, 1024)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            mesh.check_min_count(bad)
    assert mesh.check_min_count(3) == 3
    z = np.zeros((2, 4, 4), np.float32)
    cams = np.zeros((2, 2, 4, 4))
    for kw in (dict(voxel=0.1, resolution=64), dict(trunc_voxels=0), dict(min_count=0), dict(trunc_voxels=np.nan)):
        with pytest.raises(ValueError):
            mesh.mesh_depth_maps(z, z, cams, **kw)
    assert mesh._check_views(z, z, cams, None) == (2, 4, 4)
    for args in ((z, z[:1], cams, None), (z[0], z[0], cams, None), (z, z, cams[:1], None), (z, z, cams, np.zeros((2, 4, 4), np.uint8)),
                 (z, z, cams, np.zeros((1, 4, 4, 3), np.uint8))):
        with pytest.raises(ValueError):
            mesh._check_views(*args)
    lo, hi = mesh.parse_bounds("0:0:0:1:2:3.5")
    assert lo.tolist() == [0, 0, 0] and hi.tolist() == [1, 2, 3.5]
    for bad in ("0:0:0:1:2", "a:0:0:1:2:3", "0:0:0:1:2:0", "0:0:0:1:2:inf"):
        with pytest.raises(ValueError):
            mesh.parse_bounds(bad)
    # the command line: options are checked and an existing output is refused before any GPU work
    dense = str(tmp_path)
    a = mesh.parse_args(["--dense_folder", dense])
    assert a.out == os.path.join(dense, "points_mvsnet", "mesh.ply") and a.voxel is None and a.resolution is None
    assert a.trunc_voxels == 4 and a.prob_threshold == 0.8 and a.num_consistent == 3 and a.min_count == 1 and not a.force
    for bad in (["--voxel", "0.1", "--resolution", "64"], ["--voxel", "0"], ["--resolution", "1"], ["--bounds", "1:2:3"],
                ["--min_count", "0"], ["--trunc_voxels", "0"], ["--num_consistent", "-1"], ["--fusion_sources", "some"]):
        with pytest.raises(SystemExit):
            mesh.parse_args(["--dense_folder", dense] + bad)
    out = str(tmp_path / "there.ply")
    open(out, "wb").close()
    with pytest.raises(SystemExit) as e:
        mesh.prepare_output(mesh.parse_args(["--dense_folder", dense, "--out", out]))
    assert "--force" in str(e.value)
    assert mesh.prepare_output(mesh.parse_args(["--dense_folder", dense, "--out", out, "--force"])) == out


def test_library_checks_arguments_before_any_gpu_call(lib_built):
    """Argument validation happens before the first HIP call, so the codes are testable without a GPU: the pointers below are
    host buffers that a kernel must never see."""
    from mvsnet_amd import _lib
    h = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    o = (ctypes.c_float * 3)(0, 0, 0)
    names = ("depth", "prob", "V", "H", "W", "proj", "images", "img_h", "img_w", "origin", "voxel", "nx", "ny", "nz", "trunc", "thr",
             "flags", "sum", "count", "rgb_sum", "rgb_count", "ws", "wsb", "stream")
    base = dict(depth=p, prob=p, V=1, H=4, W=4, proj=p, images=None, img_h=0, img_w=0, origin=o, voxel=0.1, nx=4, ny=4, nz=4,
                trunc=0.4, thr=0.8, flags=0, sum=p, count=p, rgb_sum=None, rgb_count=None, ws=p, wsb=4096, stream=None)
    integ = lambda **kw: h.mvs_tsdf_integrate_f32(*[dict(base, **kw)[k] for k in names])
    assert set(base) == set(names)
    for kw in (dict(depth=None), dict(prob=None), dict(proj=None), dict(sum=None), dict(count=None), dict(ws=None), dict(V=0),
               dict(H=0), dict(nx=0), dict(nz=-1), dict(voxel=0.0), dict(voxel=float("nan")), dict(trunc=0.0), dict(trunc=float("inf")),
               dict(thr=float("nan")), dict(flags=1), dict(images=p), dict(images=p, rgb_sum=p, rgb_count=p, img_h=0, img_w=4),
               dict(origin=(ctypes.c_float * 3)(0, float("nan"), 0))):
        assert integ(**kw) == -1, kw
    for kw in (dict(nx=2048, ny=2048, nz=512), dict(W=(1 << 24) + 1), dict(V=1024, H=2048, W=2048)):
        assert integ(**kw) == -2, kw
    assert integ(wsb=0) == -3
    assert h.mvs_tsdf_integrate_workspace_bytes(2, 4, 4) == 256 and h.mvs_tsdf_integrate_workspace_bytes(0, 4, 4) == 0
    assert h.mvs_tsdf_integrate_workspace_bytes(1024, 2048, 2048) == 0
    assert h.mvs_surface_nets_workspace_bytes(3, 3, 3) == 256 + 256 and h.mvs_surface_nets_workspace_bytes(1, 100, 1) == 256 + 512
    assert h.mvs_surface_nets_workspace_bytes(0, 3, 3) == 0 and h.mvs_surface_nets_workspace_bytes(2048, 2048, 512) == 0
    count = lambda sum=p, cnt=p, nx=3, ny=3, nz=3, mc=1, tot=p, ws=p, wsb=4096: h.mvs_surface_nets_count_f32(
        sum, cnt, nx, ny, nz, mc, tot, ws, wsb, None)
    for kw in (dict(sum=None), dict(cnt=None), dict(tot=None), dict(ws=None), dict(nx=0), dict(mc=0)):
        assert count(**kw) == -1, kw
    assert count(nx=2048, ny=2048, nz=512) == -2 and count(wsb=511) == -3
    write = lambda sum=p, cnt=p, rs=None, rc=None, org=o, voxel=0.1, nx=3, ny=3, nz=3, mc=1, rank=p, fe=p, M=1, F=1, v=p, c=p, f=p, \
        ws=p, wsb=4096: h.mvs_surface_nets_write_f32(sum, cnt, rs, rc, org, voxel, nx, ny, nz, mc, rank, fe, M, F, v, c, f, ws, wsb, None)
    for kw in (dict(sum=None), dict(cnt=None), dict(rs=p), dict(rc=p), dict(rank=None), dict(fe=None), dict(ws=None), dict(v=None),
               dict(c=None), dict(f=None), dict(M=-1), dict(F=-1), dict(mc=0), dict(voxel=0.0), dict(nz=0)):
        assert write(**kw) == -1, kw
    assert write(nx=2048, ny=2048, nz=512) == -2 and write(wsb=511) == -3
    assert buf.raw == b"\0" * 4096                                             # nothing was written


def test_every_package_module_still_imports():
    import mvsnet_amd
    names = sorted(m.name for m in pkgutil.iter_modules(mvsnet_amd.__path__) if not m.name.startswith("lib"))
    assert "mesh" in names
    for name in names:
        importlib.import_module("mvsnet_amd." + name)
    from mvsnet_amd import _lib, build
    assert "tsdf.hip" in build.SOURCES
    assert {"mvs_tsdf_integrate_f32", "mvs_surface_nets_count_f32", "mvs_surface_nets_write_f32",
            "mvs_surface_nets_workspace_bytes"} <= set(_lib.SIGNATURES)
