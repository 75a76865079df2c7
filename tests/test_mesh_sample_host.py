"""mvsnet_amd/mesh_sample.py without a GPU: tests/mesh_sample_reference.py (the numpy restatement the kernels are held to, byte
for byte, in test_gpu_mesh_sample.py) on hand-made cases, its properties, the uniformity of the samples, literal numbers on
the analytic sphere, the six scene meshes, read_ply_mesh, the parsers of the four command lines and the argument checks of
the entry points through ctypes."""
import ctypes

import numpy as np
import pytest

from tests import mesh_clean_reference as MC
from tests import mesh_reference as M
from tests import mesh_sample_reference as R
from tests import mesh_simplify_reference as MS

TRIANGLE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
FACE = np.array([[0, 1, 2]], np.int32)


# ------------------------------------------------------------------------------------------------ hand cases

def test_one_triangle_of_half_a_unit_at_density_ten_gives_five_samples():
    s = R.sample(TRIANGLE, None, FACE, 10)
    assert s["stats"] == {"faces": 1, "invalid": 0, "zero_area": 0, "samples": 5, "area": 0.5}
    assert s["xyz"].shape == (5, 3) and s["face_index"].tolist() == [0] * 5 and (s["normals"] == [0, 0, 1]).all()
    assert (s["xyz"][:, 2] == 0).all() and (s["xyz"][:, :2] > 0).all() and (s["xyz"][:, :2].sum(1) < 1).all()


def test_error_diffusion_gives_small_faces_their_share_in_face_order():
    assert R.sample(TRIANGLE, None, np.repeat(FACE, 6, 0), 1)["counts"].tolist() == [0, 1, 0, 1, 0, 1]
    s = R.sample(TRIANGLE, None, np.repeat(FACE, 10, 0), 0.6)
    assert s["counts"].tolist() == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0] and s["stats"]["samples"] == 2
    assert s["face_index"].tolist() == [3, 6]


def test_faces_without_samples_are_counted_in_their_status_word():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, np.inf, 0], [1, 1, 1], [2, 2, 2], [0, 0, -np.inf]], np.float32)
    m = len(v)
    f = np.array([[0, 1, 2], [-1, 1, 2], [0, m, 2], [0, 1, 2 ** 31 - 1], [-2 ** 31, 1, 2], [3, 1, 2], [0, 4, 2], [0, 1, 7],   # 1..7 invalid
                  [0, 0, 1], [1, 1, 1], [0, 5, 6], [2, 1, 0]], np.int32)                                                   # 8..10 no area
    q, invalid, zero, saturated = R.quota(v, f, 100.0)
    assert invalid.tolist() == [False] + [True] * 7 + [False] * 4
    assert zero.tolist() == [False] * 8 + [True] * 3 + [False] and not saturated.any()
    assert (q > 0).tolist() == [True] + [False] * 10 + [True] and q[0] == q[11] == 50 * 65536
    s = R.sample(v, None, f, 100.0)
    assert s["stats"] == {"faces": 12, "invalid": 7, "zero_area": 3, "samples": 100, "area": 1.0}
    assert s["counts"].tolist() == [50] + [0] * 10 + [50]
    assert (s["normals"][:50] == [0, 0, 1]).all() and (s["normals"][50:] == [0, 0, -1]).all()   # the winding gives the side


def test_empty_inputs():
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for v, f in ((none_v, none_f), (TRIANGLE, none_f), (none_v, FACE)):
        s = R.sample(v, None, f, 4.0)
        assert s["xyz"].shape == (0, 3) and s["stats"]["samples"] == 0 and s["stats"]["invalid"] == len(f) and s["stats"]["area"] == 0


def test_a_saturated_face_and_too_many_samples_raise():
    big = TRIANGLE * np.float32(2048)                                          # area 2^21: t = 2^37 at density 1
    with pytest.raises(ValueError, match="saturated"):
        R.sample(big, None, FACE, 1.0)
    assert R.quota(big, FACE, 1.0)[3].tolist() == [True] and R.quota(big, FACE, 0.49)[3].tolist() == [False]
    assert R.quota(TRIANGLE, FACE, 1e300)[3].tolist() == [True]                # t = +inf
    with pytest.raises(ValueError, match="max_samples"):
        R.sample(TRIANGLE, None, FACE, 10, max_samples=4)
    assert R.sample(TRIANGLE, None, FACE, 10, max_samples=5)["stats"]["samples"] == 5


# ------------------------------------------------------------------------------------------------ properties

def _assert_inside(v, f, s):
    """Every sample within the docstring's bound of its triangle's plane, and no further than that outside an edge."""
    tri = np.asarray(v, np.float32)[np.asarray(f)[s["face_index"]]].astype(np.float64)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    p = s["xyz"].astype(np.float64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1)[:, None]
    bound = R.plane_bound(v, f, s["face_index"])
    off = np.abs(((p - a) * n).sum(1))
    worst = [float((off / bound).max())]
    assert (off <= bound).all()
    for x, y in ((a, b), (b, c), (c, a)):                                      # inward normal of the edge x -> y, in the plane
        inward = np.cross(n, y - x)
        inward /= np.linalg.norm(inward, axis=1)[:, None]
        d = ((p - x) * inward).sum(1)
        worst.append(float((-d / bound).max()))
        assert (d >= -bound).all()
    print("worst plane offset and worst distance beyond an edge, in bounds: %s" % [round(w, 3) for w in worst])


@pytest.mark.parametrize("kind,noisy", MC.SCENES)
@pytest.mark.parametrize("voxels", [2.0, 0.5])
def test_scene_meshes(kind, noisy, voxels):
    v, c, f = MC.scene_mesh(kind, noisy)
    s = R.scene_sample(kind, noisy, voxels * M.SCENE_VOXEL)
    q = R.quota(v, f, R.density_of(voxels * M.SCENE_VOXEL))[0]
    N = s["stats"]["samples"]
    assert N == int(q.sum()) >> 16 == len(s["xyz"]) == int(s["counts"].sum()) and N > 500
    assert ((s["counts"] == q >> 16) | (s["counts"] == (q >> 16) + 1)).all()     # the floor or the ceiling of q / 65536
    w0, wu, wv = s["weights"]
    assert (w0 >= 0).all() and (wu > 0).all() and (wv > 0).all() and (w0 + wu + wv == 2 ** 25).all()
    assert (np.diff(s["face_index"]) >= 0).all()
    _assert_inside(v, f, s)
    tri = c[f[s["face_index"]]].astype(np.int64)                               # a colour lies between its three corners'
    assert (s["colours"] >= tri.min(1)).all() and (s["colours"] <= tri.max(1)).all()
    length = np.linalg.norm(s["normals"].astype(np.float64), axis=1)
    assert np.abs(length - 1).max() < 2.0 ** -22
    true_area = 0.5 * np.linalg.norm(np.cross((v[f[:, 1]] - v[f[:, 0]]).astype(np.float64), (v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)), axis=1).sum()
    assert abs(s["stats"]["area"] - true_area) <= len(f) / 65536.0 / R.density_of(voxels * M.SCENE_VOXEL) + 1e-9 * true_area


def test_the_seed_moves_the_samples_and_not_the_counts():
    v, c, f = MC.scene_mesh("step", True)
    d = R.density_of(0.05)
    one, again, other = R.sample(v, c, f, d, 7), R.sample(v, c, f, d, 7), R.sample(v, c, f, d, 2 ** 64 - 1)
    assert one["xyz"].tobytes() == again["xyz"].tobytes() and one["colours"].tobytes() == again["colours"].tobytes()
    assert np.array_equal(one["counts"], other["counts"]) and np.array_equal(one["face_index"], other["face_index"])
    assert (one["xyz"] != other["xyz"]).any(1).mean() > 0.99
    assert one["normals"].tobytes() == other["normals"].tobytes()


def test_reversing_the_faces_moves_the_carried_samples_and_keeps_the_total():
    v, _, f = MC.scene_mesh("sphere", False)
    d = R.density_of(0.1)
    one, back = R.sample(v, None, f, d), R.sample(v, None, f[::-1], d)
    assert abs(one["stats"]["samples"] - back["stats"]["samples"]) <= 1
    assert not np.array_equal(one["counts"], back["counts"][::-1])
    assert np.abs(one["counts"] - back["counts"][::-1]).max() <= 1


# ------------------------------------------------------------------------------------------------ uniformity

@pytest.mark.parametrize("seed,chi2", [(0, 241), (1, 260), (12345, 244)])
def test_samples_are_uniform_over_the_unit_square(seed, chi2):
    """16 x 16 bins of 256 expected samples: chi-square with 255 degrees of freedom, mean 255 and standard deviation sqrt(510);
    the limit is five of them above the mean."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    s = R.sample(v, None, np.array([[0, 1, 2], [0, 2, 3]], np.int32), 65536, seed)
    assert s["counts"].tolist() == [32768, 32768]
    h = np.histogram2d(s["xyz"][:, 0], s["xyz"][:, 1], bins=16, range=[[0, 1], [0, 1]])[0]
    got = float(((h - 256) ** 2 / 256).sum())
    print("seed %d: chi-square %.1f" % (seed, got))
    assert got < 255 + 5 * np.sqrt(510) and round(got) == chi2


# ------------------------------------------------------------------------------------------------ literals

@pytest.mark.parametrize("spacing,N", [(0.1, 796), (0.05, 3186), (0.02, 19913)])
def test_analytic_sphere(spacing, N):
    s = R.sphere_sample(spacing)
    v, f = MS.sphere_mesh()
    assert s["stats"]["samples"] == N and s["stats"]["faces"] == 2420 and s["stats"]["invalid"] == s["stats"]["zero_area"] == 0
    assert round(s["stats"]["area"], 4) == {0.1: 7.9652, 0.05: 7.9653, 0.02: 7.9653}[spacing]
    assert round(4 * np.pi * M.SPHERE_RADIUS ** 2, 4) == 8.0425
    r = np.linalg.norm(s["xyz"].astype(np.float64), axis=1)
    assert 0.792 <= r.min() and r.max() <= 0.800
    outward = (s["normals"].astype(np.float64) * s["xyz"]).sum(1) / r
    assert outward.min() > 0                                                  # mesh.py winds its faces to look outwards
    _assert_inside(v, f, s)


def sphere_points(n=200000, seed=0):
    g = np.random.RandomState(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1)[:, None] * M.SPHERE_RADIUS).astype(np.float32)


def test_samples_score_a_simplified_sphere_that_its_vertices_do_not():
    """The issue's table: 200 000 points on the true sphere against sphere_simplify(2) at tau = 0.05."""
    from scipy.spatial import cKDTree
    gt = sphere_points()
    ov, _, of, _ = MS.sphere_simplify(2)
    s = R.sample(ov, None, of, R.density_of(0.02))
    from_vertices = float((cKDTree(ov).query(gt)[0] < 0.05).mean())
    from_samples = float((cKDTree(s["xyz"]).query(gt)[0] < 0.05).mean())
    print("completeness at 0.05: %.3f from %d vertices, %.3f from %d samples" % (from_vertices, len(ov), from_samples, len(s["xyz"])))
    assert from_samples == 1.0 and from_vertices < 0.35


# ------------------------------------------------------------------------------------------------ read_ply_mesh

def _ply(path, fmt, v, c, f, index="int", count="uchar", name="vertex_indices", extra=False, vtype="float"):
    fd = {"float": "<f4", "double": "<f8"}[vtype]
    idt = {"int": "<i4", "uint": "<u4", "short": "<i2"}[index]
    head = ["ply", "format %s 1.0" % fmt, "comment made by the test"]
    if extra:
        head += ["element camera 2", "property float focal", "property list uchar float distortion"]
    head += ["element vertex %d" % len(v)] + ["property %s %s" % (vtype, a) for a in "xyz"]
    if c is not None:
        head += ["property uchar %s" % a for a in ("red", "green", "blue")]
    head += ["property float quality", "element face %d" % len(f), "property uchar flags", "property list %s %s %s" % (count, index, name),
             "end_header"]
    out = ("\n".join(head) + "\n").encode("ascii")
    if fmt == "ascii":
        rows = ["1.5 2 0.25 0.5", "2.5 0"] if extra else []
        for k in range(len(v)):
            rows.append(" ".join([repr(float(x)) for x in v[k]] + ([str(int(x)) for x in c[k]] if c is not None else []) + ["0.5"]))
        rows += ["7 %d %s" % (len(r), " ".join(str(int(x)) for x in r)) for r in f]
        out += ("\n".join(rows) + "\n").encode("ascii")
    else:
        if extra:
            out += np.array([1.5], "<f4").tobytes() + bytes([2]) + np.array([0.25, 0.5], "<f4").tobytes()
            out += np.array([2.5], "<f4").tobytes() + bytes([0])
        for k in range(len(v)):
            out += np.asarray(v[k], fd).tobytes() + (bytes(int(x) for x in c[k]) if c is not None else b"") + np.array([0.5], "<f4").tobytes()
        for r in f:
            out += bytes([7]) + np.array([len(r)], {"uchar": "u1", "int": "<i4"}[count]).tobytes() + np.asarray(r, idt).tobytes()
    with open(path, "wb") as fh:
        fh.write(out)
    return str(path)


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_read_ply_mesh(tmp_path, fmt):
    from mvsnet_amd import mesh, mesh_sample
    rs = np.random.RandomState(4)
    v = rs.standard_normal((7, 3)).astype(np.float32)
    c = rs.randint(0, 256, (7, 3)).astype(np.uint8)
    f = rs.randint(0, 7, (9, 3)).astype(np.int32)
    for k, kw in enumerate((dict(), dict(c=None), dict(index="uint"), dict(index="short", count="int", name="vertex_index"),
                            dict(extra=True), dict(vtype="double"))):
        colours = kw.pop("c", c)
        gv, gc, gf = mesh_sample.read_ply_mesh(_ply(tmp_path / ("m%d.ply" % k), fmt, v, colours, f, **kw))
        assert gv.dtype == np.float32 and gf.dtype == np.int32 and gv.tobytes() == v.tobytes() and gf.tobytes() == f.tobytes(), kw
        assert (gc is None) if colours is None else (gc.dtype == np.uint8 and gc.tobytes() == c.tobytes())
    quad = [list(r) for r in f[:4]] + [[0, 1, 2, 3]] + [list(r) for r in f[4:]]
    with pytest.raises(ValueError, match="not a triangle"):
        mesh_sample.read_ply_mesh(_ply(tmp_path / "quad.ply", fmt, v, c, quad))
    with pytest.raises(ValueError, match="no faces"):
        mesh_sample.read_ply_mesh(_ply(tmp_path / "cloud.ply", fmt, v, c, []))
    with pytest.raises(ValueError, match="vertex_indices"):
        mesh_sample.read_ply_mesh(_ply(tmp_path / "name.ply", fmt, v, c, f, name="corners"))
    whole = open(_ply(tmp_path / "cut.ply", fmt, v, c, f), "rb").read()
    with open(tmp_path / "cut.ply", "wb") as fh:
        fh.write(whole[:-5])
    with pytest.raises(ValueError, match="file ends"):
        mesh_sample.read_ply_mesh(str(tmp_path / "cut.ply"))
    from mvsnet_amd import evaluate
    pts, rgb = evaluate.read_ply_points(str(tmp_path / "m0.ply"))               # the point reader still takes the vertices alone
    assert pts.tobytes() == v.tobytes() and rgb.tobytes() == c.tobytes()
    if fmt != "ascii":
        mesh.write_mesh_ply(str(tmp_path / "own.ply"), v, c, f)                # the project's own mesh files are read as well
        gv, gc, gf = mesh_sample.read_ply_mesh(str(tmp_path / "own.ply"))
        assert gv.tobytes() == v.tobytes() and gc.tobytes() == c.tobytes() and gf.tobytes() == f.tobytes()
        big = open(str(tmp_path / "own.ply"), "rb").read().replace(b"binary_little_endian", b"binary_big_endian")
        with open(tmp_path / "big.ply", "wb") as fh:
            fh.write(big)
        with pytest.raises(ValueError, match="big-endian"):
            mesh_sample.read_ply_mesh(str(tmp_path / "big.ply"))


# ------------------------------------------------------------------------------------------------ options, parsers, entry points

def test_option_checks_come_before_any_gpu_work():
    from mvsnet_amd import evaluate, mesh, mesh_sample
    assert mesh_sample.check_spacing(0.02) == 1.0 / (0.02 * 0.02) == R.density_of(0.02) and mesh_sample.check_spacing(2) == 0.25
    assert mesh_sample.check_density(3) == 3.0 and mesh_sample.check_seed(2 ** 64 - 1) == 2 ** 64 - 1
    assert mesh_sample.check_max_samples(2 ** 40) == 2 ** 31 - 1 and mesh_sample.check_max_samples(0) == 0
    for bad in (0, -1.0, np.nan, np.inf, 1e-200, 1e200, "x", None, True):
        with pytest.raises(ValueError):
            mesh_sample.check_spacing(bad)
    for bad in (0, -1.0, np.nan, np.inf, "x", None, True):
        with pytest.raises(ValueError):
            mesh_sample.check_density(bad)
        with pytest.raises(ValueError):
            mesh_sample.sample_mesh(TRIANGLE, None, FACE, bad)                 # a ValueError with or without a GPU
    for bad in (-1, 2 ** 64, 0.5, "x", None, True):
        with pytest.raises(ValueError):
            mesh_sample.sample_mesh(TRIANGLE, None, FACE, 1.0, bad)
    for bad in (-1, 0.5, None, True):
        with pytest.raises(ValueError):
            mesh_sample.sample_mesh(TRIANGLE, None, FACE, 1.0, max_samples=bad)
    for args in ((TRIANGLE[:, :2], None, FACE), (TRIANGLE, None, FACE[:, :2]), (TRIANGLE, np.zeros((2, 3), np.uint8), FACE), (TRIANGLE, None, 7)):
        with pytest.raises(ValueError):
            mesh_sample.sample_mesh(*args, 1.0)
    with pytest.raises(ValueError):
        mesh_sample.sample_mesh(TRIANGLE, None, FACE, 1.0, device="cpu")
    with pytest.raises(ValueError, match="2\\^26"):
        mesh_sample.sample_mesh(TRIANGLE, None, np.broadcast_to(FACE, (2 ** 26 + 1, 3)), 1.0)
    pts = np.zeros((4, 3), np.float32)
    for kw in (dict(pred_faces=FACE), dict(pred_spacing=0.1), dict(gt_faces=FACE), dict(gt_spacing=0.1),
               dict(pred_faces=FACE, pred_spacing=0), dict(gt_faces=FACE, gt_spacing=np.nan), dict(pred_faces=FACE[:, :2], pred_spacing=1.0)):
        with pytest.raises(ValueError):
            evaluate.evaluate_point_clouds(TRIANGLE, pts, max_dist=1.0, **kw)
    with pytest.raises(ValueError, match="go together"):
        mesh.mesh_dense_folder("nowhere", "nowhere/mesh.ply", eval_gt="gt.ply")
    with pytest.raises(ValueError):
        mesh.mesh_dense_folder("nowhere", "nowhere/mesh.ply", eval_gt="gt.ply", eval_spacing=-1)
    with pytest.raises(ValueError):
        mesh.mesh_dense_folder("nowhere", "nowhere/mesh.ply", eval_gt="gt.ply", eval_spacing=0.1, eval_thresholds=[30.0])


def test_the_four_command_lines_check_their_options(tmp_path, capsys):
    from mvsnet_amd import depthfusion, evaluate, mesh, mesh_sample
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    a = mesh_sample.parse_args(["--mesh", src, "--out", out, "--spacing", "0.02"])
    assert (a.density, a.seed, a.normals, a.force, a.max_samples) == (1.0 / (0.02 * 0.02), 0, False, False, 2 ** 27)
    a = mesh_sample.parse_args(["--mesh", src, "--out", out, "--spacing", "2", "--seed", "18446744073709551615", "--normals", "--force"])
    assert a.density == 0.25 and a.seed == 2 ** 64 - 1 and a.normals and a.force
    for extra in (["--spacing", "0"], ["--spacing", "-1"], ["--spacing", "nan"], ["--spacing", "inf"], ["--spacing", "1", "--seed", "-1"],
                  ["--spacing", "1", "--seed", "18446744073709551616"], ["--spacing", "1", "--max_samples", "-1"], []):
        with pytest.raises(SystemExit):
            mesh_sample.parse_args(["--mesh", src, "--out", out] + extra)
    open(out, "wb").close()                                                    # an existing output is refused before any GPU work
    with pytest.raises(SystemExit) as e:
        mesh_sample.main(["--mesh", src, "--out", out, "--spacing", "1"])
    assert "--force" in str(e.value)
    a = mesh.parse_args(["--dense_folder", str(tmp_path)])
    assert a.eval_gt is None and a.eval_spacing is None
    a = mesh.parse_args(["--dense_folder", str(tmp_path), "--eval_gt", src, "--eval_spacing", "0.5", "--eval_max_dist", "3", "--eval_thresholds", "1,2"])
    assert (a.eval_gt, a.eval_spacing, a.eval_max_dist, a.eval_thresholds) == (src, 0.5, 3.0, [1.0, 2.0])
    for extra in (["--eval_gt", src], ["--eval_spacing", "1"], ["--eval_gt", src, "--eval_spacing", "0"], ["--eval_gt", src, "--eval_spacing", "nan"],
                  ["--eval_gt", src, "--eval_spacing", "1", "--eval_thresholds", "30"], ["--eval_gt", src, "--eval_spacing", "1", "--eval_thresholds", "x"]):
        with pytest.raises(SystemExit) as e:
            mesh.parse_args(["--dense_folder", str(tmp_path)] + extra)
        assert "--eval_" in str(e.value)
    none = str(tmp_path / "none")
    for extra, text in ((["--mesh_eval_spacing", "1"], "needs --mesh and --eval_gt"), (["--mesh", "--mesh_eval_spacing", "1"], "needs --mesh and --eval_gt"),
                        (["--eval_gt", src, "--mesh_eval_spacing", "1"], "needs --mesh and --eval_gt"),
                        (["--mesh", "--eval_gt", src, "--mesh_eval_spacing", "0"], "--mesh_eval_spacing"),
                        (["--mesh", "--eval_gt", src, "--mesh_eval_spacing", "inf"], "--mesh_eval_spacing")):
        with pytest.raises(SystemExit) as e:
            depthfusion.main(["--dense_folder", none, "--fusion", "hip"] + extra)
        assert text in str(e.value)
    for extra in (["--pred_spacing", "0"], ["--gt_spacing", "-2"], ["--gt_spacing", "nan"]):
        with pytest.raises(SystemExit) as e:
            evaluate.main(["--pred", src, "--gt", src, "--max_dist", "1"] + extra)
        assert "spacing" in str(e.value)
    assert not (tmp_path / "none").exists()


def test_library_checks_arguments_before_any_gpu_call(lib_built):
    """Argument validation happens before the first HIP call, so the codes are testable without a GPU: the pointers below are
    host buffers that a kernel must never see."""
    from mvsnet_amd import _lib, build
    h = _lib.load()
    assert "mesh_sample.hip" in build.SOURCES and h.mvs_abi_version() == 1
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big, nan, inf = 2 ** 31, float("nan"), float("inf")
    wsb = h.mvs_mesh_sample_workspace_bytes
    assert wsb(0, 0) == 256 and wsb(big - 1, 2 ** 26) == 256
    assert wsb(-1, 0) == 0 and wsb(0, -1) == 0 and wsb(big, 1) == 0 and wsb(1, 2 ** 26 + 1) == 0
    quota = lambda v=p, M=8, f=p, F=4, d=1.0, q=p, ws=p, n=256: h.mvs_mesh_sample_quota_f32(v, M, f, F, d, q, ws, n, None)
    for kw in (dict(v=None), dict(f=None), dict(q=None), dict(ws=None), dict(M=-1), dict(F=-1), dict(d=0.0), dict(d=-1.0), dict(d=nan), dict(d=inf)):
        assert quota(**kw) == -1, kw
    assert quota(M=big) == -2 and quota(F=2 ** 26 + 1) == -2 and quota(n=255) == -3
    write = lambda v=p, c=p, M=8, f=p, F=4, s=p, N=4, seed=0, xyz=p, face=p, rgb=p, nrm=p: h.mvs_mesh_sample_write_f32(
        v, c, M, f, F, s, N, seed, xyz, face, rgb, nrm, None)
    for kw in (dict(v=None), dict(f=None), dict(s=None), dict(xyz=None), dict(c=None), dict(M=-1), dict(F=-1), dict(N=-1), dict(M=0), dict(F=0)):
        assert write(**kw) == -1, kw
    assert write(M=big) == -2 and write(F=2 ** 26 + 1) == -2 and write(N=big) == -2
    assert write(N=0) == 0 and write(v=None, c=None, M=0, f=None, F=0, s=None, N=0, xyz=None, face=None, rgb=None, nrm=None) == 0
