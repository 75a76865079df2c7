"""Host-side tests of the mesh simplification (no GPU): tests/mesh_simplify_reference.py on hand cases, against its float64 twin
and against numbers computed once with a prototype of the statement in mvsnet_amd/mesh_simplify.py; the option checks, the
parsers of the three command lines and the argument checks of the entry points through ctypes."""
import ctypes

import numpy as np
import pytest

from tests import mesh_clean_reference as MC
from tests import mesh_reference as M
from tests import mesh_simplify_reference as R

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
ZERO = np.zeros(3, np.float32)


def _f(rows):
    return np.asarray(rows, np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ hand cases

def test_two_triangles_inside_one_cell_leave_nothing():
    v = np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.2], [0.9, 0.9, 0.3], [0.1, 0.9, 0.4]], np.float32)
    ov, oc, of, rep = R.simplify(v, None, _f([[0, 1, 2], [0, 2, 3]]), 1.0, ZERO)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and oc is None
    assert (rep["clusters"], rep["degenerate_faces"], rep["faces_out"], rep["vertices_out"]) == (1, 2, 0, 0)


def _flat_grid(n):
    """n x n quads on (n+1)^2 vertices numbered row by row, two triangles each (mesh_clean_reference.grid's pattern)."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (j * (n + 1) + i).reshape(-1)
    return np.stack([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)], 1).reshape(-1, 3).astype(np.int32)


def test_two_by_two_vertices_per_cell_give_the_coarse_grid_at_the_exact_means():
    n = 5
    t = np.repeat(np.arange(n), 2) + np.tile([0.25, 0.75], n)                  # two vertices per cell and axis
    y, x = np.meshgrid(t, t, indexing="ij")
    v = np.stack([x.reshape(-1), y.reshape(-1), np.zeros(x.size)], 1).astype(np.float32)
    c = np.tile(np.array([[10, 20, 30]], np.uint8), (len(v), 1))
    ov, oc, of, rep = R.simplify(v, c, _flat_grid(2 * n - 1), 1.0, ZERO)
    cy, cx = np.meshgrid(np.arange(n) + 0.5, np.arange(n) + 0.5, indexing="ij")
    assert ov.tobytes() == np.stack([cx.reshape(-1), cy.reshape(-1), np.zeros(n * n)], 1).astype(np.float32).tobytes()
    assert of.tobytes() == _flat_grid(n - 1).tobytes() and (oc == [10, 20, 30]).all()
    assert rep["clusters"] == n * n and rep["duplicate_faces"] == 0 and rep["degenerate_faces"] == 2 * (2 * n - 1) ** 2 - 2 * (n - 1) ** 2
    assert M.mesh_topology(of)["V"] == n * n


def test_a_vertex_on_a_cell_boundary_goes_to_the_upper_cell():
    v = np.array([[1.0, 0.5, 2.0], [np.nextafter(np.float32(1), np.float32(0)), 0.5, 0.0], [0.75, -0.25, 0.5]], np.float32)
    ok, k, key, q, _ = R.cells(v, 0.5, np.array([0, -0.25, 0], np.float32))
    assert ok.all() and k.tolist() == [[2, 1, 4], [1, 1, 0], [1, 0, 1]]
    assert q[0].tolist() == [0, 2 ** 19, 0] and q[2].tolist() == [2 ** 19, 0, 0]
    assert key[0] == 2 | (1 << 21) | (4 << 42)


def test_a_fold_keeps_the_face_of_the_lower_index():
    cells = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]], np.float32)
    v = np.concatenate([cells, cells + np.float32(0.25)])
    ov, _, of, rep = R.simplify(v, None, _f([[1, 2, 0], [3, 5, 4], [2, 0, 1]]), 1.0, ZERO)
    assert of.tolist() == [[1, 2, 0]] and rep["duplicate_faces"] == 2 and rep["degenerate_faces"] == 0
    assert ov.tolist() == (cells + np.float32(0.125)).tolist()                 # both sides of the fold contribute to the means
    ov, _, of, rep = R.simplify(v, None, _f([[3, 5, 4], [1, 2, 0]]), 1.0, ZERO)
    assert of.tolist() == [[0, 2, 1]]                                          # its own winding


def test_a_face_that_repeats_an_index_is_valid_and_degenerate():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.5, 0.5]], np.float32)
    ov, _, of, rep = R.simplify(v, None, _f([[3, 3, 1], [0, 1, 2]]), 1.0, ZERO)
    assert (rep["invalid_faces"], rep["degenerate_faces"], rep["faces_out"]) == (0, 1, 1)
    assert abs(ov[0, 0] - 0.55) < 2.0 ** -20 and ov[0, 1:].tolist() == [0.5, 0.5]       # vertex 3 contributes: a valid face names it


def test_faces_that_name_no_vertex_and_vertices_that_are_not_finite():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    bad = [[-1, 0, 1], [0, 1, len(v)], [0, INT32_MAX, 1], [INT32_MIN, 0, 1], [0, 1, 3], [4, 1, 2], [0, 5, 2]]
    ov, _, of, rep = R.simplify(v, None, _f(bad + [[0, 1, 2]]), 1.0, ZERO)
    assert (rep["invalid_faces"], rep["unclusterable_vertices"], rep["faces_out"], rep["clusters"]) == (7, 3, 1, 3)
    assert of.tolist() == [[0, 1, 2]] and np.isfinite(ov).all()
    assert R.default_origin(v).tolist() == [0.5, 0.5, 0.5]                      # the minimum over the finite vertices only
    with pytest.raises(ValueError):
        R.default_origin(v[3:], 1)
    assert R.default_origin(v[3:], 0).tolist() == [0, 0, 0]


def test_cells_below_zero_and_beyond_the_last_are_out_of_range():
    last = float(2 ** 21)
    v = np.array([[-0.5, 0.5, 0.5], [last, 0.5, 0.5], [last - 0.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [0.5, -1e-9, 0.5]], np.float32)
    ok, k, _, _, _ = R.cells(v, 1.0, ZERO)
    assert ok.tolist() == [False, False, True, True, True, False] and k[2, 0] == 2 ** 21 - 1
    _, _, of, rep = R.simplify(v, None, _f([[0, 3, 4], [1, 3, 4], [2, 3, 4], [5, 3, 4]]), 1.0, ZERO)
    assert (rep["invalid_faces"], rep["unclusterable_vertices"], rep["faces_out"]) == (3, 3, 1) and of.tolist() == [[0, 1, 2]]


def test_an_unreferenced_vertex_does_not_move_a_mean():
    v = np.array([[0.25, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.75, 0.5, 0.5], [0.5, 0.5, 0.5]], np.float32)
    bad = [[4, 1, 99]]                                                          # an invalid face does not count as naming vertex 4
    ov, _, _, rep = R.simplify(v, None, _f([[0, 1, 2]] + bad), 1.0, ZERO)
    assert ov[0].tolist() == [0.25, 0.5, 0.5] and rep["clusters"] == 3
    ov, _, _, _ = R.simplify(v, None, _f([[0, 1, 2], [3, 3, 3]]), 1.0, ZERO)
    assert ov[0].tolist() == [0.5, 0.5, 0.5]


def test_empty_inputs():
    none_v, none_f = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for v, f, origin in ((none_v, none_f, None), (np.ones((4, 3), np.float32), none_f, None), (none_v, _f([[0, 1, 2]]), ZERO)):
        ov, oc, of, rep = R.simplify(v, np.zeros((len(v), 3), np.uint8), f, 1.0, origin)
        assert ov.shape == (0, 3) and ov.dtype == np.float32 and oc.shape == (0, 3) and of.shape == (0, 3) and of.dtype == np.int32
        assert rep["clusters"] == 0 and rep["invalid_faces"] == len(f)
    with pytest.raises(ValueError):
        R.simplify(none_v, None, _f([[0, 1, 2]]), 1.0)


def test_colour_rounding_on_a_tie_goes_up():
    v = np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]], np.float32)
    c = np.array([[0, 1, 254], [1, 2, 255], [7, 7, 7], [9, 9, 9]], np.uint8)
    _, oc, _, _ = R.simplify(v, c, _f([[0, 2, 3], [1, 2, 3]]), 1.0, ZERO)
    assert oc.tolist() == [[1, 2, 255], [7, 7, 7], [9, 9, 9]]                   # (2 C + n) // (2 n): 0.5 -> 1, 1.5 -> 2, 254.5 -> 255


# ------------------------------------------------------------------------------------------------ the float64 twin

def _assert_twin(v, f, cell, origin):
    got = R.all_clusters(v, None, f, cell, origin).astype(np.float64)
    mean, members, bound = R.twin(v, f, cell, origin)
    err = np.abs(got - mean)
    print("cell %g: %d clusters, worst error %.3g of a bound of %.3g" % (cell, len(mean), err.max(), bound[err.argmax() // 3].max()))
    assert (err <= bound).all()
    return members


@pytest.mark.parametrize("kind,noisy", MC.SCENES)
def test_positions_lie_within_the_derived_bound_of_the_float64_means(kind, noisy):
    v, _, f = MC.scene_mesh(kind, noisy)
    for mult in (1, 2, 3, 7.5):
        members = _assert_twin(v, f, R.voxels(mult, M.SCENE_VOXEL), np.asarray(M.SCENE_ORIGIN, np.float32))
    assert members.max() > 20


def test_twin_far_from_the_origin_and_with_tiny_cells():
    v, f = MC.grid(40)
    _assert_twin(v + np.float32(1000), f, 0.6, None)
    _assert_twin(v, f, 1e-5, None)
    _assert_twin(v * np.float32(1e4), f, 7e3, np.array([-5, -5, -2e4], np.float32))


# ------------------------------------------------------------------------------------------------ literals

def test_analytic_sphere():
    v, f = R.sphere_mesh()
    assert (len(v), len(f)) == (1212, 2420)
    rows = {2: (304, 604, 2.0476, 0.080), 3: (136, 268, 1.9502, 0.145)}
    for mult, (nv, nf, volume, radial) in rows.items():
        ov, _, of, rep = R.sphere_simplify(mult)
        top = M.mesh_topology(of)
        assert (len(ov), len(of)) == (nv, nf) and rep["clusters"] == nv
        assert top["manifold"] and top["oriented"] and top["V"] - top["E"] + top["F"] == 2
        assert round(M.signed_volume(ov, of), 4) == volume
        worst = np.abs(np.linalg.norm(ov.astype(np.float64), axis=1) - M.SPHERE_RADIUS).max() / M.SPHERE_VOXEL
        assert round(worst, 3) == radial
    assert round(M.signed_volume(v, f), 4) == 2.1067
    ov, _, of, rep = R.sphere_simplify(1)                                      # one vertex per cell: the mesh comes back
    assert (len(ov), len(of), rep["degenerate_faces"], rep["duplicate_faces"]) == (1212, 2420, 0, 0)
    cell, origin = R.voxels(1, M.SPHERE_VOXEL), np.asarray(M.SPHERE_ORIGIN, np.float32)
    members = _assert_twin(v, f, cell, origin)                                 # each vertex within the bound of its input
    assert (members == 1).all()
    top = M.mesh_topology(of)
    assert top["manifold"] and top["oriented"] and round(M.signed_volume(ov, of), 4) == 2.1067


def test_clean_plane():
    sc = M.scene("plane")
    ov, oc, of, rep = R.scene_simplify("plane", False, 2)
    assert (len(ov), len(of), rep["degenerate_faces"], rep["duplicate_faces"]) == (1008, 1886, 4830, 460)
    assert (rep["vertices_in"], rep["faces_in"]) == (3713, 7176) and oc.shape == (1008, 3)
    assert round((sc["surface_distance"](ov) / M.SCENE_VOXEL).max(), 3) == 0.026
    ov, _, of, rep = R.scene_simplify("plane", False, 3)
    assert (len(ov), len(of)) == (304, 540)
    assert round((sc["surface_distance"](ov) / M.SCENE_VOXEL).max(), 3) == 0.025


@pytest.mark.parametrize("kind,noisy,clusters,vertices,faces", [("plane", True, 1174, 1159, 2142), ("sphere", False, 1316, 1315, 2206),
                                                                ("sphere", True, 1336, 1330, 2216), ("step", False, None, 1152, 2116),
                                                                ("step", True, None, 1267, 2354)])
def test_other_scenes_at_two_voxels(kind, noisy, clusters, vertices, faces):
    ov, _, of, rep = R.scene_simplify(kind, noisy, 2)
    assert (len(ov), len(of)) == (vertices, faces) and (clusters is None or rep["clusters"] == clusters)
    assert len(np.unique(of)) == len(ov) and rep["faces_in"] == rep["faces_out"] + rep["degenerate_faces"] + rep["duplicate_faces"]


# ------------------------------------------------------------------------------------------------ options, parsers, entry points

def test_option_checks_come_before_any_gpu_work():
    from mvsnet_amd import mesh, mesh_simplify
    assert mesh_simplify.check_cell(0.1) == float(np.float32(0.1)) and mesh_simplify.check_cell(np.float32(2)) == 2.0
    assert mesh_simplify.check_origin([1, 2.5, -3]).tolist() == [1, 2.5, -3] and mesh_simplify.check_origin((0.1, 0, 0)).dtype == np.float32
    assert mesh_simplify.check_voxels(None) is None and mesh_simplify.check_voxels(0) is None and mesh_simplify.check_voxels(2.5) == 2.5
    v, f = np.ones((4, 3), np.float32), np.zeros((1, 3), np.int32)
    for bad in (0, -1.0, np.nan, np.inf, 1e-60, 1e60, "x", None, True):
        with pytest.raises(ValueError):
            mesh_simplify.check_cell(bad)
        with pytest.raises(ValueError):
            mesh_simplify.simplify_mesh(v, None, f, bad)                        # a ValueError with or without a GPU
    for bad in ((1, 2), (1, 2, np.nan), (1, 2, 1e60), "abc", 3.0):
        with pytest.raises(ValueError):
            mesh_simplify.simplify_mesh(v, None, f, 1.0, bad)
    for bad in (-1, np.nan, np.inf, "x", True):
        with pytest.raises(ValueError):
            mesh_simplify.check_voxels(bad)
    z = np.zeros((2, 4, 4), np.float32)
    for bad in (-2, np.nan):
        with pytest.raises(ValueError):
            mesh.mesh_depth_maps(z, z, np.zeros((2, 2, 4, 4)), simplify_voxels=bad)
    for args in ((v[:, :2], None, f), (v, None, f[:, :2]), (v, np.zeros((3, 3), np.uint8), f), (v, None, 7)):
        with pytest.raises(ValueError):
            mesh_simplify.simplify_mesh(*args, 1.0)
    wide = np.array([[0, 0, 0], [3e6, 1, 1]], np.float32)
    with pytest.raises(ValueError, match="2\\^21"):
        mesh_simplify.simplify_mesh(wide, None, f, 1.0)                        # the default origin: more than 2^21 cells on an axis
    with pytest.raises(ValueError, match="finite"):
        mesh_simplify.simplify_mesh(np.full((2, 3), np.nan, np.float32), None, f, 1.0)
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(v, None, f, 1.0, device="cpu")
    assert mesh_simplify.parse_origin("1:-2.5:3e1").tolist() == [1, -2.5, 30]


def test_the_three_command_lines_check_their_options(tmp_path):
    from mvsnet_amd import depthfusion, mesh, mesh_simplify
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    a = mesh_simplify.parse_args(["--mesh", src, "--out", out, "--cell", "0.1"])
    assert (a.cell, a.origin, a.force) == (float(np.float32(0.1)), None, False)
    a = mesh_simplify.parse_args(["--mesh", src, "--out", out, "--cell", "2", "--origin=-1.5:0:2", "--force"])
    assert a.cell == 2.0 and a.origin.tolist() == [-1.5, 0, 2] and a.force
    for extra in (["--cell", "0"], ["--cell", "-1"], ["--cell", "nan"], ["--cell", "inf"], ["--cell", "1", "--origin", "1:2"],
                  ["--cell", "1", "--origin", "1:2:x"], ["--cell", "1", "--origin", "1:2:inf"], []):
        with pytest.raises(SystemExit):
            mesh_simplify.parse_args(["--mesh", src, "--out", out] + extra)
    open(out, "wb").close()                                                    # an existing output is refused before any GPU work
    with pytest.raises(SystemExit) as e:
        mesh_simplify.main(["--mesh", src, "--out", out, "--cell", "1"])
    assert "--force" in str(e.value)
    assert mesh.parse_args(["--dense_folder", str(tmp_path)]).simplify_voxels is None
    assert mesh.parse_args(["--dense_folder", str(tmp_path), "--simplify_voxels", "2.5"]).simplify_voxels == 2.5
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            mesh.parse_args(["--dense_folder", str(tmp_path), "--simplify_voxels", bad])
        assert "--simplify_voxels" in str(e.value)
    with pytest.raises(SystemExit) as e:
        depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--fusion", "hip", "--mesh_simplify_voxels", "2"])
    assert "needs --mesh" in str(e.value)
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit) as e:
            depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--fusion", "hip", "--mesh", "--mesh_simplify_voxels", bad])
        assert "--mesh_simplify_voxels must be positive" in str(e.value)
    with pytest.raises(SystemExit) as e:
        depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--mesh", "--mesh_simplify_voxels", "2"])
    assert "--mesh needs --fusion hip" in str(e.value)
    assert not (tmp_path / "none").exists()


def test_library_checks_arguments_before_any_gpu_call(lib_built):
    """Argument validation happens before the first HIP call, so the codes are testable without a GPU: the pointers below are
    host buffers that a kernel must never see."""
    from mvsnet_amd import _lib, build
    h = _lib.load()
    assert "mesh_simplify.hip" in build.SOURCES and h.mvs_abi_version() == 1
    buf = ctypes.create_string_buffer(8192)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big, nan, inf = 2 ** 31, float("nan"), float("inf")
    wsb = h.mvs_mesh_cluster_workspace_bytes
    assert wsb(0, 0) == 3 * 256 and wsb(1, 5) == 768 and wsb(4, 0) == 768 and wsb(65, 1) == 256 + 512 + 17 * 256
    assert wsb(-1, 0) == 0 and wsb(0, -1) == 0 and wsb(big, 1) == 0 and wsb(1, big) == 0 and wsb(big - 1, big - 1) == 256 + 2 ** 33 + 2 ** 37
    keys = lambda v=p, M=8, f=p, F=4, ox=0.0, oy=0.0, oz=0.0, cell=1.0, k=p, q=p, ws=p, n=8192: h.mvs_mesh_cluster_keys_f32(
        v, M, f, F, ox, oy, oz, cell, k, q, ws, n, None)
    for kw in (dict(v=None), dict(f=None), dict(k=None), dict(q=None), dict(ws=None), dict(M=-1), dict(F=-1), dict(cell=0.0), dict(cell=-1.0),
               dict(cell=nan), dict(cell=inf), dict(ox=nan), dict(oy=inf), dict(oz=-inf)):
        assert keys(**kw) == -1, kw
    assert keys(M=big) == -2 and keys(F=big) == -2 and keys(n=1023) == -3 and keys(M=1000, n=8191) == -3
    heads = lambda sk=p, M=8, head=p: h.mvs_mesh_cluster_heads_i64(sk, M, head, None)
    assert heads(sk=None) == -1 and heads(head=None) == -1 and heads(M=-1) == -1 and heads(M=big) == -2 and heads(sk=None, M=0, head=None) == 0
    sums = lambda sk=p, order=p, rank=p, q=p, c=p, M=8, ox=0.0, oy=0.0, oz=0.0, cell=1.0, vc=p, cv=p, cc=p, ws=p, n=8192: \
        h.mvs_mesh_cluster_sums_f32(sk, order, rank, q, c, M, ox, oy, oz, cell, vc, cv, cc, ws, n, None)
    for kw in (dict(sk=None), dict(order=None), dict(rank=None), dict(q=None), dict(vc=None), dict(cv=None), dict(c=None), dict(cc=None),
               dict(ws=None), dict(M=-1), dict(cell=0.0), dict(cell=nan), dict(oz=nan)):
        assert sums(**kw) == -1, kw
    assert sums(M=big) == -2 and sums(n=1023) == -3 and sums(M=0, n=768) == 0
    faces = lambda f=p, M=8, F=4, vc=p, cf=p, lo=p, hi=p, ws=p, n=8192: h.mvs_mesh_cluster_faces_i32(f, M, F, vc, cf, lo, hi, ws, n, None)
    for kw in (dict(f=None), dict(vc=None), dict(cf=None), dict(lo=None), dict(ws=None), dict(M=-1), dict(F=-1)):
        assert faces(**kw) == -1, kw
    assert faces(M=big) == -2 and faces(F=big) == -2 and faces(n=1023) == -3
    assert faces(M=2 ** 21 + 1, hi=None, n=2 ** 40) == -2 and faces(M=2 ** 21 + 1, n=1024) == -3      # one key only up to 2^21 vertices
    mark = lambda cf=p, M=8, F=4, lo=p, hi=p, order=p, fk=p, vk=p, ws=p, n=8192: h.mvs_mesh_cluster_mark_i32(
        cf, M, F, lo, hi, order, fk, vk, ws, n, None)
    for kw in (dict(cf=None), dict(lo=None), dict(order=None), dict(fk=None), dict(vk=None), dict(ws=None), dict(M=-1), dict(F=-1)):
        assert mark(**kw) == -1, kw
    assert mark(M=big) == -2 and mark(F=big) == -2 and mark(n=1023) == -3
