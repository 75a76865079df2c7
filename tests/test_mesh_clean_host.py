"""Host tests of the mesh-cleaning semantics (tests/mesh_clean_reference.py, the numpy restatement that the GPU must equal) and
of the host side of mvsnet_amd.mesh_clean: the reference against scipy's connected components, hand cases, the literal
numbers of the six scene meshes, option checks, the three command lines' parsers and the library's argument checks.  No GPU is
needed."""
import ctypes

import numpy as np
import pytest

from tests import mesh_clean_reference as R
from tests import mesh_reference as M

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


def _scipy_labels(vertices, faces):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    g = np.asarray(faces, np.int64)[R.valid_faces(vertices, faces)]
    a, b = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    n = len(vertices)
    return connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n)), directed=False)[1]


def _assert_same_partition_with_minima_as_labels(vertices, faces):
    ours, theirs = R.vertex_labels(vertices, faces), _scipy_labels(vertices, faces)
    # the same partition: the pairs (ours, theirs) are a bijection between the two label sets
    pairs = np.unique(np.stack([ours, theirs], 1), axis=0)
    assert len(pairs) == len(np.unique(ours)) == len(np.unique(theirs))
    # the labels are the component minima
    minima = np.full(len(vertices), len(vertices), np.int64)
    np.minimum.at(minima, theirs, np.arange(len(vertices)))
    assert np.array_equal(ours, minima[theirs])


@pytest.mark.parametrize("kind,noisy", R.SCENES)
def test_reference_and_scipy_agree_on_the_scene_meshes(kind, noisy):
    v, _, f = R.scene_mesh(kind, noisy)
    _assert_same_partition_with_minima_as_labels(v, f)


@pytest.mark.parametrize("seed", range(6))
def test_reference_and_scipy_agree_on_random_face_lists(seed):
    rs = np.random.RandomState(seed)
    m = int(rs.randint(1, 400))
    v = rs.randn(m, 3).astype(np.float32)
    f = rs.randint(-2, m + 2, (int(rs.randint(0, m)), 3)).astype(np.int32)     # a few indices fall outside
    v[rs.randint(0, m, 3)] = [np.nan, np.inf, 1.0]
    _assert_same_partition_with_minima_as_labels(v, f)


# ------------------------------------------------------------------------------------------------ hand cases

SQUARE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 2, 2], [3, 2, 2], [2, 3, 2], [9, 9, 9]], np.float32)


def test_two_triangles_sharing_one_vertex_or_none():
    one = R.components(SQUARE, [[0, 1, 2], [2, 4, 5]])
    assert one["labels"].tolist() == [0] and one["faces"].tolist() == [2] and one["face_labels"].tolist() == [0, 0]
    assert one["unreferenced"] == 3 and one["invalid"] == 0
    two = R.components(SQUARE, [[4, 5, 6], [1, 2, 3]])
    assert two["labels"].tolist() == [1, 4] and two["faces"].tolist() == [1, 1] and two["face_labels"].tolist() == [4, 1]
    assert two["lo"].tolist() == [[0, 0, 0], [2, 2, 2]] and two["hi"].tolist() == [[1, 1, 0], [3, 3, 2]]
    assert two["d2"].tolist() == [2.0, 2.0] and two["unreferenced"] == 2
    # output order is input order: face (4,5,6) first, vertices 1,2,3 before 4,5,6
    v, c, f, rep = R.clean(SQUARE, None, [[4, 5, 6], [1, 2, 3]])
    assert c is None and v.tolist() == SQUARE[1:7].tolist() and f.tolist() == [[3, 4, 5], [0, 1, 2]]
    assert rep["components"] == 2 and rep["vertices_out"] == 6 and rep["largest"] == [[1, 1, 2.0 ** 0.5], [4, 1, 2.0 ** 0.5]]


def test_a_face_that_repeats_an_index_is_valid():
    comp = R.components(SQUARE, [[3, 3, 5]])
    assert comp["labels"].tolist() == [3] and comp["faces"].tolist() == [1] and comp["invalid"] == 0 and comp["unreferenced"] == 6
    v, _, f, _ = R.clean(SQUARE, None, [[3, 3, 5]])
    assert v.tolist() == SQUARE[[3, 5]].tolist() and f.tolist() == [[0, 0, 1]]


def test_faces_that_name_no_vertex_and_vertices_that_are_not_finite():
    bad = [[-1, 0, 1], [0, 1, len(SQUARE)], [0, INT32_MAX, 1], [INT32_MIN, 0, 1]]
    comp = R.components(SQUARE, bad + [[0, 1, 2]])
    assert comp["face_labels"].tolist() == [-1, -1, -1, -1, 0] and comp["invalid"] == 4 and comp["labels"].tolist() == [0]
    v = SQUARE.copy()
    v[1, 2], v[5, 0] = np.nan, np.inf
    comp = R.components(v, [[0, 1, 2], [4, 5, 6], [2, 3, 4], [0, 2, 3]])
    assert comp["face_labels"].tolist() == [-1, -1, 0, 0] and comp["invalid"] == 2     # (2,3,4) and (0,2,3) share 2 and 3
    assert comp["unreferenced"] == 4                                                   # 1, 5, 6, 7
    cols = np.arange(24, dtype=np.uint8).reshape(8, 3)
    out_v, out_c, out_f, rep = R.clean(v, cols, [[0, 1, 2], [4, 5, 6], [2, 3, 4], [0, 2, 3]])
    assert out_v.tolist() == v[[0, 2, 3, 4]].tolist() and out_c.tolist() == cols[[0, 2, 3, 4]].tolist()
    assert out_f.tolist() == [[1, 2, 3], [0, 1, 2]] and rep["invalid_faces"] == 2 and rep["faces_out"] == 2


def test_empty_inputs_and_an_isolated_vertex():
    for v, f in ((np.zeros((0, 3)), np.zeros((0, 3))), (SQUARE, np.zeros((0, 3))), (np.zeros((0, 3)), [[0, 1, 2]])):
        out_v, out_c, out_f, rep = R.clean(v, None, f)
        assert out_v.shape == (0, 3) and out_f.shape == (0, 3) and rep["components"] == 0 and rep["largest"] == []
        assert rep["unreferenced"] == len(v) and rep["invalid_faces"] == len(f)
    comp = R.components(SQUARE, [[0, 1, 2]])
    assert comp["vertex_labels"].tolist() == [0, 0, 0, 3, 4, 5, 6, 7] and comp["unreferenced"] == 5


def test_keep_largest_ties_go_to_the_smaller_label_and_the_extent_bound_is_inclusive():
    faces = [[4, 5, 6], [0, 1, 2], [7, 7, 7]]
    comp = R.components(SQUARE, faces)
    assert comp["labels"].tolist() == [0, 4, 7] and comp["d2"].tolist() == [2.0, 2.0, 0.0]
    assert R.select(comp, keep_largest=1).tolist() == [True, False, False]
    assert R.select(comp, keep_largest=2).tolist() == [True, True, False]
    assert R.select(comp, keep_largest=5).tolist() == [True, True, True]
    root2 = float(np.sqrt(np.float32(2.0)))
    d2 = float(np.float32(root2) * np.float32(root2))
    # float32(sqrt 2)^2 rounds to 1.9999999 < 2: kept; the next float32 up squares to 2.0000002 > 2: dropped
    assert d2 < 2.0 and R.select(comp, min_extent=root2).tolist() == [True, True, False]
    assert R.select(comp, min_extent=float(np.nextafter(np.float32(root2), np.float32(2)))).tolist() == [False, False, False]
    # d2 exactly equal to min_extent^2 is kept: a box of extent (3, 4, 0) has d2 = 25 = 5 * 5
    v = np.array([[0, 0, 0], [3, 0, 0], [3, 4, 0]], np.float32)
    comp = R.components(v, [[0, 1, 2]])
    assert comp["d2"].tolist() == [25.0] and R.select(comp, min_extent=5.0).tolist() == [True]
    assert R.select(comp, min_extent=float(np.nextafter(np.float32(5), np.float32(6)))).tolist() == [False]
    # keep_largest ranks the passing components only
    assert R.select(R.components(SQUARE, faces + [[0, 2, 3]]), min_faces=1, min_extent=1.0, keep_largest=1).tolist() == [True, False, False]
    assert R.select(R.components(SQUARE, faces + [[0, 2, 3]]), min_faces=3, keep_largest=1).tolist() == [False, False, False]


# ------------------------------------------------------------------------------------------------ scene meshes

def _far(kind, vertices, faces):
    dist = M.scene(kind, noisy=True)["surface_distance"](vertices[np.unique(faces)]) / M.SCENE_VOXEL
    return int((dist > 2).sum()), float(dist.max())


def test_noisy_plane():
    v, c, f = R.scene_mesh("plane", True)
    _, _, _, rep = R.scene_clean("plane", True)
    assert (rep["vertices_in"], rep["faces_in"], rep["components"], rep["unreferenced"]) == (4256, 8158, 8, 32)
    assert [n for _, n, _ in rep["largest"]] == [8138, 4, 4, 4, 2, 2, 2, 2] and _far("plane", v, f)[0] == 34
    cv, cc, cf, rep = R.scene_clean("plane", True, min_faces=8)
    assert (len(cv), len(cf), rep["components_kept"]) == (4190, 8138, 1)
    far, worst = _far("plane", cv, cf)
    print("noisy plane, min_faces=8: %d far, worst %.4f voxels" % (far, worst))
    assert far == 0 and worst < 1.5
    for options in (dict(keep_largest=1), dict(min_extent=2 * M.SCENE_VOXEL)):
        ov, oc, of, _ = R.scene_clean("plane", True, **options)
        assert ov.tobytes() == cv.tobytes() and oc.tobytes() == cc.tobytes() and of.tobytes() == cf.tobytes()


def test_noisy_sphere():
    v, c, f = R.scene_mesh("sphere", True)
    _, _, _, rep = R.scene_clean("sphere", True)
    assert (rep["vertices_in"], rep["faces_in"], rep["components"], rep["unreferenced"]) == (4380, 7678, 10, 48)
    assert [n for _, n, _ in rep["largest"]] == [4014, 3522, 78, 24, 14, 8, 6, 6, 4, 2] and _far("sphere", v, f)[0] == 66
    cv, cc, cf, rep = R.scene_clean("sphere", True, min_extent=5 * M.SCENE_VOXEL)
    assert (len(cv), len(cf), rep["components_kept"]) == (4263, 7614, 3) and _far("sphere", cv, cf)[0] == 14


def test_clean_scenes():
    v, c, f = R.scene_mesh("plane", False)
    cv, cc, cf, rep = R.scene_clean("plane", False, min_faces=8)
    assert cv.tobytes() == v.tobytes() and cc.tobytes() == c.tobytes() and cf.tobytes() == f.tobytes() and rep["components"] == 1
    _, _, _, rep = R.scene_clean("sphere", False)
    assert [n for _, n, _ in rep["largest"]] == [4064, 3400, 80, 58, 40, 6] and rep["unreferenced"] == 5


# ------------------------------------------------------------------------------------------------ host side of the module

BAD_OPTIONS = (dict(min_faces=-1), dict(min_faces=1.5), dict(min_faces=True), dict(min_faces="a"), dict(keep_largest=-1),
               dict(keep_largest=0.5), dict(min_extent=-0.1), dict(min_extent=np.nan), dict(min_extent=np.inf), dict(min_extent="x"),
               dict(min_extent=None))


def test_option_checks_come_before_any_gpu_work():
    from mvsnet_amd import mesh, mesh_clean
    assert mesh_clean.check_options() == (0, 0.0, 0) and mesh_clean.check_options(np.int64(3), 1, 2.0) == (3, 1.0, 2)
    assert not mesh_clean.wanted(0, 0.0, 0) and mesh_clean.wanted(0, 0.5, 0) and mesh_clean.wanted(1, 0, 0) and mesh_clean.wanted(0, 0, 1)
    f = np.zeros((1, 3), np.int32)
    for bad in BAD_OPTIONS:
        with pytest.raises(ValueError):
            mesh_clean.check_options(**bad)
        with pytest.raises(ValueError):
            mesh_clean.clean_mesh(SQUARE, None, f, **bad)                      # a ValueError with or without a GPU
    z = np.zeros((2, 4, 4), np.float32)
    for bad in (dict(min_component_faces=-1), dict(min_component_extent=np.nan), dict(keep_largest=1.5)):
        with pytest.raises(ValueError):
            mesh.mesh_depth_maps(z, z, np.zeros((2, 2, 4, 4)), **bad)
    for args in ((SQUARE[:, :2], None, f), (SQUARE, None, f[:, :2]), (SQUARE, np.zeros((3, 3), np.uint8), f), (SQUARE, None, 7)):
        with pytest.raises(ValueError):
            mesh_clean.clean_mesh(*args)
    with pytest.raises(ValueError):
        mesh_clean.mesh_components(SQUARE, f[0])
    with pytest.raises(ValueError):
        mesh_clean.clean_mesh(SQUARE, None, f, device="cpu")


def test_the_three_command_lines_check_their_options(tmp_path):
    from mvsnet_amd import depthfusion, mesh, mesh_clean
    src, out = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    a = mesh_clean.parse_args(["--mesh", src, "--out", out])
    assert (a.min_component_faces, a.min_component_extent, a.keep_largest, a.force) == (0, 0.0, 0, False)
    a = mesh_clean.parse_args(["--mesh", src, "--out", out, "--min_component_faces", "8", "--min_component_extent", "0.25",
                               "--keep_largest", "2", "--force"])
    assert (a.min_component_faces, a.min_component_extent, a.keep_largest, a.force) == (8, 0.25, 2, True)
    bad = (["--min_component_faces", "-1"], ["--min_component_faces", "1.5"], ["--min_component_extent", "-1"],
           ["--min_component_extent", "nan"], ["--min_component_extent", "inf"], ["--keep_largest", "-2"])
    for extra in bad:
        with pytest.raises(SystemExit):
            mesh_clean.parse_args(["--mesh", src, "--out", out] + extra)
        with pytest.raises(SystemExit):
            mesh.parse_args(["--dense_folder", str(tmp_path)] + extra)
    for missing in (["--mesh", src], ["--out", out]):
        with pytest.raises(SystemExit):
            mesh_clean.parse_args(missing)
    # an existing output is refused before any GPU work
    open(out, "wb").close()
    with pytest.raises(SystemExit) as e:
        mesh_clean.main(["--mesh", src, "--out", out])
    assert "--force" in str(e.value)
    assert mesh_clean.prepare_output(mesh_clean.parse_args(["--mesh", src, "--out", out, "--force"])) == out
    a = mesh.parse_args(["--dense_folder", str(tmp_path)])
    assert (a.min_component_faces, a.min_component_extent, a.keep_largest) == (0, 0.0, 0)
    a = mesh.parse_args(["--dense_folder", str(tmp_path), "--min_component_faces", "8", "--keep_largest", "1"])
    assert (a.min_component_faces, a.min_component_extent, a.keep_largest) == (8, 0.0, 1)
    # depthfusion: refused without --mesh, like the other dependent flags, and checked before any work
    for extra in (["--mesh_min_component_faces", "8"], ["--mesh_min_component_extent", "0.1"], ["--mesh_keep_largest", "1"]):
        with pytest.raises(SystemExit) as e:
            depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--fusion", "hip"] + extra)
        assert "needs --mesh" in str(e.value)
    for extra in (["--mesh_min_component_faces", "-1"], ["--mesh_min_component_extent", "nan"], ["--mesh_keep_largest", "-1"]):
        with pytest.raises(SystemExit) as e:
            depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--fusion", "hip", "--mesh"] + extra)
        assert ">= 0" in str(e.value)
    with pytest.raises(SystemExit) as e:
        depthfusion.main(["--dense_folder", str(tmp_path / "none"), "--mesh", "--mesh_keep_largest", "1"])
    assert "--mesh needs --fusion hip" in str(e.value)
    assert not (tmp_path / "none").exists()


def test_library_checks_arguments_before_any_gpu_call(lib_built):
    """Argument validation happens before the first HIP call, so the codes are testable without a GPU: the pointers below are
    host buffers that a kernel must never see."""
    from mvsnet_amd import _lib, build
    h = _lib.load()
    assert "mesh_components.hip" in build.SOURCES
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 2 ** 31
    wsb = h.mvs_mesh_components_workspace_bytes
    assert wsb(0, 0) == 256 + 2 * 256 and wsb(1, 5) == 768 and wsb(64, 0) == 768 and wsb(65, 1) == 256 + 2 * 512
    assert wsb(-1, 0) == 0 and wsb(0, -1) == 0 and wsb(big, 1) == 0 and wsb(1, big) == 0 and wsb(big - 1, big - 1) == 256 + 2 ** 34
    label = lambda v=p, M=8, f=p, F=4, vl=p, fl=p, ws=p, n=4096: h.mvs_mesh_components_label_i32(v, M, f, F, vl, fl, ws, n, None)
    for kw in (dict(v=None), dict(f=None), dict(vl=None), dict(fl=None), dict(ws=None), dict(M=-1), dict(F=-1)):
        assert label(**kw) == -1, kw
    assert label(M=big) == -2 and label(F=big) == -2 and label(n=767) == -3 and label(M=1000, n=4095) == -3
    measure = lambda v=p, M=8, F=4, vl=p, fl=p, cnt=p, box=p, ws=p, n=4096: h.mvs_mesh_components_measure_f32(
        v, M, F, vl, fl, cnt, box, ws, n, None)
    for kw in (dict(v=None), dict(vl=None), dict(fl=None), dict(cnt=None), dict(box=None), dict(ws=None), dict(M=-1), dict(F=-1)):
        assert measure(**kw) == -1, kw
    assert measure(M=big) == -2 and measure(F=big) == -2 and measure(n=0) == -3
    mark = lambda f=p, M=8, F=4, fl=p, kl=p, fk=p, vk=p: h.mvs_mesh_compact_mark_i32(f, M, F, fl, kl, fk, vk, None)
    for kw in (dict(f=None), dict(fl=None), dict(kl=None), dict(fk=None), dict(vk=None), dict(M=-1), dict(F=-1)):
        assert mark(**kw) == -1, kw
    assert mark(M=big) == -2 and mark(F=big) == -2
    write = lambda v=p, c=p, M=8, f=p, F=4, fk=p, fr=p, vk=p, vr=p, Mo=3, Fo=1, ov=p, oc=p, of=p: h.mvs_mesh_compact_write_f32(
        v, c, M, f, F, fk, fr, vk, vr, Mo, Fo, ov, oc, of, None)
    for kw in (dict(v=None), dict(f=None), dict(fk=None), dict(fr=None), dict(vk=None), dict(vr=None), dict(ov=None), dict(of=None),
               dict(c=None), dict(oc=None), dict(M=-1), dict(F=-1), dict(Mo=-1), dict(Fo=-1), dict(Mo=9), dict(Fo=5)):
        assert write(**kw) == -1, kw
    assert write(M=big) == -2 and write(F=big) == -2
    assert write(Mo=0, Fo=0, ov=None, oc=None, of=None) == 0                   # an empty result: nothing is launched
    assert buf.raw == b"\0" * 4096                                             # nothing was written
