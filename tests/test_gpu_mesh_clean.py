"""GPU tests of the connected components, measures and compaction of csrc/mesh_components.hip through mvsnet_amd.mesh_clean,
against tests/mesh_clean_reference.py byte for byte (boxes by value): the six scene meshes under every kind of option, meshes
built to show diameter-bound work, a wrong hook, one hot word and grid strides, sizes around a wave, invalid faces between
guard words, reproducibility, the error word after every call, the hooks in mvsnet_amd.mesh and the three command lines."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mesh_clean_reference as R
from tests import mesh_reference as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = [dict(), dict(min_faces=8), dict(min_extent=2 * M.SCENE_VOXEL), dict(min_extent=5 * M.SCENE_VOXEL), dict(keep_largest=1),
           dict(keep_largest=2), dict(min_faces=8, keep_largest=3)]


def _assert_clean(got, want):
    (v, c, f, rep), (wv, wc, wf, wrep) = got, want
    print("vertices %d (want %d), faces %d (want %d); report %s" % (len(v), len(wv), len(f), len(wf), json.dumps(rep)))
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == wv.shape and f.shape == wf.shape
    assert v.tobytes() == wv.tobytes() and f.tobytes() == wf.tobytes()
    assert (c is None) == (wc is None)
    if c is not None:
        assert c.dtype == np.uint8 and c.tobytes() == wc.tobytes()
    assert rep["error_word"] == 0                                              # read back by the call, asserted here
    assert rep == wrep


def _assert_components(got, want):
    assert got["error_word"] == 0
    assert got["face_labels"].dtype == np.int32 and got["face_labels"].tobytes() == want["face_labels"].tobytes()
    assert got["labels"].tobytes() == want["labels"].tobytes() and got["faces"].tobytes() == want["faces"].tobytes()
    assert got["lo"].dtype == np.float32 and np.array_equal(got["lo"], want["lo"]) and np.array_equal(got["hi"], want["hi"])
    assert (got["unreferenced"], got["invalid"]) == (want["unreferenced"], want["invalid"])


def _check(vertices, colours, faces, **options):
    from mvsnet_amd import mesh_clean
    got = mesh_clean.clean_mesh(vertices, colours, faces, **options)
    _assert_clean(got, R.clean(vertices, colours, faces, **options))
    return got


# ------------------------------------------------------------------------------------------------ scene meshes

@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("kind,noisy", R.SCENES)
def test_scene_meshes_equal_the_reference(kind, noisy, colour):
    from mvsnet_amd import mesh_clean
    v, c, f = R.scene_mesh(kind, noisy)
    _assert_components(mesh_clean.mesh_components(v, f), R.components(v, f))
    for options in OPTIONS:
        want = R.scene_clean(kind, noisy, **options)
        if not colour:
            want = (want[0], None, want[2], want[3])
        _assert_clean(mesh_clean.clean_mesh(v, c if colour else None, f, **options), want)


def test_the_noisy_plane_loses_its_fragments():
    from mvsnet_amd import mesh_clean
    v, c, f = R.scene_mesh("plane", True)
    ov, oc, of, rep = mesh_clean.clean_mesh(v, c, f, min_faces=8)
    assert (len(ov), len(of), rep["components"], rep["components_kept"], rep["unreferenced"]) == (4190, 8138, 8, 1, 32)
    dist = M.scene("plane", noisy=True)["surface_distance"](ov[np.unique(of)]) / M.SCENE_VOXEL
    assert dist.max() < 1.5


# ------------------------------------------------------------------------------------------------ built meshes

_strip, _grid = R.strip, R.grid            # the built meshes live beside the reference: test_gpu_arena_geometry.py uses them too


@pytest.mark.parametrize("seed", [0, 1])
def test_a_long_strip_is_one_component(seed):
    from mvsnet_amd import mesh_clean
    v, f = _strip(20000, seed)
    got = mesh_clean.mesh_components(v, f)
    assert got["labels"].tolist() == [0] and got["faces"].tolist() == [20000] and (got["face_labels"] == 0).all()
    assert got["unreferenced"] == 0 and got["error_word"] == 0
    _assert_components(got, R.components(v, f))
    _check(v, None, f, min_faces=3)


def test_a_strip_cut_into_seven_pieces():
    from mvsnet_amd import mesh_clean
    v, f = _strip(20000, 2, cuts=7)
    want = R.components(v, f)
    assert len(want["labels"]) == 7
    _assert_components(mesh_clean.mesh_components(v, f), want)
    _check(v, None, f, keep_largest=3)
    got = _check(v, None, f, min_extent=1428.3)                         # the first piece is one face longer than the others
    assert got[3]["components_kept"] == 1


def test_separate_triangles_are_as_many_components():
    from mvsnet_amd import mesh_clean
    n = 50000
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    v = np.random.RandomState(4).rand(3 * n, 3).astype(np.float32)
    got = mesh_clean.mesh_components(v, f)
    assert len(got["labels"]) == n and np.array_equal(got["labels"], 3 * np.arange(n)) and (got["faces"] == 1).all()
    _assert_components(got, R.components(v, f))
    ov, _, of, rep = _check(v, None, f, keep_largest=3)
    assert rep["components"] == n and [row[0] for row in rep["largest"][:3]] == [0, 3, 6] and of.tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    assert ov.tobytes() == v[:9].tobytes()


def test_one_hot_word():
    rs = np.random.RandomState(5)
    v = rs.randn(9000, 3).astype(np.float32)
    f = rs.randint(1, 9000, (4096, 3)).astype(np.int32)
    f[np.arange(4096), rs.randint(0, 3, 4096)] = 0                             # every face names vertex 0
    got = _check(v, None, f)
    assert got[3]["components"] == 1 and got[3]["largest"][0][:2] == [0, 4096]
    same = np.tile(np.array([[7, 3, 5]], np.int32), (4096, 1))                 # 4 096 copies of one face
    got = _check(v, None, same, min_faces=4096)
    assert got[3]["largest"][0][:2] == [3, 4096] and got[3]["vertices_out"] == 3 and got[3]["unreferenced"] == 8997


def test_a_grid_of_quads():
    v, f = _grid(300)
    assert len(f) == 180000
    got = _check(v, None, f, min_faces=8)
    assert got[3]["components"] == 1 and got[3]["faces_out"] == 180000
    v, f = _grid(300, gap=50)
    got = _check(v, None, f, keep_largest=4)
    assert got[3]["components"] == 6 and got[3]["components_kept"] == 4 and [row[0] for row in got[3]["largest"][:2]] == [0, 50 * 301]


@pytest.mark.parametrize("n_faces", [0, 1, 63, 64, 65])
def test_sizes_around_a_wave(n_faces):
    v, f = _grid(8)
    _check(v, np.arange(3 * len(v), dtype=np.uint8).reshape(-1, 3), f[:n_faces])
    _check(v, None, f[::2][:n_faces], min_faces=2)


def test_no_vertices():
    from mvsnet_amd import mesh_clean
    none = np.zeros((0, 3), np.float32)
    _check(none, None, np.zeros((0, 3), np.int32))
    got = _check(none, np.zeros((0, 3), np.uint8), np.array([[0, 1, 2], [0, 0, 0]], np.int32), keep_largest=1)
    assert got[3]["invalid_faces"] == 2 and got[3]["components"] == 0
    comp = mesh_clean.mesh_components(none, np.zeros((0, 3), np.int32))
    assert comp["labels"].shape == (0,) and comp["lo"].shape == (0, 3) and comp["error_word"] == 0


# ------------------------------------------------------------------------------------------------ invalid faces, guards, errors

def test_invalid_faces_and_vertices_between_guard_words():
    """The arrays sit inside larger device buffers filled with a guard value: a face that names no vertex is never dereferenced
    (an index of INT32_MAX would land far outside), and nothing beside the outputs is written."""
    import torch
    from mvsnet_amd import mesh_clean
    rs = np.random.RandomState(8)
    v, f = (a.copy() for a in _grid(12))
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    f[5], f[17], f[40], f[99] = [-1, 0, 1], [0, 1, len(v)], [3, 2 ** 31 - 1, 4], [-2 ** 31, 7, 8]
    v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
    v[3, 2], v[4, 2] = -0.0, 0.0
    want = R.clean(v, c, f, min_faces=2)
    assert want[3]["invalid_faces"] > 4 and want[3]["components"] >= 1
    G = 64
    vb = torch.full((G + v.size + G,), 12345.0, dtype=torch.float32, device="cuda")
    fb = torch.full((G + f.size + G,), 1 << 30, dtype=torch.int32, device="cuda")
    cb = torch.full((G + c.size + G,), 201, dtype=torch.uint8, device="cuda")
    vb[G:G + v.size], fb[G:G + f.size], cb[G:G + c.size] = (torch.as_tensor(a.reshape(-1)).cuda() for a in (v, f, c))
    tv, tf, tc = vb[G:G + v.size].view(-1, 3), fb[G:G + f.size].view(-1, 3), cb[G:G + c.size].view(-1, 3)
    ov, oc, of, rep = mesh_clean.clean_mesh(tv, tc, tf, min_faces=2)
    assert isinstance(ov, torch.Tensor) and ov.is_cuda                          # tensors in, tensors out
    _assert_clean((ov.cpu().numpy(), oc.cpu().numpy(), of.cpu().numpy(), rep), want)
    _assert_components(mesh_clean.mesh_components(tv, tf), R.components(v, f))
    for buf, guard, n in ((vb, 12345.0, v.size), (fb, 1 << 30, f.size), (cb, 201, c.size)):
        assert (buf[:G] == guard).all() and (buf[G + n:] == guard).all()
    assert vb[G:G + v.size].cpu().numpy().tobytes() == v.tobytes() and fb[G:G + f.size].cpu().numpy().tobytes() == f.tobytes()


def test_bad_arguments_return_their_codes_and_leave_the_buffers_alone():
    import torch
    from mvsnet_amd import _lib
    h = _lib.load()
    ptr = _lib.ptr
    v, f = _grid(4)
    M_, F_ = len(v), len(f)
    tv, tf = torch.as_tensor(v).cuda(), torch.as_tensor(f).cuda()
    out = [torch.full((8 * M_ + 8 * F_,), 77, dtype=torch.int32, device="cuda") for _ in range(6)]
    ws = torch.full((4096,), 9, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr()
    assert h.mvs_mesh_components_label_i32(ptr(tv), M_, ptr(tf), F_, ptr(out[0]), ptr(out[1]), ptr(ws), 767, st) == -3
    assert h.mvs_mesh_components_label_i32(ptr(tv), -1, ptr(tf), F_, ptr(out[0]), ptr(out[1]), ptr(ws), 4096, st) == -1
    assert h.mvs_mesh_components_label_i32(ptr(tv), M_, None, F_, ptr(out[0]), ptr(out[1]), ptr(ws), 4096, st) == -1
    assert h.mvs_mesh_components_label_i32(ptr(tv), M_, ptr(tf), 2 ** 31, ptr(out[0]), ptr(out[1]), ptr(ws), 4096, st) == -2
    assert h.mvs_mesh_components_measure_f32(ptr(tv), M_, F_, ptr(out[0]), ptr(out[1]), None, ptr(out[3]), ptr(ws), 4096, st) == -1
    assert h.mvs_mesh_components_measure_f32(ptr(tv), M_, F_, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(ws), 16, st) == -3
    assert h.mvs_mesh_compact_mark_i32(ptr(tf), M_, F_, ptr(out[1]), None, ptr(out[4]), ptr(out[5]), st) == -1
    assert h.mvs_mesh_compact_mark_i32(ptr(tf), 2 ** 31, F_, ptr(out[1]), ptr(out[0]), ptr(out[4]), ptr(out[5]), st) == -2
    assert h.mvs_mesh_compact_write_f32(ptr(tv), None, M_, ptr(tf), F_, ptr(out[4]), ptr(out[4]), ptr(out[5]), ptr(out[5]), M_ + 1, 1,
                                        ptr(out[2]), None, ptr(out[3]), st) == -1
    assert h.mvs_mesh_compact_write_f32(ptr(tv), None, M_, ptr(tf), F_, ptr(out[4]), ptr(out[4]), ptr(out[5]), ptr(out[5]), 1, 1,
                                        None, None, ptr(out[3]), st) == -1
    torch.cuda.synchronize()
    assert all((o == 77).all() for o in out) and (ws == 9).all()
    assert tv.cpu().numpy().tobytes() == v.tobytes() and tf.cpu().numpy().tobytes() == f.tobytes()


def test_two_runs_and_a_side_stream_give_the_same_bytes():
    import torch
    from mvsnet_amd import mesh_clean
    v, c, f = R.scene_mesh("sphere", True)
    rs = np.random.RandomState(3)
    f = f[rs.permutation(len(f))]
    runs = [mesh_clean.clean_mesh(v, c, f, min_faces=4, keep_largest=5) for _ in range(2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(mesh_clean.clean_mesh(v, c, f, min_faces=4, keep_largest=5))
        comp = mesh_clean.mesh_components(v, f)
    side.synchronize()
    _assert_components(comp, R.components(v, f))
    for run in runs:
        assert run[3]["error_word"] == 0 and run[3] == runs[0][3]
        for a, b in zip(run[:3], runs[0][:3]):
            assert a.tobytes() == b.tobytes()
    _assert_clean(runs[0], R.clean(v, c, f, min_faces=4, keep_largest=5))


# ------------------------------------------------------------------------------------------------ mesh.py and the command lines

def _noisy_volume(kind):
    from mvsnet_amd import mesh
    sc = M.scene(kind, noisy=True)
    vol = mesh.TsdfVolume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, M.SCENE_TRUNC, colour=True)
    return vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"])


def test_extract_with_clean_equals_clean_mesh_of_extract():
    from mvsnet_amd import mesh_clean
    vol = _noisy_volume("sphere")
    plain = vol.extract()
    assert len(plain) == 3
    for got, want in zip(plain, R.scene_mesh("sphere", True)):
        assert got.tobytes() == want.tobytes()
    for options in (dict(min_faces=8), dict(min_extent=5 * M.SCENE_VOXEL, keep_largest=2), dict()):
        _assert_clean(vol.extract(clean=options), mesh_clean.clean_mesh(*plain, **options))
    _assert_clean(vol.extract(clean=dict(min_extent=5 * M.SCENE_VOXEL)), R.scene_clean("sphere", True, min_extent=5 * M.SCENE_VOXEL))
    with pytest.raises(ValueError):
        vol.extract(clean=dict(min_faces=-1))


def test_mesh_depth_maps_removes_the_fragments_of_the_noisy_plane():
    from mvsnet_amd import mesh
    sc = M.scene("plane", noisy=True)
    bounds = (np.array(M.SCENE_ORIGIN, np.float64), np.array(M.SCENE_ORIGIN, np.float64) + M.SCENE_VOXEL * (np.array(M.SCENE_DIMS) - 1))
    kw = dict(voxel=M.SCENE_VOXEL, bounds=bounds, num_consistent=0)
    v, c, f = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], **kw)
    print("raw: %d vertices, %d faces" % (len(v), len(f)))
    cv, cc, cf = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], min_component_faces=8, **kw)
    print("cleaned: %d vertices, %d faces" % (len(cv), len(cf)))
    want = R.clean(v, c, f, min_faces=8)
    assert cv.tobytes() == want[0].tobytes() and cc.tobytes() == want[1].tobytes() and cf.tobytes() == want[2].tobytes()
    assert (len(cv), len(cf)) == (4190, 8138)


def _write_dense(folder, s):
    from mvsnet_amd import predictlib
    out = os.path.join(folder, "depths_mvsnet")
    os.makedirs(out)
    for i in range(s["depths"].shape[0]):
        predictlib.write_output_slice(out, s["depths"][i], s["probs"][i], s["images"][i][:, :, ::-1], s["cams"][i], i)


def _run(*argv):
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m"] + list(argv), cwd=ROOT, capture_output=True, text=True)
    return r.returncode, r.stdout[-4000:] + r.stderr[-2000:]


def _json_line(text, prefix=""):
    line = [ln for ln in text.splitlines() if ln.startswith(prefix + "{")][-1]
    return json.loads(line[len(prefix):])


COMMON = ["--voxel", "0.05", "--num_consistent", "0", "--bounds=-1.4:-1.2:2.9:1.35:1.15:6.05"]


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    """The noisy plane as a dense folder, and its mesh without any cleaning, shared by the command-line tests."""
    from mvsnet_amd import fusion, mesh
    folder = str(tmp_path_factory.mktemp("dense"))
    _write_dense(folder, M.scene("plane", noisy=True))
    idx, d, p, cams, im = fusion.load_dense_folder(folder)
    raw = mesh.mesh_depth_maps(d, p, cams, im, voxel=0.05, num_consistent=0, bounds=mesh.parse_bounds(COMMON[-1].split("=")[1]))
    return folder, raw


def test_mesh_command_line_without_the_options_writes_the_bytes_of_the_extraction(dense, tmp_path):
    from mvsnet_amd import mesh
    folder, raw = dense
    plain, want = str(tmp_path / "plain.ply"), str(tmp_path / "want.ply")
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", folder, *COMMON, "--out", plain)
    assert code == 0, text
    mesh.write_mesh_ply(want, *raw)
    assert open(plain, "rb").read() == open(want, "rb").read()
    assert set(_json_line(text)) == {"views", "vertices", "faces", "out"}      # no new report field


def test_mesh_command_line_with_min_component_faces(dense, tmp_path):
    from mvsnet_amd import mesh
    folder, raw = dense
    cleaned, want = str(tmp_path / "cleaned.ply"), str(tmp_path / "want.ply")
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", folder, *COMMON, "--out", cleaned, "--min_component_faces", "8")
    assert code == 0, text
    ref = R.clean(*raw, min_faces=8)
    rep = _json_line(text)
    assert len(ref[2]) < len(raw[2]) and rep["components_kept"] == 1 and rep["error_word"] == 0
    assert {k: rep[k] for k in ref[3]} == ref[3] and rep["vertices"] == len(ref[0]) and rep["faces"] == len(ref[2])
    mesh.write_mesh_ply(want, *ref[:3])
    assert open(cleaned, "rb").read() == open(want, "rb").read()


def test_mesh_clean_command_line_on_a_written_ply(dense, tmp_path):
    from mvsnet_amd import mesh
    folder, raw = dense
    plain, again, want = str(tmp_path / "plain.ply"), str(tmp_path / "again.ply"), str(tmp_path / "want.ply")
    mesh.write_mesh_ply(plain, *raw)
    code, text = _run("mvsnet_amd.mesh_clean", "--mesh", plain, "--out", again, "--min_component_faces", "8")
    assert code == 0, text
    ref = R.clean(*raw, min_faces=8)
    rep = _json_line(text)
    assert {k: rep[k] for k in ref[3]} == ref[3] and rep["out"] == again
    mesh.write_mesh_ply(want, *ref[:3])
    assert open(again, "rb").read() == open(want, "rb").read()
    code, text = _run("mvsnet_amd.mesh_clean", "--mesh", plain, "--out", again, "--keep_largest", "1")   # refused before any GPU work
    assert code != 0 and "--force" in text


def test_depthfusion_command_line_passes_the_options_through(dense):
    from mvsnet_amd import mesh
    folder, _ = dense
    code, text = _run("mvsnet_amd.depthfusion", "--dense_folder", folder, "--fusion", "hip", "--mesh", "--mesh_min_component_faces", "8")
    assert code == 0, text
    rep = _json_line(text, "meshed: ")
    assert rep["error_word"] == 0 and rep["faces_out"] == rep["faces"] and rep["components_kept"] <= rep["components"]
    v2, c2, f2 = mesh.read_mesh_ply(rep["out"])
    assert len(f2) == rep["faces_out"] and len(v2) == rep["vertices_out"]
    comp = R.components(v2, f2)
    assert comp["unreferenced"] == 0 and comp["faces"].min() >= 8
