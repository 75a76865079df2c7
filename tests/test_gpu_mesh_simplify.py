"""GPU tests of the vertex clustering of csrc/mesh_simplify.hip through mvsnet_amd.mesh_simplify, against
tests/mesh_simplify_reference.py byte for byte: the six scene meshes and the analytic sphere at several cells, origins that put
vertices out of range, one hot cluster and runs that straddle waves and workgroups, quad grids, duplicates, sizes around a
wave, invalid faces between guard words, the two-key sort of the faces, reproducibility, refused arguments, the hooks in
mvsnet_amd.mesh and the three command lines."""
import json
import os

import numpy as np
import pytest

from tests import mesh_clean_reference as MC
from tests import mesh_reference as M
from tests import mesh_simplify_reference as R
from tests.test_gpu_mesh_clean import COMMON, _json_line, _noisy_volume, _run, dense  # noqa: F401  (dense is a fixture)

pytestmark = pytest.mark.gpu
SCENE_O = np.asarray(M.SCENE_ORIGIN, np.float32)


def _assert_same(got, want):
    (v, c, f, rep), (wv, wc, wf, wrep) = got, want
    print("vertices %d (want %d), faces %d (want %d); report %s" % (len(v), len(wv), len(f), len(wf), json.dumps(rep)))
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == wv.shape and f.shape == wf.shape
    assert v.tobytes() == wv.tobytes() and f.tobytes() == wf.tobytes()
    assert (c is None) == (wc is None)
    if c is not None:
        assert c.dtype == np.uint8 and c.tobytes() == wc.tobytes()
    assert rep == wrep


def _check(vertices, colours, faces, cell, origin=None, **kw):
    from mvsnet_amd import mesh_simplify
    got = mesh_simplify.simplify_mesh(vertices, colours, faces, cell, origin, **kw)
    _assert_same(got, R.simplify(vertices, colours, faces, cell, origin))
    return got


# ------------------------------------------------------------------------------------------------ the project's meshes

@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("kind,noisy", MC.SCENES + [("analytic", False)])
def test_scene_meshes_equal_the_reference(kind, noisy, colour):
    if kind == "analytic":
        m = M.extract(M.analytic_sphere())
        v, c, f, origin, voxel = m["vertices"], m["colours"], m["faces"], np.asarray(M.SPHERE_ORIGIN, np.float32), M.SPHERE_VOXEL
    else:
        (v, c, f), origin, voxel = MC.scene_mesh(kind, noisy), SCENE_O, M.SCENE_VOXEL
    for mult in (1, 2, 3, 100):
        got = _check(v, c if colour else None, f, R.voxels(mult, voxel), origin)
        if mult == 100:
            assert got[3]["clusters"] == 1 and got[3]["faces_out"] == 0 and got[3]["vertices_out"] == 0
            assert got[3]["degenerate_faces"] == len(f)
    if kind == "analytic":
        assert (got[3]["vertices_in"], got[3]["faces_in"]) == (1212, 2420)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_origins_that_put_vertices_out_of_range(axis):
    v, c, f = MC.scene_mesh("sphere", False)
    origin = SCENE_O.copy()
    origin[axis] = np.median(v[:, axis])                                       # half of the vertices have k < 0 on this axis
    got = _check(v, c, f, 0.1, origin)
    assert 0 < got[3]["unclusterable_vertices"] < len(v) and 0 < got[3]["invalid_faces"] < len(f) and got[3]["faces_out"] > 0
    cell = np.float32(np.ptp(v[:, axis]) / 2 ** 22)                            # and here k >= 2^21 beyond the middle of the axis
    origin = v.min(0)
    got = _check(v, c, f, cell, origin)
    assert 0 < got[3]["unclusterable_vertices"] < len(v) and 0 < got[3]["invalid_faces"] < len(f)


# ------------------------------------------------------------------------------------------------ built meshes

@pytest.mark.parametrize("seed", [0, 1])
def test_one_cell_strip_and_runs_across_waves(seed):
    """The strip's two rows of vertices are 60 apart.  A cell larger than the strip: all 20 002 vertices accumulate on one
    cluster (the hot word), and one more face to two far vertices carries that cluster into the output.  A cell of 50: runs of
    100 sorted positions, which straddle waves and workgroups; the faces across cell borders survive."""
    v, f = (a.copy() for a in MC.strip(20000, seed))
    v[:, 1] *= 60
    n = len(v)
    v = np.concatenate([v, np.array([[12000, 0, 0], [0, 12000, 0]], np.float32)])
    f = np.concatenate([f, np.array([[5, n, n + 1]], np.int32)])
    c = np.random.RandomState(seed).randint(0, 256, (len(v), 3)).astype(np.uint8)
    origin = np.array([-1, -1, -1], np.float32)
    got = _check(v, c, f, 11000.0, origin)
    assert got[3]["clusters"] == 3 and got[3]["faces_out"] == 1 and got[3]["degenerate_faces"] == 20000
    got = _check(v, c, f, 50.0, origin)
    assert got[3]["clusters"] > 200 and got[3]["faces_out"] > 200
    _check(v, None, f, 50.0, origin)


@pytest.mark.parametrize("quads", [1.5, 2, 7])
def test_a_grid_of_quads(quads):
    v, f = MC.grid(300)
    got = _check(v, None, f, np.float32(quads * 0.25))
    assert got[3]["faces_out"] < len(f) / 2 and got[3]["invalid_faces"] == 0


def test_duplicates():
    rs = np.random.RandomState(5)
    v = rs.randn(9000, 3).astype(np.float32)
    same = np.tile(np.array([[7, 3, 5]], np.int32), (4096, 1))                 # 4 096 copies of one face
    same[1::2] = same[1::2, ::-1]                                              # every other one with the other orientation
    got = _check(v, None, same, 0.01)
    assert got[3]["faces_out"] == 1 and got[3]["duplicate_faces"] == 4095 and got[3]["vertices_out"] == 3 and got[3]["clusters"] == 3
    assert np.abs(got[0][got[2][0]] - v[[7, 3, 5]]).max() < 1e-6               # face 0 stays, with its own winding
    f = rs.randint(1, 9000, (4096, 3)).astype(np.int32)
    f[np.arange(4096), rs.randint(0, 3, 4096)] = 0                             # every face names vertex 0
    _check(v, None, f, 0.01)
    got = _check(v, None, f, 0.5)
    assert got[3]["duplicate_faces"] > 0 and got[3]["degenerate_faces"] > 0


@pytest.mark.parametrize("n_vertices", [0, 1, 63, 64, 65])
def test_sizes_around_a_wave(n_vertices):
    v, f = MC.grid(8)
    origin = np.array([-0.1, -0.1, -0.1], np.float32)
    c = np.arange(3 * len(v), dtype=np.uint8).reshape(-1, 3)
    for n_faces in (0, 1, 63, 64, 65):
        _check(v[:n_vertices], c[:n_vertices], f[:n_faces], 0.3, origin)       # faces beyond the vertices are invalid
        _check(v[:n_vertices], None, f[::2][:n_faces], 0.6, origin)


def test_no_finite_vertex():
    from mvsnet_amd import mesh_simplify
    none = np.zeros((0, 3), np.float32)
    _check(none, None, np.zeros((0, 3), np.int32), 1.0)
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(none, None, np.array([[0, 1, 2]], np.int32), 1.0)
    import torch
    nan = torch.full((4, 3), float("nan"), device="cuda")
    with pytest.raises(ValueError):
        mesh_simplify.simplify_mesh(nan, None, torch.zeros((1, 3), dtype=torch.int32, device="cuda"), 1.0)


# ------------------------------------------------------------------------------------------------ invalid faces, guards, errors

def test_invalid_faces_and_vertices_between_guard_words():
    """The arrays sit inside larger device buffers filled with a guard value: a face that names no vertex is never dereferenced,
    and nothing beside the outputs is written."""
    import torch
    from mvsnet_amd import mesh_simplify
    rs = np.random.RandomState(8)
    v, f = (a.copy() for a in MC.grid(12))
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    f[5], f[17], f[40], f[99] = [-1, 0, 1], [0, 1, len(v)], [3, 2 ** 31 - 1, 4], [-2 ** 31, 7, 8]
    v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
    want = R.simplify(v, c, f, 0.4)
    assert want[3]["invalid_faces"] > 4 and want[3]["unclusterable_vertices"] == 3 and want[3]["faces_out"] > 0
    G = 64
    vb = torch.full((G + v.size + G,), 12345.0, dtype=torch.float32, device="cuda")
    fb = torch.full((G + f.size + G,), 1 << 30, dtype=torch.int32, device="cuda")
    cb = torch.full((G + c.size + G,), 201, dtype=torch.uint8, device="cuda")
    vb[G:G + v.size], fb[G:G + f.size], cb[G:G + c.size] = (torch.as_tensor(a.reshape(-1)).cuda() for a in (v, f, c))
    tv, tf, tc = vb[G:G + v.size].view(-1, 3), fb[G:G + f.size].view(-1, 3), cb[G:G + c.size].view(-1, 3)
    ov, oc, of, rep = mesh_simplify.simplify_mesh(tv, tc, tf, 0.4)              # the default origin, found on the device
    assert isinstance(ov, torch.Tensor) and ov.is_cuda                          # tensors in, tensors out
    _assert_same((ov.cpu().numpy(), oc.cpu().numpy(), of.cpu().numpy(), rep), want)
    for buf, guard, n in ((vb, 12345.0, v.size), (fb, 1 << 30, f.size), (cb, 201, c.size)):
        assert (buf[:G] == guard).all() and (buf[G + n:] == guard).all()
    assert vb[G:G + v.size].cpu().numpy().tobytes() == v.tobytes() and fb[G:G + f.size].cpu().numpy().tobytes() == f.tobytes()


def test_bad_arguments_return_their_codes_and_leave_the_buffers_alone():
    import torch
    from mvsnet_amd import _lib
    h = _lib.load()
    ptr = _lib.ptr
    v, f = MC.grid(4)
    M_, F_ = len(v), len(f)
    tv, tf = torch.as_tensor(v).cuda(), torch.as_tensor(f).cuda()
    o = [torch.full((16 * M_ + 16 * F_,), 77, dtype=torch.int32, device="cuda") for _ in range(6)]
    wsb = h.mvs_mesh_cluster_workspace_bytes(M_, F_)
    ws = torch.full((wsb,), 9, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr()
    nan = float("nan")
    keys = lambda **k: h.mvs_mesh_cluster_keys_f32(*[k.get(n, d) for n, d in (
        ("v", ptr(tv)), ("M", M_), ("f", ptr(tf)), ("F", F_), ("ox", 0.0), ("oy", 0.0), ("oz", 0.0), ("cell", 1.0), ("keys", ptr(o[0])),
        ("offsets", ptr(o[1])), ("ws", ptr(ws)), ("wsb", wsb))], st)
    assert keys(wsb=wsb - 1) == -3 and keys(M=-1) == -1 and keys(F=2 ** 31) == -2 and keys(cell=0.0) == -1 and keys(cell=nan) == -1
    assert keys(ox=float("inf")) == -1 and keys(keys=None) == -1 and keys(f=None) == -1 and keys(ws=None) == -1
    assert h.mvs_mesh_cluster_heads_i64(None, M_, ptr(o[0]), st) == -1 and h.mvs_mesh_cluster_heads_i64(ptr(o[1]), 2 ** 31, ptr(o[0]), st) == -2
    sums = lambda **k: h.mvs_mesh_cluster_sums_f32(*[k.get(n, d) for n, d in (
        ("sk", ptr(o[0])), ("order", ptr(o[1])), ("rank", ptr(o[2])), ("offsets", ptr(o[3])), ("colours", None), ("M", M_), ("ox", 0.0),
        ("oy", 0.0), ("oz", 0.0), ("cell", 1.0), ("vc", ptr(o[4])), ("cv", ptr(o[5])), ("cc", None), ("ws", ptr(ws)), ("wsb", wsb))], st)
    assert sums(wsb=wsb - 1) == -3 and sums(M=-1) == -1 and sums(M=2 ** 31) == -2 and sums(cell=-1.0) == -1 and sums(order=None) == -1
    assert sums(cc=ptr(o[5])) == -1                                             # colours out without colours in
    faces = lambda **k: h.mvs_mesh_cluster_faces_i32(*[k.get(n, d) for n, d in (
        ("f", ptr(tf)), ("M", M_), ("F", F_), ("vc", ptr(o[0])), ("cf", ptr(o[1])), ("lo", ptr(o[2])), ("hi", None), ("ws", ptr(ws)),
        ("wsb", wsb))], st)
    assert faces(wsb=wsb - 1) == -3 and faces(F=-1) == -1 and faces(lo=None) == -1 and faces(F=2 ** 31) == -2
    assert faces(M=2 ** 21 + 1, wsb=2 ** 40) == -2 and faces(M=2 ** 21 + 1, hi=ptr(o[3])) == -3      # one key only up to 2^21 vertices
    mark = lambda **k: h.mvs_mesh_cluster_mark_i32(*[k.get(n, d) for n, d in (
        ("cf", ptr(o[1])), ("M", M_), ("F", F_), ("lo", ptr(o[2])), ("hi", None), ("order", ptr(o[3])), ("fk", ptr(o[4])), ("vk", ptr(o[5])),
        ("ws", ptr(ws)), ("wsb", wsb))], st)
    assert mark(wsb=wsb - 1) == -3 and mark(M=-1) == -1 and mark(order=None) == -1 and mark(vk=None) == -1 and mark(M=2 ** 31) == -2
    assert h.mvs_mesh_cluster_workspace_bytes(-1, 0) == 0 and h.mvs_mesh_cluster_workspace_bytes(0, 2 ** 31) == 0
    torch.cuda.synchronize()
    assert all((x == 77).all() for x in o) and (ws == 9).all()
    assert tv.cpu().numpy().tobytes() == v.tobytes() and tf.cpu().numpy().tobytes() == f.tobytes()


def test_the_two_key_sort_of_the_faces_gives_the_one_key_bytes():
    from mvsnet_amd import mesh_simplify
    for kind, noisy, mult in (("sphere", True, 2), ("plane", False, 2), ("step", True, 1)):
        v, c, f = MC.scene_mesh(kind, noisy)
        f = f[np.random.RandomState(2).permutation(len(f))]
        cell = R.voxels(mult, M.SCENE_VOXEL)
        one = mesh_simplify.simplify_mesh(v, c, f, cell, SCENE_O, two_keys=False)
        two = _check(v, c, f, cell, SCENE_O, two_keys=True)
        _assert_same(one, two)
        assert mult == 1 or two[3]["duplicate_faces"] > 0


def test_two_runs_and_a_side_stream_give_the_same_bytes():
    import torch
    from mvsnet_amd import mesh_simplify
    v, c, f = MC.scene_mesh("sphere", True)
    f = f[np.random.RandomState(3).permutation(len(f))]
    cell = R.voxels(2, M.SCENE_VOXEL)
    runs = [mesh_simplify.simplify_mesh(v, c, f, cell, SCENE_O) for _ in range(2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(mesh_simplify.simplify_mesh(v, c, f, cell, SCENE_O))
    side.synchronize()
    for run in runs:
        _assert_same(run, runs[0])
    _assert_same(runs[0], R.simplify(v, c, f, cell, SCENE_O))


# ------------------------------------------------------------------------------------------------ mesh.py and the command lines

def _cell(mult, voxel):
    """float32(S voxel) with the volume's float32 voxel, as mesh.py forms it."""
    return np.float32(float(mult) * float(np.float32(voxel)))


def test_extract_with_simplify_after_clean():
    from mvsnet_amd import mesh_clean
    vol = _noisy_volume("sphere")
    plain = vol.extract()
    assert len(plain) == 3
    for got, want in zip(plain, MC.scene_mesh("sphere", True)):                # without the option: today's bytes
        assert got.tobytes() == want.tobytes()
    cell = _cell(2, M.SCENE_VOXEL)
    v, c, f, rep = vol.extract(simplify=cell)
    assert set(rep) == {"simplify"}
    _assert_same((v, c, f, rep["simplify"]), R.simplify(*plain, cell, SCENE_O))
    options = dict(min_faces=8)
    cleaned = mesh_clean.clean_mesh(*plain, **options)
    v, c, f, rep = vol.extract(clean=options, simplify=cell)
    assert {k: rep[k] for k in cleaned[3]} == cleaned[3]                       # the cleaning ran first and reports as before
    _assert_same((v, c, f, rep["simplify"]), R.simplify(*cleaned[:3], cell, SCENE_O))
    assert rep["simplify"]["faces_in"] == cleaned[3]["faces_out"] < len(plain[2])
    again = vol.extract(clean=options)
    assert "simplify" not in again[3] and again[2].tobytes() == cleaned[2].tobytes()
    with pytest.raises(ValueError):
        vol.extract(simplify=0.0)


def test_mesh_depth_maps_with_simplify_voxels():
    from mvsnet_amd import mesh
    sc = M.scene("plane", noisy=False)
    bounds = (np.array(M.SCENE_ORIGIN, np.float64), np.array(M.SCENE_ORIGIN, np.float64) + M.SCENE_VOXEL * (np.array(M.SCENE_DIMS) - 1))
    kw = dict(voxel=M.SCENE_VOXEL, bounds=bounds, num_consistent=0)
    raw = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], **kw)
    vol = mesh.TsdfVolume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, 4 * M.SCENE_VOXEL, colour=True)
    plain = vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"]).extract()
    for a, b in zip(raw, plain):                                               # without the option the mesh bytes equal extract()'s
        assert a.tobytes() == b.tobytes()
    off = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], simplify_voxels=0, **kw)
    for a, b in zip(off, plain):
        assert a.tobytes() == b.tobytes()
    v, c, f = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], simplify_voxels=2, **kw)
    want = R.simplify(*plain, _cell(2, M.SCENE_VOXEL), SCENE_O)
    assert v.tobytes() == want[0].tobytes() and c.tobytes() == want[1].tobytes() and f.tobytes() == want[2].tobytes()
    assert (len(v), len(f)) == (1008, 1886)
    dist = sc["surface_distance"](v) / M.SCENE_VOXEL
    assert dist.max() < 0.03
    with pytest.raises(ValueError):
        mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], simplify_voxels=-1, **kw)


def test_mesh_command_line_with_simplify_voxels(dense, tmp_path):
    from mvsnet_amd import mesh
    folder, raw = dense
    out, want = str(tmp_path / "small.ply"), str(tmp_path / "want.ply")
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", folder, *COMMON, "--out", out, "--simplify_voxels", "2.5",
                      "--min_component_faces", "8")
    assert code == 0, text
    cleaned = MC.clean(*raw, min_faces=8)
    ref = R.simplify(*cleaned[:3], _cell(2.5, 0.05), SCENE_O)
    rep = _json_line(text)
    assert rep["simplify"] == ref[3] and rep["vertices"] == len(ref[0]) and rep["faces"] == len(ref[2]) < len(raw[2]) / 4
    assert {k: rep[k] for k in cleaned[3]} == cleaned[3]
    mesh.write_mesh_ply(want, *ref[:3])
    assert open(out, "rb").read() == open(want, "rb").read()


def test_mesh_simplify_command_line_on_a_written_ply(dense, tmp_path):
    from mvsnet_amd import mesh
    folder, raw = dense
    plain, again, want = str(tmp_path / "plain.ply"), str(tmp_path / "again.ply"), str(tmp_path / "want.ply")
    mesh.write_mesh_ply(plain, *raw)
    code, text = _run("mvsnet_amd.mesh_simplify", "--mesh", plain, "--out", again, "--cell", "0.1", "--origin=-1.4:-1.2:2.9")
    assert code == 0, text
    ref = R.simplify(*raw, 0.1, SCENE_O)
    rep = _json_line(text)
    assert {k: rep[k] for k in ref[3]} == ref[3] and rep["out"] == again
    mesh.write_mesh_ply(want, *ref[:3])
    assert open(again, "rb").read() == open(want, "rb").read()
    code, text = _run("mvsnet_amd.mesh_simplify", "--mesh", plain, "--out", again, "--cell", "0.2")      # refused before any GPU work
    assert code != 0 and "--force" in text
    code, text = _run("mvsnet_amd.mesh_simplify", "--mesh", plain, "--out", again, "--cell", "0.2", "--force")     # the default origin
    assert code == 0, text
    ref = R.simplify(*raw, 0.2)
    assert _json_line(text)["faces_out"] == ref[3]["faces_out"]
    assert mesh.read_mesh_ply(again)[2].tobytes() == ref[2].tobytes()


def test_depthfusion_command_line_passes_the_option_through(dense):
    from mvsnet_amd import mesh
    folder, _ = dense
    code, text = _run("mvsnet_amd.depthfusion", "--dense_folder", folder, "--fusion", "hip", "--mesh", "--mesh_simplify_voxels", "2")
    assert code == 0, text
    rep = _json_line(text, "meshed: ")["simplify"]
    v2, c2, f2 = mesh.read_mesh_ply(_json_line(text, "meshed: ")["out"])
    assert len(f2) == rep["faces_out"] < rep["faces_in"] / 3 and len(v2) == rep["vertices_out"] and rep["cell"] > 0
    assert len(np.unique(f2)) == len(v2)                                       # no unreferenced vertex
