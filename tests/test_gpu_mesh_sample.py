"""GPU tests of the surface sampling of csrc/mesh_sample.hip through mvsnet_amd.mesh_sample, against
tests/mesh_sample_reference.py byte for byte: the six scene meshes and the analytic sphere at three spacings under every
combination of outputs, runs of faces that straddle workgroups and the LDS cap from both sides, no sample at all, sample and
face counts around a workgroup and a wave, invalid faces between guard words, reproducibility, refused arguments, the errors,
the wiring into evaluate, mesh and depthfusion, and the four command lines."""
import itertools
import json
import os

import numpy as np
import pytest

from tests import mesh_clean_reference as MC
from tests import mesh_reference as M
from tests import mesh_sample_reference as R
from tests import mesh_simplify_reference as MS
from tests.test_gpu_mesh_clean import COMMON, _json_line, _run, dense  # noqa: F401  (dense is a fixture)
from tests.test_mesh_sample_host import FACE, TRIANGLE, sphere_points

pytestmark = pytest.mark.gpu
OUTPUTS = [dict(colour=c, normals=n, face_index=i) for c, n, i in itertools.product([False, True], repeat=3)]
DEGENERATE = [0, 0, 1]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = int((np.ascontiguousarray(got).reshape(-1).view(np.uint8) != np.ascontiguousarray(want).reshape(-1).view(np.uint8)).sum())
    assert bad == 0, "%s: %d bytes differ" % (what, bad)


def _assert_same(got, want, colour=True, normals=True, face_index=True):
    out, stats = got
    print("samples %d (want %d); stats %s" % (len(out["xyz"]), len(want["xyz"]), json.dumps(stats)))
    assert stats == want["stats"]
    _same(out["xyz"], want["xyz"], "xyz")
    for key, asked in (("colours", colour and want["colours"] is not None), ("normals", normals), ("face_index", face_index)):
        if asked:
            _same(out[key], want[key], key)
        else:
            assert out[key] is None, key


def _check(vertices, colours, faces, density, seed=0, want=None, **kw):
    from mvsnet_amd import mesh_sample
    kw = dict(dict(normals=True, face_index=True), **kw)
    got = mesh_sample.sample_mesh(vertices, colours, faces, density, seed, **kw)
    want = want or R.sample(vertices, colours, faces, density, seed)
    _assert_same(got, want, colour=colours is not None, normals=kw["normals"], face_index=kw["face_index"])
    return got


# ------------------------------------------------------------------------------------------------ the project's meshes

@pytest.mark.parametrize("kind,noisy", MC.SCENES + [("analytic", False)])
def test_scene_meshes_equal_the_reference(kind, noisy):
    if kind == "analytic":
        (v, f), spacings = MS.sphere_mesh(), (0.1, 0.05, 0.02)
        c = np.random.RandomState(3).randint(0, 256, (len(v), 3)).astype(np.uint8)
    else:
        (v, c, f), spacings = MC.scene_mesh(kind, noisy), tuple(m * M.SCENE_VOXEL for m in (2.0, 1.0, 0.5))
    for spacing in spacings:
        want = R.sphere_sample(spacing, 0, True) if kind == "analytic" else R.scene_sample(kind, noisy, spacing)
        for o in OUTPUTS:
            _check(v, c if o["colour"] else None, f, R.density_of(spacing), want=want, normals=o["normals"], face_index=o["face_index"])
    if kind == "analytic":
        assert want["stats"]["samples"] == 19913
        _check(v, c, f, R.density_of(0.05), seed=2 ** 64 - 1)


# ------------------------------------------------------------------------------------------------ built meshes

def _tiny_big_tiny(tiny=4096, scale=1e-4):
    """`tiny` triangles of 1e-3 expected samples each, one triangle of 100 000 samples, `tiny` more: at density 200 000."""
    rs = np.random.RandomState(6)
    base = rs.rand(2 * tiny, 1, 3).astype(np.float32)
    small = (base + np.float32(scale) * TRIANGLE[None]).reshape(-1, 3)
    v = np.concatenate([small, TRIANGLE + np.float32(2)]).astype(np.float32)
    fs = np.arange(6 * tiny, dtype=np.int32).reshape(-1, 3)
    big = np.array([[6 * tiny, 6 * tiny + 1, 6 * tiny + 2]], np.int32)
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    return v, c, np.concatenate([fs[:tiny], big, fs[tiny:]]), 200000.0


@pytest.mark.parametrize("shuffled", [False, True])
def test_many_faces_without_a_sample_around_one_with_very_many(shuffled):
    """The first and the last workgroups' runs hold more faces than the LDS cap (the search stays in global memory), those in the
    middle one face."""
    v, c, f, density = _tiny_big_tiny()
    if shuffled:
        f = f[np.random.RandomState(1).permutation(len(f))]
    got = _check(v, c, f, density)
    counts = np.bincount(got[0]["face_index"], minlength=len(f))
    assert counts.max() == 100000 and got[1]["samples"] == 100000 + 8 and (np.sort(counts)[:-1] <= 1).all()
    _check(v, None, f, density, seed=9, normals=False)


@pytest.mark.parametrize("run", [1023, 1024, 1025, 2500])
def test_runs_of_faces_around_the_lds_cap(run):
    """255 faces of one sample, faces without area, then 300 faces of one sample: the first workgroup's run is `run` faces."""
    v = np.concatenate([TRIANGLE, TRIANGLE + np.float32(1)])
    f = np.array([[0, 1, 2]] * 255 + [DEGENERATE] * (run - 256) + [[3, 4, 5]] * 300, np.int32)
    got = _check(v, None, f, 2.0)
    assert got[1]["samples"] == 555 and got[1]["zero_area"] == run - 256
    assert got[0]["face_index"][255] == run - 1


def test_no_sample_at_all():
    v, c, f = MC.scene_mesh("plane", False)
    got = _check(v, c, f, R.density_of(4.0))                                   # 6.26 units of area at one sample per 16
    assert got[1]["samples"] == 0 and got[0]["xyz"].shape == (0, 3) and got[0]["colours"].shape == (0, 3)
    assert 6.2637 - len(f) / 65536.0 * 16.0 < got[1]["area"] < 6.2637           # every face's quota lost less than 2^-16 of a sample


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_sample_counts_around_a_workgroup(N):
    got = _check(TRIANGLE, None, FACE, 2.0 * N)                                # half a unit of area: exactly N
    assert got[1]["samples"] == N
    v, f = MC.grid(3)
    got = _check(v, None, f, 1.7 * N)                                          # 18 faces that share about as many
    assert N // 2 < got[1]["samples"] < 2 * N + 2


@pytest.mark.parametrize("n_faces", [0, 1, 63, 64, 65])
def test_face_counts_around_a_wave(n_faces):
    v, f = MC.grid(8)
    c = np.arange(3 * len(v), dtype=np.uint8).reshape(-1, 3)
    for n_vertices in (len(v), 40, 0):                                         # faces beyond the vertices are invalid
        _check(v[:n_vertices], c[:n_vertices], f[:n_faces], 700.0)
        _check(v[:n_vertices], None, f[::2][:n_faces], 3.0)


# ------------------------------------------------------------------------------------------------ invalid faces, guards, errors

def test_invalid_faces_and_vertices_between_guard_words():
    """The arrays sit inside larger device buffers filled with a guard value: a face that names no vertex is never dereferenced,
    and nothing beside the outputs is written."""
    import torch
    from mvsnet_amd import mesh_sample
    rs = np.random.RandomState(8)
    v, f = (a.copy() for a in MC.grid(12))
    c = rs.randint(0, 256, (len(v), 3)).astype(np.uint8)
    f[5], f[17], f[40], f[99], f[100] = [-1, 0, 1], [0, 1, len(v)], [3, 2 ** 31 - 1, 4], [-2 ** 31, 7, 8], [9, 9, 10]
    v[20, 1], v[77, 0], v[100, 2] = np.nan, np.inf, -np.inf
    want = R.sample(v, c, f, 900.0, 5)
    assert want["stats"]["invalid"] > 4 and want["stats"]["zero_area"] == 1 and want["stats"]["samples"] > 1000
    G = 64
    vb = torch.full((G + v.size + G,), 12345.0, dtype=torch.float32, device="cuda")
    fb = torch.full((G + f.size + G,), 1 << 30, dtype=torch.int32, device="cuda")
    cb = torch.full((G + c.size + G,), 201, dtype=torch.uint8, device="cuda")
    vb[G:G + v.size], fb[G:G + f.size], cb[G:G + c.size] = (torch.as_tensor(a.reshape(-1)).cuda() for a in (v, f, c))
    tv, tf, tc = vb[G:G + v.size].view(-1, 3), fb[G:G + f.size].view(-1, 3), cb[G:G + c.size].view(-1, 3)
    out, stats = mesh_sample.sample_mesh(tv, tc, tf, 900.0, 5, normals=True, face_index=True)
    assert isinstance(out["xyz"], torch.Tensor) and out["xyz"].is_cuda          # tensors in, tensors out
    _assert_same(({k: t.cpu().numpy() for k, t in out.items()}, stats), want)
    assert np.isfinite(out["xyz"].cpu().numpy()).all()
    for buf, guard, n in ((vb, 12345.0, v.size), (fb, 1 << 30, f.size), (cb, 201, c.size)):
        assert (buf[:G] == guard).all() and (buf[G + n:] == guard).all()
    assert vb[G:G + v.size].cpu().numpy().tobytes() == v.tobytes() and fb[G:G + f.size].cpu().numpy().tobytes() == f.tobytes()


def test_sums_that_are_not_the_scan_of_the_quota_stay_inside_the_arrays():
    """The write call with sums the caller made up: decreasing, huge, negative.  Every sample is either a point of a face with
    indices inside the mesh or zeros with face -1."""
    import torch
    from mvsnet_amd import _lib
    h = _lib.load()
    v, f = MC.grid(6)
    f = f.copy()
    f[7] = [0, 1, len(v)]
    tv, tf = torch.as_tensor(v).cuda(), torch.as_tensor(f).cuda()
    N = 700
    rs = np.random.RandomState(2)
    for sums in (np.arange(len(f), 0, -1) * 10 << 16, np.full(len(f), 2 ** 62), np.full(len(f), -5), rs.randint(-2 ** 40, 2 ** 40, len(f)),
                 np.arange(1, len(f) + 1) * 5 << 16):
        ts = torch.as_tensor(np.asarray(sums, np.int64)).cuda()
        xyz = torch.full((N + 8, 3), 7.0, device="cuda")
        face = torch.full((N + 8,), 77, dtype=torch.int32, device="cuda")
        rc = h.mvs_mesh_sample_write_f32(_lib.ptr(tv), None, len(v), _lib.ptr(tf), len(f), _lib.ptr(ts), N, 3, _lib.ptr(xyz), _lib.ptr(face),
                                         None, None, _lib.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        fi, p = face.cpu().numpy(), xyz.cpu().numpy()
        assert (fi[N:] == 77).all() and (p[N:] == 7).all()
        assert ((fi[:N] >= -1) & (fi[:N] < len(f)) & (fi[:N] != 7)).all()
        assert (p[:N][fi[:N] < 0] == 0).all() and np.isfinite(p).all()
        inside = fi[:N] >= 0
        assert (p[:N][inside] >= v.min(0)).all() and (p[:N][inside] <= v.max(0)).all()


def test_bad_arguments_return_their_codes_and_leave_the_buffers_alone():
    import torch
    from mvsnet_amd import _lib
    h = _lib.load()
    ptr = _lib.ptr
    v, f = MC.grid(4)
    M_, F_ = len(v), len(f)
    tv, tf = torch.as_tensor(v).cuda(), torch.as_tensor(f).cuda()
    tc = torch.zeros((M_, 3), dtype=torch.uint8, device="cuda")
    o = [torch.full((16 * M_ + 16 * F_,), 77, dtype=torch.int32, device="cuda") for _ in range(5)]
    wsb = h.mvs_mesh_sample_workspace_bytes(M_, F_)
    ws = torch.full((wsb,), 9, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr()
    quota = lambda **k: h.mvs_mesh_sample_quota_f32(*[k.get(n, d) for n, d in (
        ("v", ptr(tv)), ("M", M_), ("f", ptr(tf)), ("F", F_), ("d", 1.0), ("q", ptr(o[0])), ("ws", ptr(ws)), ("wsb", wsb))], st)
    assert quota(wsb=wsb - 1) == -3 and quota(M=-1) == -1 and quota(F=-1) == -1 and quota(F=2 ** 26 + 1) == -2 and quota(M=2 ** 31) == -2
    assert quota(d=0.0) == -1 and quota(d=float("nan")) == -1 and quota(d=float("inf")) == -1 and quota(d=-2.0) == -1
    assert quota(v=None) == -1 and quota(f=None) == -1 and quota(q=None) == -1 and quota(ws=None) == -1
    write = lambda **k: h.mvs_mesh_sample_write_f32(*[k.get(n, d) for n, d in (
        ("v", ptr(tv)), ("c", None), ("M", M_), ("f", ptr(tf)), ("F", F_), ("s", ptr(o[0])), ("N", 10), ("seed", 0), ("xyz", ptr(o[1])),
        ("face", ptr(o[2])), ("rgb", None), ("nrm", ptr(o[4])))], st)
    assert write(N=-1) == -1 and write(N=2 ** 31) == -2 and write(M=-1) == -1 and write(F=2 ** 26 + 1) == -2 and write(M=0) == -1 and write(F=0) == -1
    assert write(v=None) == -1 and write(f=None) == -1 and write(s=None) == -1 and write(xyz=None) == -1
    assert write(rgb=ptr(o[3])) == -1 and write(N=0, c=ptr(tc), rgb=ptr(o[3])) == 0       # colours out without colours in; nothing to write
    assert h.mvs_mesh_sample_workspace_bytes(-1, 0) == 0 and h.mvs_mesh_sample_workspace_bytes(0, 2 ** 26 + 1) == 0
    torch.cuda.synchronize()
    assert all((x == 77).all() for x in o) and (ws == 9).all()
    assert tv.cpu().numpy().tobytes() == v.tobytes() and tf.cpu().numpy().tobytes() == f.tobytes()


def test_a_saturated_face_and_too_many_samples_raise():
    from mvsnet_amd import mesh_sample
    big = TRIANGLE * np.float32(2048)
    with pytest.raises(ValueError, match="1 faces expect"):
        mesh_sample.sample_mesh(big, None, FACE, 1.0)
    with pytest.raises(ValueError, match="1 faces expect"):
        mesh_sample.sample_mesh(TRIANGLE, None, FACE, 1e300)
    with pytest.raises(ValueError, match="max_samples = 4"):
        mesh_sample.sample_mesh(TRIANGLE, None, FACE, 10, max_samples=4)
    assert mesh_sample.sample_mesh(TRIANGLE, None, FACE, 10, max_samples=5)[1]["samples"] == 5
    v, _, f = MC.scene_mesh("step", False)
    with pytest.raises(ValueError, match="max_samples"):
        mesh_sample.sample_mesh(v, None, f, 1e8)                               # 6.6e8 samples: refused before anything is allocated
    assert mesh_sample.sample_mesh(big, None, FACE, 0.49)[1]["samples"] == int(0.49 * 2 ** 21)


def test_two_runs_and_a_side_stream_give_the_same_bytes():
    import torch
    from mvsnet_amd import mesh_sample
    v, c, f = MC.scene_mesh("sphere", True)
    f = f[np.random.RandomState(3).permutation(len(f))]
    d = R.density_of(0.02)
    runs = [mesh_sample.sample_mesh(v, c, f, d, 11, normals=True, face_index=True) for _ in range(2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(mesh_sample.sample_mesh(v, c, f, d, 11, normals=True, face_index=True))
    side.synchronize()
    want = R.sample(v, c, f, d, 11)
    for run in runs:
        _assert_same(run, want)


# ------------------------------------------------------------------------------------------------ evaluate, mesh.py, depthfusion.py

def _without_sampling(metrics):
    return {k: x for k, x in metrics.items() if not k.endswith("_sampling")}


def test_evaluating_a_mesh_equals_evaluating_its_samples():
    from mvsnet_amd import evaluate, mesh_sample
    v, _, f = MC.scene_mesh("sphere", False)
    gv, _, gf = MC.scene_mesh("sphere", True)
    kw = dict(max_dist=0.5, thresholds=[0.02, 0.1], crop=[-1, -1, 3, 1, 1, 6], voxel_pred=0.03)
    cloud, stats = mesh_sample.sample_mesh(v, None, f, R.density_of(0.04))
    want = evaluate.evaluate_point_clouds(cloud["xyz"], gv, **kw)
    got = evaluate.evaluate_point_clouds(v, gv, pred_faces=f, pred_spacing=0.04, **kw)
    assert got["pred_sampling"] == dict(stats, spacing=0.04) and "gt_sampling" not in got
    assert _without_sampling(got) == want and got["pred_points"] == stats["samples"] > got["pred_points_used"]
    gcloud, gstats = mesh_sample.sample_mesh(gv, None, gf, R.density_of(0.05))
    want = evaluate.evaluate_point_clouds(cloud["xyz"], gcloud["xyz"], **kw)
    got = evaluate.evaluate_point_clouds(v, gv, pred_faces=f, pred_spacing=0.04, gt_faces=gf, gt_spacing=0.05, **kw)
    assert got["gt_sampling"] == dict(gstats, spacing=0.05) and _without_sampling(got) == want
    plain = evaluate.evaluate_point_clouds(v, gv, **kw)                         # without the options: today's report
    assert "pred_sampling" not in plain and "gt_sampling" not in plain and plain["pred_points"] == len(v)


def test_samples_score_a_simplified_sphere_that_its_vertices_do_not():
    from mvsnet_amd import evaluate
    gt = sphere_points()
    ov, _, of, _ = MS.sphere_simplify(2)
    kw = dict(max_dist=1.0, thresholds=[0.05])
    sampled = evaluate.evaluate_point_clouds(ov, gt, pred_faces=of, pred_spacing=0.02, **kw)
    vertices = evaluate.evaluate_point_clouds(ov, gt, **kw)
    print("completeness at 0.05: %.3f from %d vertices, %.3f from %d samples" % (vertices["recall"][0], len(ov), sampled["recall"][0],
                                                                                 sampled["pred_points"]))
    assert sampled["recall"][0] == 1.0 and vertices["recall"][0] < 0.35
    assert sampled["pred_points"] == R.sample(ov, None, of, R.density_of(0.02))["stats"]["samples"]


@pytest.fixture(scope="module")
def gt_ply(dense, tmp_path_factory):
    """A ground-truth cloud for the dense folder's scene: the vertices of its mesh, as a point PLY."""
    from mvsnet_amd import fusion
    path = str(tmp_path_factory.mktemp("gt") / "gt.ply")
    fusion.write_ply(path, dense[1][0], dense[1][1])
    return path


def test_mesh_dense_folder_and_hip_fusion_write_mesh_metrics(dense, gt_ply, tmp_path):
    from mvsnet_amd import depthfusion, evaluate, mesh
    folder, raw = dense
    kw = dict(voxel=0.05, num_consistent=0, bounds=mesh.parse_bounds(COMMON[-1].split("=")[1]), simplify_voxels=2)
    plain, scored = str(tmp_path / "a" / "mesh.ply"), str(tmp_path / "b" / "mesh.ply")
    rep = mesh.mesh_dense_folder(folder, plain, **kw)
    assert "mesh_metrics" not in rep and os.listdir(str(tmp_path / "a")) == ["mesh.ply"]
    rep = mesh.mesh_dense_folder(folder, scored, eval_gt=gt_ply, eval_spacing=0.03, eval_max_dist=1.0, eval_thresholds=[0.05], **kw)
    assert open(plain, "rb").read() == open(scored, "rb").read()
    assert rep["mesh_metrics"] == str(tmp_path / "b" / "mesh_metrics.json")
    got = json.load(open(rep["mesh_metrics"]))
    v, _, f = mesh.read_mesh_ply(scored)
    want = evaluate.evaluate_point_clouds(v, raw[0], max_dist=1.0, thresholds=[0.05], pred_faces=f, pred_spacing=0.03)
    assert got == json.loads(json.dumps(want)) and got["pred_sampling"]["samples"] > 5000 and 0 < got["recall"][0] <= 1
    common = dict(dedupe=True, eval_gt=gt_ply, eval_max_dist=1.0, eval_thresholds=[0.05], mesh=True, mesh_simplify_voxels=2)
    one = depthfusion.hip_fusion(folder, str(tmp_path / "p1"), 0.8, 1.0, 0.01, 3, **common)
    two = depthfusion.hip_fusion(folder, str(tmp_path / "p2"), 0.8, 1.0, 0.01, 3, mesh_eval_spacing=0.03, **common)
    d1, d2 = os.path.dirname(one), os.path.dirname(two)
    assert sorted(os.listdir(d1)) == ["final3d_model.ply", "mesh.ply", "metrics.json"]
    assert sorted(os.listdir(d2)) == ["final3d_model.ply", "mesh.ply", "mesh_metrics.json", "metrics.json"]
    for name in ("final3d_model.ply", "mesh.ply", "metrics.json"):
        assert open(os.path.join(d1, name), "rb").read() == open(os.path.join(d2, name), "rb").read(), name
    assert json.load(open(os.path.join(d2, "mesh_metrics.json")))["pred_sampling"]["spacing"] == 0.03


def test_the_four_command_lines(dense, gt_ply, tmp_path):
    from mvsnet_amd import fusion, mesh
    folder, raw = dense
    src, cloud = str(tmp_path / "mesh.ply"), str(tmp_path / "cloud.ply")
    mesh.write_mesh_ply(src, *raw)
    code, text = _run("mvsnet_amd.mesh_sample", "--mesh", src, "--out", cloud, "--spacing", "0.03", "--seed", "4", "--normals")
    assert code == 0, text
    want = R.sample(*raw, R.density_of(0.03), 4)
    rep = _json_line(text)
    assert {k: rep[k] for k in want["stats"]} == want["stats"] and rep["out"] == cloud and rep["seed"] == 4
    xyz, rgb, nrm = fusion.read_ply_normals(cloud)
    assert xyz.tobytes() == want["xyz"].tobytes() and rgb.tobytes() == want["colours"].tobytes() and nrm.tobytes() == want["normals"].tobytes()
    code, text = _run("mvsnet_amd.mesh_sample", "--mesh", src, "--out", cloud, "--spacing", "0.03")          # refused before any GPU work
    assert code != 0 and "--force" in text

    code, text = _run("mvsnet_amd.evaluate", "--pred", src, "--gt", gt_ply, "--max_dist", "1", "--thresholds", "0.05", "--pred_spacing", "0.03",
                      "--out", str(tmp_path / "m.json"))
    assert code == 0, text
    rep = _json_line(text)
    assert rep["pred_sampling"]["samples"] == R.sample(raw[0], None, raw[2], R.density_of(0.03))["stats"]["samples"] == rep["pred_points"]
    assert rep["recall"][0] > 0.9 and json.load(open(str(tmp_path / "m.json"))) == rep

    out = str(tmp_path / "made" / "mesh.ply")
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", folder, *COMMON, "--out", out, "--eval_gt", gt_ply, "--eval_spacing", "0.03",
                      "--eval_max_dist", "1", "--eval_thresholds", "0.05")
    assert code == 0, text
    assert _json_line(text)["mesh_metrics"] == str(tmp_path / "made" / "mesh_metrics.json")
    assert json.load(open(str(tmp_path / "made" / "mesh_metrics.json")))["pred_sampling"] == rep["pred_sampling"]
    want_ply = str(tmp_path / "want.ply")
    mesh.write_mesh_ply(want_ply, *raw)
    assert open(out, "rb").read() == open(want_ply, "rb").read()

    code, text = _run("mvsnet_amd.depthfusion", "--dense_folder", folder, "--fusion", "hip", "--mesh", "--eval_gt", gt_ply, "--eval_max_dist", "1",
                      "--eval_thresholds", "0.05", "--mesh_eval_spacing", "0.03")
    assert code == 0, text
    made = os.path.dirname(_json_line(text, "meshed: ")["out"])
    assert sorted(os.listdir(made)) == ["final3d_model.ply", "mesh.ply", "mesh_metrics.json", "metrics.json"]
    assert "pred_sampling" in json.load(open(os.path.join(made, "mesh_metrics.json")))
    assert "pred_sampling" not in json.load(open(os.path.join(made, "metrics.json")))
