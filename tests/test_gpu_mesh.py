"""GPU tests of the TSDF fusion and the surface-nets extraction (csrc/tsdf.hip through mvsnet_amd.mesh) against the float32
restatement of tests/mesh_reference.py, byte for byte: integration on the three scenes and on volumes of awkward sizes, with
and without images, in one call and in two, with views that see nothing and pixels that count
for nothing; extraction of the analytic sphere and the scenes; reproducibility; the consistency masks; argument checks; and
the command lines end to end."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_reference as F
from tests import mesh_reference as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["plane", "sphere", "step"]
SMALL_DIMS = [(5, 4, 3), (64, 3, 3), (65, 9, 7), (1, 7, 7)]


def _origin(dims):
    """The standard volume's origin, or for a small volume one that puts the plane Z = 4 between its z-slices."""
    if dims == M.SCENE_DIMS:
        return M.SCENE_ORIGIN
    return (-0.5 * (dims[0] - 1) * M.SCENE_VOXEL + 0.004, -0.5 * (dims[1] - 1) * M.SCENE_VOXEL - 0.003,
            4.0 - 0.5 * (dims[2] - 1) * M.SCENE_VOXEL - 0.013)


@functools.lru_cache(maxsize=None)
def _reference(kind, colour, dims=M.SCENE_DIMS):
    """The float32 statement's volume; shared, never modified."""
    if dims == M.SCENE_DIMS:
        return M.scene_volume(kind, colour)
    sc = M.scene(kind)
    vol = M.new_volume(_origin(dims), M.SCENE_VOXEL, dims, M.SCENE_TRUNC, colour=colour)
    return M.integrate(vol, sc["depths"], sc["probs"], sc["cams"], sc["images"] if colour else None)


def _volume(dims=M.SCENE_DIMS, colour=False, origin=None, voxel=M.SCENE_VOXEL, trunc=M.SCENE_TRUNC):
    from mvsnet_amd import mesh
    return mesh.TsdfVolume(_origin(dims) if origin is None else origin, voxel, dims, trunc, colour=colour)


def _assert_state(vol, want):
    got = vol.state()
    keys = ["sum", "count"] + (["rgb_sum", "rgb_count"] if want["rgb_sum"] is not None else [])
    diff = {k: int((np.ascontiguousarray(got[k]).view(np.uint32) != np.ascontiguousarray(want[k]).view(np.uint32)).sum()) for k in keys}
    print("nodes that differ:", diff, "of", want["count"].size, "observed", int((want["count"] > 0).sum()))
    assert got["sum"].dtype == np.float32 and got["count"].dtype == np.int32 and got["sum"].shape == want["sum"].shape
    assert all(v == 0 for v in diff.values())


def _load(vol, ref):
    """Puts a reference volume's sums on the device."""
    import torch
    vol.sum.copy_(torch.as_tensor(ref["sum"]))
    vol.count.copy_(torch.as_tensor(ref["count"]))
    if ref["rgb_sum"] is not None:
        vol.rgb_sum.copy_(torch.as_tensor(ref["rgb_sum"].view(np.int32)))
        vol.rgb_count.copy_(torch.as_tensor(ref["rgb_count"]))
    return vol


def _assert_mesh(got, want):
    v, c, f = got
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    print("vertices %d (want %d), faces %d (want %d)" % (len(v), len(want["vertices"]), len(f), len(want["faces"])))
    assert v.shape == want["vertices"].shape and f.shape == want["faces"].shape and c.shape == want["colours"].shape
    nv = int((v.view(np.uint32) != want["vertices"].view(np.uint32)).sum())
    nc, nf = int((c != want["colours"]).sum()), int((f != want["faces"]).sum())
    print("values that differ: vertices %d, colours %d, faces %d" % (nv, nc, nf))
    assert nv == 0 and nc == 0 and nf == 0


# ------------------------------------------------------------------------------------------------ integration

@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_integration_of_a_scene_equals_the_float32_reference(kind, colour):
    sc = M.scene(kind)
    vol = _volume(colour=colour)
    vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"] if colour else None)
    want = _reference(kind, colour)
    assert int((want["count"] > 0).sum()) > 50000
    _assert_state(vol, want)


@pytest.mark.parametrize("dims", SMALL_DIMS)
def test_integration_into_volumes_of_awkward_sizes(dims):
    sc = M.scene("plane")
    vol = _volume(dims, colour=True)
    vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"])
    want = _reference("plane", True, dims)
    assert (want["sum"] < 0).any() and (want["sum"] > 0).any()                 # the surface passes through the volume
    _assert_state(vol, want)


def test_two_calls_equal_one_call():
    sc = M.scene("sphere")
    vol = _volume(colour=True)
    vol.integrate(sc["depths"][:3], sc["probs"][:3], sc["cams"][:3], sc["images"][:3])
    vol.integrate(sc["depths"][3:], sc["probs"][3:], sc["cams"][3:], sc["images"][3:])
    _assert_state(vol, _reference("sphere", True))


@functools.lru_cache(maxsize=None)
def _blind_views():
    """The sphere scene plus a camera behind which the whole volume lies and one that looks away from it, between the
    scene's views: seven views of which two add nothing."""
    sc = M.scene("sphere")
    behind, away = np.array(sc["cams"][0]), np.array(sc["cams"][0])
    behind[0, :3, :3], behind[0, :3, 3] = np.eye(3), -np.array([0.0, 0.0, 9.0])          # at Z = 9 looking along +Z
    R = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])                                   # at the origin looking along +X
    away[0, :3, :3], away[0, :3, 3] = R, 0.0
    order = [0, 1, 5, 2, 3, 6, 4]
    cams = np.concatenate([sc["cams"], behind[None], away[None]])[order]
    pick = lambda a: np.concatenate([a, a[:2]])[order]
    return pick(sc["depths"]), pick(sc["probs"]), cams, pick(sc["images"])


def test_views_that_see_nothing_of_the_volume_add_nothing():
    depths, probs, cams, images = _blind_views()
    want = M.integrate(M.new_volume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, M.SCENE_TRUNC, colour=True), depths, probs, cams,
                       images)
    vol = _volume(colour=True)
    vol.integrate(depths, probs, cams, images)
    five = _reference("sphere", True)
    assert np.array_equal(want["sum"], five["sum"]) and np.array_equal(want["count"], five["count"])
    _assert_state(vol, five)


@functools.lru_cache(maxsize=None)
def _spoilt():
    """The step scene with pixels that count for nothing: NaN, inf, negative and zero depths and low probabilities."""
    sc = M.scene("step")
    rs = np.random.RandomState(11)
    depths, probs = sc["depths"].copy(), sc["probs"].copy()
    what = rs.randint(0, 12, depths.shape)
    for code, value in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, -3.5), (4, 0.0)):
        depths[what == code] = value
    probs[what == 5] = 0.79
    probs[what == 6] = np.nan
    want = M.integrate(M.new_volume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, M.SCENE_TRUNC, colour=True), depths, probs,
                       sc["cams"], sc["images"])
    return depths, probs, sc["cams"], sc["images"], want


def test_pixels_that_are_not_finite_negative_or_improbable_count_for_nothing():
    depths, probs, cams, images, want = _spoilt()
    clean = _reference("step", True)
    assert 0 < int(want["count"].sum()) < int(clean["count"].sum())
    vol = _volume(colour=True)
    vol.integrate(depths, probs, cams, images)
    _assert_state(vol, want)
    # the threshold is the caller's: at 0.75 the pixels of probability 0.79 count again
    want75 = M.integrate(M.new_volume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, M.SCENE_TRUNC), depths, probs, cams,
                         prob_threshold=0.75)
    assert int(want75["count"].sum()) > int(want["count"].sum())
    vol = _volume()
    vol.integrate(depths, probs, cams, prob_threshold=0.75)
    _assert_state(vol, want75)


def test_two_runs_give_the_same_bytes():
    sc = M.scene("sphere")
    runs = []
    for _ in range(2):
        vol = _volume(colour=True)
        vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"])
        state = vol.state()
        runs.append([state[k] for k in ("sum", "count", "rgb_sum", "rgb_count")] + list(vol.extract()))
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ extraction

@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_extraction_of_a_scene_equals_the_float32_reference(kind, min_count):
    ref = _reference(kind, True)
    want = M.extract(ref, min_count)
    assert len(want["faces"]) > 3000
    _assert_mesh(_load(_volume(colour=True), ref).extract(min_count), want)


def test_extraction_of_the_analytic_sphere():
    ref = M.analytic_sphere()
    vol = _volume(M.SPHERE_DIMS, origin=M.SPHERE_ORIGIN, voxel=M.SPHERE_VOXEL, trunc=4 * M.SPHERE_VOXEL)
    got = _load(vol, ref).extract()
    assert len(got[0]) == 1212 and len(got[2]) == 2420 and (got[1] == 0).all()
    _assert_mesh(got, M.extract(ref))


@pytest.mark.parametrize("dims", SMALL_DIMS)
def test_extraction_from_volumes_of_awkward_sizes(dims):
    ref = _reference("plane", True, dims)
    want = M.extract(ref)
    assert (len(want["vertices"]) > 0) == (min(dims) > 1)
    _assert_mesh(_load(_volume(dims, colour=True), ref).extract(), want)


def test_a_volume_without_a_surface_gives_an_empty_mesh():
    vol = _volume((20, 9, 6))
    v, c, f = vol.extract()                                                    # nothing observed
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    vol.sum.fill_(0.5), vol.count.fill_(2)                                     # observed and outside everywhere
    v, c, f = vol.extract()
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    vol.sum.fill_(-0.5)                                                        # inside everywhere: no sign change either
    assert [len(a) for a in vol.extract()] == [0, 0, 0]
    assert [len(a) for a in vol.extract(min_count=3)] == [0, 0, 0]
    f32, cnt = vol.tsdf()
    assert (f32 == -0.25).all() and (cnt == 2).all()


def test_scene_to_mesh_end_to_end_equals_the_reference():
    sc = M.scene("sphere")
    vol = _volume(colour=True)
    vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"])
    _assert_mesh(vol.extract(), M.scene_mesh("sphere", colour=True))


# ------------------------------------------------------------------------------------------------ the whole chain of stages

CHAIN = ("clean", "smooth", "simplify", "recolour")                           # mesh.STAGES' order
SUBSETS = [tuple(n for k, n in enumerate(CHAIN) if bits >> k & 1) for bits in range(16)]


@functools.lru_cache(maxsize=None)
def _chain_scene():
    """The noisy sphere, integrated once -> (volume, its plain extraction, extract's value per stage)."""
    from mvsnet_amd import mesh_colour
    from tests.test_gpu_mesh_clean import _noisy_volume
    sc = M.scene("sphere", noisy=True)
    vol = _noisy_volume("sphere")
    voxel = float(np.float32(M.SCENE_VOXEL))
    cams = mesh_colour.scale_cams(sc["cams"], sc["depths"].shape[1:3], sc["images"].shape[1:3])
    values = dict(clean=dict(min_faces=8), smooth=dict(iterations=3, lam=0.5, mu=-0.53, boundary="fixed", max_displacement=voxel),
                  simplify=float(np.float32(2 * voxel)), recolour=dict(cams=cams, images=sc["images"]))
    return vol, vol.extract(), values


@functools.lru_cache(maxsize=None)
def _composed(names):
    """The public functions of the stages in `names`, one after the other on the plain extraction -> (vertices, colours, faces,
    {stage: its report}); every chain is computed once and is the start of the longer ones."""
    from mvsnet_amd import mesh_clean, mesh_colour, mesh_simplify, mesh_smooth
    vol, plain, values = _chain_scene()
    if not names:
        return plain + ({},)
    v, c, f, reports = _composed(names[:-1])
    value = values[names[-1]]
    if names[-1] == "clean":
        v, c, f, rep = mesh_clean.clean_mesh(v, c, f, **value)
    elif names[-1] == "smooth":
        v, c, f, rep = mesh_smooth.smooth_mesh(v, c, f, **value)
    elif names[-1] == "simplify":
        v, c, f, rep = mesh_simplify.simplify_mesh(v, c, f, value, vol.origin)
    else:
        v, c, f, rep = mesh_colour.colour_mesh(v, c, f, value["cams"], value["images"])
    return v, c, f, dict(reports, **{names[-1]: rep})


@pytest.mark.parametrize("names", SUBSETS, ids=["+".join(s) or "none" for s in SUBSETS])
def test_extract_with_any_subset_of_the_stages_equals_their_public_functions_in_order(names):
    vol, plain, values = _chain_scene()
    got = vol.extract(**{n: values[n] for n in names})
    v, c, f, reports = _composed(names)
    assert len(got) == (4 if names else 3)
    for a, b, what in zip(got, (v, c, f), ("vertices", "colours", "faces")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (names, what)
    if names:
        clean = reports.get("clean", {})
        assert set(got[3]) == set(clean) | (set(names) - {"clean"})                # clean's fields at top level, the others by name
        assert {k: got[3][k] for k in clean} == clean
        for n in names:
            assert n == "clean" or got[3][n] == reports[n], n
    assert len(got[0]) > 0 and len(got[2]) > 0 and (got[0].tobytes() != plain[0].tobytes()) == (names not in ((), ("recolour",)))


# ------------------------------------------------------------------------------------------------ masks, arguments, commands

@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_consistency_masks_equal_the_reference_masks(kind):
    from mvsnet_amd import mesh
    sc = M.scene(kind, noisy=True)
    ref = F.reference_fusion(sc["depths"], sc["probs"], sc["cams"], num_consistent=3, dedupe=False)
    got = mesh.consistency_masks(sc["depths"], sc["probs"], sc["cams"], num_consistent=3)
    assert got.dtype == bool and got.shape == ref["keep"].shape
    # the project's rule for its float32 fusion against the float64 statement (tests/test_gpu_fusion.py): equal wherever the
    # reference's own margin to a decision boundary is clear of float32 error
    clear = ref["margin"] > 1e-4
    print(kind, "kept %d, differ %d, margin not clear at %d" % (int(ref["keep"].sum()), int((got != ref["keep"]).sum()), int((~clear).sum())))
    assert clear.mean() > 0.99 and np.array_equal(got[clear], ref["keep"][clear])


def test_bad_arguments_return_their_codes_and_leave_the_buffers_alone():
    import torch
    from mvsnet_amd import _lib
    h = _lib.load()
    sc = M.scene("plane")
    vol = _volume((9, 8, 7), colour=True)
    vol.sum.fill_(0.25), vol.count.fill_(3), vol.rgb_sum.fill_(7), vol.rgb_count.fill_(1)
    d, p = torch.as_tensor(sc["depths"]).cuda(), torch.as_tensor(sc["probs"]).cuda()
    proj = torch.zeros(60, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    o = (ctypes.c_float * 3)(0, 0, 0)
    ptr = _lib.ptr

    def integ(V=5, voxel=0.05, nx=9, trunc=0.2, flags=0, wsb=ws.numel(), depth=d):
        return h.mvs_tsdf_integrate_f32(ptr(depth), ptr(p), V, 40, 48, ptr(proj), None, 0, 0, o, voxel, nx, 8, 7, trunc, 0.8, flags,
                                        ptr(vol.sum), ptr(vol.count), None, None, ptr(ws), wsb, _lib.stream_ptr())

    assert integ(V=0) == -1 and integ(voxel=-1.0) == -1 and integ(trunc=0.0) == -1 and integ(flags=1) == -1 and integ(depth=None) == -1
    assert integ(nx=1 << 30) == -2 and integ(wsb=1024) == -3
    tot = torch.full((2,), 99, dtype=torch.int32, device="cuda")
    assert h.mvs_surface_nets_count_f32(ptr(vol.sum), ptr(vol.count), 9, 8, 7, 0, ptr(tot), ptr(ws), ws.numel(), None) == -1
    assert h.mvs_surface_nets_count_f32(ptr(vol.sum), ptr(vol.count), 9, 8, 7, 1, ptr(tot), ptr(ws), 16, None) == -3
    out = torch.full((64,), 5, dtype=torch.int32, device="cuda")
    assert h.mvs_surface_nets_write_f32(ptr(vol.sum), ptr(vol.count), None, None, o, 0.05, 9, 8, 7, 1, ptr(out), ptr(out), -1, 0,
                                        ptr(out), ptr(out), ptr(out), ptr(ws), ws.numel(), None) == -1
    assert h.mvs_surface_nets_write_f32(ptr(vol.sum), ptr(vol.count), None, None, o, 0.05, 9, 8, 7, 1, ptr(out), ptr(out), 1, 1,
                                        ptr(out), ptr(out), ptr(out), ptr(ws), 16, None) == -3
    torch.cuda.synchronize()
    assert (vol.sum == 0.25).all() and (vol.count == 3).all() and (vol.rgb_sum == 7).all() and (vol.rgb_count == 1).all()
    assert (tot == 99).all() and (out == 5).all() and (ws == 0).all()
    from mvsnet_amd import mesh
    with pytest.raises(ValueError):
        vol.integrate(sc["depths"], sc["probs"][:, :-1], sc["cams"])
    with pytest.raises(ValueError):
        vol.integrate(sc["depths"], sc["probs"], sc["cams"][:4])
    with pytest.raises(ValueError):
        vol.extract(min_count=0)
    with pytest.raises(ValueError):
        mesh.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), 0.4, device="cpu")


def _write_dense(folder, s):
    from mvsnet_amd import predictlib
    out = os.path.join(folder, "depths_mvsnet")
    os.makedirs(out)
    for i in range(s["depths"].shape[0]):
        predictlib.write_output_slice(out, s["depths"][i], s["probs"][i], s["images"][i][:, :, ::-1], s["cams"][i], i)


def _run(*argv):
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m"] + list(argv), cwd=ROOT, capture_output=True, text=True)
    return r.returncode, r.stdout[-2000:] + r.stderr[-2000:]


def test_command_lines_end_to_end(tmp_path):
    from mvsnet_amd import evaluate, fusion, mesh
    sc = M.scene("sphere", noisy=True)
    dense = str(tmp_path / "dense")
    _write_dense(dense, sc)
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", dense, "--voxel", "0.05")
    assert code == 0, text
    path = os.path.join(dense, "points_mvsnet", "mesh.ply")
    v, c, f = mesh.read_mesh_ply(path)
    idx, d, p, cams, im = fusion.load_dense_folder(dense)
    want = mesh.mesh_depth_maps(d, p, cams, im, voxel=0.05)
    assert len(f) > 3000 and c.std() > 5
    assert np.array_equal(v, want[0]) and np.array_equal(c, want[1]) and np.array_equal(f, want[2])
    pts, _ = evaluate.read_ply_points(path)
    assert np.array_equal(np.asarray(pts, np.float32), v)
    # the masks did their work: no face-referenced vertex is farther than 2 voxels from the surface
    assert (sc["surface_distance"](v[np.unique(f)]) / 0.05 <= 2).all()
    # an existing file is refused without --force, before any work
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", dense, "--voxel", "0.05")
    assert code != 0 and "--force" in text
    # depthfusion --fusion hip --mesh writes mesh.ply beside final3d_model.ply, with the default resolution
    code, text = _run("mvsnet_amd.depthfusion", "--dense_folder", dense, "--fusion", "hip", "--mesh")
    assert code == 0, text
    found = [b for b, _, fs in os.walk(os.path.join(dense, "points_mvsnet")) if "final3d_model.ply" in fs]
    assert len(found) == 1 and os.path.isfile(os.path.join(found[0], "mesh.ply"))
    v2, c2, f2 = mesh.read_mesh_ply(os.path.join(found[0], "mesh.ply"))
    assert len(f2) > len(f)                                                    # 256 nodes along the longest axis: finer
