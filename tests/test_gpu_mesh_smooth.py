"""GPU tests of the Taubin smoothing of csrc/mesh_smooth.hip through mvsnet_amd.mesh_smooth, against
tests/mesh_smooth_reference.py byte for byte, no tolerance: the built meshes of the reference (invalid faces and vertices that
are not finite, strips around a wave's edge, a closed sphere, a row of 200 neighbours, three faces on one edge, a face given
twice, vertices without faces, nothing) under the three boundary modes, with and without the second pass, the bound and colours,
as numpy arrays and as device tensors; a side stream, the keep-old rule near FLT_MAX, the hooks in mvsnet_amd.mesh and the
command line."""
import functools
import json

import numpy as np
import pytest

from tests import mesh_clean_reference as MC
from tests import mesh_reference as M
from tests import mesh_simplify_reference as MS
from tests import mesh_smooth_reference as R
from tests.test_gpu_arena_geometry import same_bytes
from tests.test_gpu_mesh_clean import COMMON, _json_line, _noisy_volume, _run, dense  # noqa: F401  (dense is a fixture)

pytestmark = pytest.mark.gpu
SCENE_O = np.asarray(M.SCENE_ORIGIN, np.float32)


@functools.lru_cache(maxsize=None)
def _want(name, boundary, mu, iterations, r):
    """The reference, computed once per case and shared (colours and the kind of the input do not change it)."""
    v, c, f = R.mesh(name)
    return R.smooth(v, c, f, iterations, 0.5, mu, boundary, r)


def _assert_same(got, want, colour=True):
    (v, c, f, rep), (wv, wc, wf, wrep) = got, want
    assert v.dtype == np.float32 and f.dtype == np.int32
    same_bytes(v, wv, "vertices")
    same_bytes(f, wf, "faces")
    assert (c is None) == (not colour)
    if colour:
        assert c.dtype == np.uint8
        same_bytes(c, wc, "colours")
    assert rep == wrep, (rep, wrep)


@pytest.mark.parametrize("name", R.MESHES)
def test_built_meshes_equal_the_reference(name):
    import torch
    from mvsnet_amd import mesh_smooth
    v, c, f = R.mesh(name)
    tv, tc, tf = (torch.as_tensor(x.copy()).cuda() for x in (v, c, f))         # the reference's arrays are read-only
    moved = 0
    for boundary in ("fixed", "curve", "free"):
        for mu in (-0.53, 0.0):
            for iterations in (1, 3):
                for r in (None, 0.004):
                    want = _want(name, boundary, mu, iterations, r)
                    for colour in (False, True):
                        got = mesh_smooth.smooth_mesh(v, c if colour else None, f, iterations, 0.5, mu, boundary, r)
                        assert isinstance(got[0], np.ndarray)
                        _assert_same(got, want, colour)
                        ov, oc, of, rep = mesh_smooth.smooth_mesh(tv, tc if colour else None, tf, iterations, 0.5, mu, boundary, r)
                        assert isinstance(ov, torch.Tensor) and ov.is_cuda and of.is_cuda      # tensors in, tensors out
                        _assert_same((ov.cpu().numpy(), None if oc is None else oc.cpu().numpy(), of.cpu().numpy(), rep), want, colour)
                    moved += int((want[0].view(np.uint32) != v.view(np.uint32)).any())
    same_bytes(tv.cpu().numpy(), v, "the input vertices")                      # the input is never written
    same_bytes(tf.cpu().numpy(), f, "the input faces")
    rep = _want(name, "fixed", -0.53, 1, None)[3]
    print(name, json.dumps(rep))
    assert moved == (0 if name in ("lone", "none") else 16 if name in ("three", "strip63", "strip64", "strip65") else 24), moved
    if name == "grid":
        assert (rep["invalid_faces"], rep["non_finite_vertices"]) == (4, 3)
    if name == "sphere":
        assert rep["boundary_edges"] == 0 and rep["fixed_vertices"] == 0
    if name == "fan200":
        assert _want(name, "free", 0.0, 1, None)[3]["fixed_vertices"] == 0 and rep["edges"] == 400
    if name == "three":
        assert rep["non_manifold_edges"] == 1
    if name == "doubled":
        assert rep["boundary_edges"] == 0 and rep["edges"] == 3


def test_a_side_stream_and_a_second_run_give_the_same_bytes():
    import torch
    from mvsnet_amd import mesh_smooth
    v, c, f = R.mesh("grid")
    runs = [mesh_smooth.smooth_mesh(v, c, f, 3, boundary="curve", max_displacement=0.01) for _ in range(2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(mesh_smooth.smooth_mesh(v, c, f, 3, boundary="curve", max_displacement=0.01))
    side.synchronize()
    want = R.smooth(v, c, f, 3, boundary="curve", max_displacement=0.01)
    for run in runs:
        _assert_same(run, want)


def test_a_value_near_float_max_keeps_its_old_position():
    from mvsnet_amd import mesh_smooth
    v, f = R.near_float_max()
    lam = 2.0 ** -20
    ys = R.passes(v, f, 1, lam, -1.0, "free")[1]
    got = mesh_smooth.smooth_mesh(v, None, f, 1, lam, -1.0, "free")
    same_bytes(got[0], ys[0], "the first pass's positions, kept by the second")
    assert np.isfinite(got[0]).all() and (got[0][:, 0] != v[:, 0]).all()
    same_bytes(mesh_smooth.smooth_mesh(v, None, f, 2, lam, -1.0, "free")[0], R.smooth(v, None, f, 2, lam, -1.0, "free")[0], "two iterations")


def test_invalid_options_raise_before_the_device_is_touched():
    from mvsnet_amd import mesh_smooth
    v, c, f = R.mesh("three")
    for kw in (dict(iterations=0), dict(lam=0.0), dict(mu=0.5), dict(boundary="open"), dict(max_displacement=0.0)):
        with pytest.raises(ValueError):
            mesh_smooth.smooth_mesh(v, c, f, **dict(dict(iterations=1), **kw))


# ------------------------------------------------------------------------------------------------ mesh.py and the command line

def test_extract_with_smooth_between_clean_and_simplify():
    from mvsnet_amd import mesh_clean, mesh_smooth
    vol = _noisy_volume("sphere")
    plain = vol.extract()
    assert len(plain) == 3
    for got, want in zip(plain, MC.scene_mesh("sphere", True)):                # without the option: the bytes of before
        same_bytes(got, want, "extract()")
    cell = np.float32(2 * float(np.float32(M.SCENE_VOXEL)))
    clean = dict(min_faces=8)
    cleaned = MC.scene_clean("sphere", True, min_faces=8)
    v, c, f, rep = vol.extract(clean=clean, simplify=cell)                     # the path through clean and simplify, unchanged
    assert "smooth" not in rep
    want = MS.simplify(*cleaned[:3], cell, SCENE_O)
    for got, w in zip((v, c, f), want[:3]):
        same_bytes(got, w, "extract(clean, simplify)")
    assert rep["simplify"] == want[3]
    options = dict(iterations=3, lam=0.5, mu=-0.53, boundary="fixed", max_displacement=float(np.float32(M.SCENE_VOXEL)))
    v, c, f, rep = vol.extract(smooth=options)
    assert set(rep) == {"smooth"}
    _assert_same((v, c, f, rep["smooth"]), mesh_smooth.smooth_mesh(*plain, **options))
    _assert_same((v, c, f, rep["smooth"]), R.smooth(*plain, **options))
    assert rep["smooth"]["vertices"] == len(plain[0]) and (v != plain[0]).any()
    v, c, f, rep = vol.extract(clean=clean, smooth=options, simplify=cell)     # cleaned, then smoothed, then simplified
    kept = mesh_clean.clean_mesh(*plain, **clean)
    smoothed = mesh_smooth.smooth_mesh(*kept[:3], **options)
    assert rep["smooth"] == smoothed[3] and rep["smooth"]["faces"] == kept[3]["faces_out"]
    want = MS.simplify(*smoothed[:3], cell, SCENE_O)
    for got, w in zip((v, c, f), want[:3]):
        same_bytes(got, w, "extract(clean, smooth, simplify)")
    with pytest.raises(ValueError):
        vol.extract(smooth=dict(iterations=0))


def test_mesh_depth_maps_with_smooth_iterations():
    from mvsnet_amd import mesh
    sc = M.scene("plane", noisy=False)
    bounds = (np.array(M.SCENE_ORIGIN, np.float64), np.array(M.SCENE_ORIGIN, np.float64) + M.SCENE_VOXEL * (np.array(M.SCENE_DIMS) - 1))
    kw = dict(voxel=M.SCENE_VOXEL, bounds=bounds, num_consistent=0)
    vol = mesh.TsdfVolume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, 4 * M.SCENE_VOXEL, colour=True)
    plain = vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"]).extract()
    off = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], smooth_iterations=0, smooth_lambda=0.3, **kw)
    for a, b in zip(off, plain):                                               # 0 iterations: the bytes of the extraction
        same_bytes(a, b, "smooth_iterations 0")
    v, c, f = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], smooth_iterations=2, smooth_boundary="curve",
                                   smooth_max_voxels=0.5, **kw)
    r = np.float32(0.5 * float(np.float32(M.SCENE_VOXEL)))
    want = R.smooth(*plain, 2, boundary="curve", max_displacement=r)
    same_bytes(v, want[0], "vertices")
    same_bytes(c, want[1], "colours")
    same_bytes(f, want[2], "faces")
    assert (v != plain[0]).any() and np.abs(v.astype(np.float64) - plain[0]).max() <= float(r) + 8 * 2.0 ** -24   # r and one rounding


def test_mesh_and_depthfusion_command_lines_pass_the_options_through(dense, tmp_path):
    from mvsnet_amd import mesh
    folder, raw = dense
    out, want = str(tmp_path / "smooth.ply"), str(tmp_path / "want.ply")
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", folder, *COMMON, "--out", out, "--smooth_iterations", "3", "--smooth_mu=-0.5",
                      "--smooth_max_voxels", "0.5", "--min_component_faces", "8")
    assert code == 0, text
    cleaned = MC.clean(*raw, min_faces=8)
    ref = R.smooth(*cleaned[:3], 3, 0.5, -0.5, "fixed", np.float32(0.5 * float(np.float32(0.05))))
    rep = _json_line(text)
    assert rep["smooth"] == ref[3] and rep["vertices"] == len(ref[0]) and rep["faces"] == len(ref[2])
    assert {k: rep[k] for k in cleaned[3]} == cleaned[3]                       # the cleaning ran first and reports as before
    mesh.write_mesh_ply(want, *ref[:3])
    assert open(out, "rb").read() == open(want, "rb").read()
    code, text = _run("mvsnet_amd.depthfusion", "--dense_folder", folder, "--fusion", "hip", "--mesh", "--mesh_smooth_iterations", "2",
                      "--mesh_smooth_boundary", "free")
    assert code == 0, text
    rep = _json_line(text, "meshed: ")
    assert rep["smooth"]["iterations"] == 2 and rep["smooth"]["boundary"] == "free" and rep["smooth"]["max_displacement"] > 0
    assert rep["smooth"]["vertices"] == rep["vertices"] == len(mesh.read_mesh_ply(rep["out"])[0])


def test_mesh_smooth_command_line_on_a_written_ply(tmp_path):
    from mvsnet_amd import mesh
    v, c, f = R.mesh("sphere")
    src, out, want = str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), str(tmp_path / "want.ply")
    mesh.write_mesh_ply(src, v, c, f)
    code, text = _run("mvsnet_amd.mesh_smooth", "--mesh", src, "--out", out, "--iterations", "4", "--lambda", "0.4", "--mu=-0.43",
                      "--boundary", "free", "--max_displacement", "0.05")
    assert code == 0, text
    ref = R.smooth(v, c, f, 4, 0.4, -0.43, "free", 0.05)
    rep = _json_line(text)
    assert {k: rep[k] for k in ref[3]} == ref[3] and rep["out"] == out
    mesh.write_mesh_ply(want, *ref[:3])
    assert open(out, "rb").read() == open(want, "rb").read()
    code, text = _run("mvsnet_amd.mesh_smooth", "--mesh", src, "--out", out, "--iterations", "1")  # refused before any GPU work
    assert code != 0 and "--force" in text
