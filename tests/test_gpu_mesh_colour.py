"""GPU tests of the vertex normals and the colouring of csrc/mesh_colour.hip through mvsnet_amd.mesh_colour, against
tests/mesh_colour_reference.py byte for byte, no tolerance: every built mesh in every scene of the reference (normals, the float64
sums, the counts, the report and the final colours, with and without input colours, as numpy arrays and as device tensors),
chunks of 1, 2 and V views, a side stream, two calls that continue one set of sums, the hook in mvsnet_amd.mesh and the command
lines on a session and a dense folder."""
import functools
import json
import os

import numpy as np
import pytest

from tests import mesh_colour_reference as R
from tests import mesh_reference as M
from tests._helpers import make_session
from tests.test_gpu_arena_geometry import same_bytes
from tests.test_gpu_mesh_clean import COMMON, _json_line, _run, _write_dense, dense  # noqa: F401  (dense is a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    from mvsnet_amd import _lib as L
    import torch
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def _assert_same(got, want, state=None):
    """(vertices, colours, faces, report) against the reference's (vertices, colours, faces, report, state, ...)."""
    v, c, f, rep = got
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    same_bytes(v, want[0], "vertices")
    same_bytes(f, want[2], "faces")
    if state is not None:
        same_bytes(state["normals"].cpu().numpy(), want[4]["normals"], "normals")
        same_bytes(state["acc"].cpu().numpy(), want[4]["acc"], "acc")
        same_bytes(state["seen"].cpu().numpy(), want[4]["seen"], "seen")
    assert rep == want[3], (rep, want[3])
    same_bytes(c, want[1], "colours")


@pytest.mark.parametrize("scene", R.SCENES)
@pytest.mark.parametrize("name", R.MESHES)
def test_every_mesh_in_every_scene_equals_the_reference(name, scene):
    import torch
    from mvsnet_amd import mesh_colour
    v, c, f = R.mesh(name)
    s = R.scene(scene)
    want = R.case(name, scene)
    print(name, scene, json.dumps(want[3]), sorted(R.hazards(name, scene)))
    normals = mesh_colour.vertex_normals(v, f)
    assert isinstance(normals, np.ndarray) and normals.dtype == np.float32
    same_bytes(normals, want[4]["normals"], "vertex_normals")
    state = {}
    _assert_same(mesh_colour.colour_mesh(v, c, f, s["cams"], s["images"], state=state), want, state)
    state = {}
    _assert_same(mesh_colour.colour_mesh(v, None, f, s["cams"], s["images"], state=state), R.case(name, scene, False), state)
    tv, tc, tf = (torch.as_tensor(x.copy()).cuda() for x in (v, c, f))         # the reference's arrays are read-only
    tn = mesh_colour.vertex_normals(tv, tf)
    assert isinstance(tn, torch.Tensor) and tn.is_cuda
    same_bytes(tn.cpu().numpy(), want[4]["normals"], "vertex_normals of tensors")
    ov, oc, of, rep = mesh_colour.colour_mesh(tv, tc, tf, s["cams"], [torch.as_tensor(im.copy()).cuda() for im in s["images"]])
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (ov, oc, of))                    # tensors in, tensors out
    _assert_same((ov.cpu().numpy(), oc.cpu().numpy(), of.cpu().numpy(), rep), want)
    for t, x, what in ((tv, v, "vertices"), (tc, c, "colours"), (tf, f, "faces")):                  # the inputs are never written
        same_bytes(t.cpu().numpy(), x, "the input " + what)
    if name == "grid":
        assert (rep["invalid_faces"], rep["zero_normals"]) == (4, 2) and 0 < rep["unseen_vertices"] < len(v)
    if name == "none":
        assert rep["vertices"] == 0 and rep["unseen_vertices"] == 0 and len(oc) == 0


@pytest.mark.parametrize("scene", ["five", "mixed", "nine"])
def test_chunks_of_one_two_and_all_views_give_the_same_bytes(scene):
    from mvsnet_amd import mesh_colour
    v, c, f = R.mesh("grid")
    s = R.scene(scene)
    want = R.case("grid", scene)
    for chunk in (1, 2, len(s["images"])):
        state = {}
        got = mesh_colour.colour_mesh(v, c, f, s["cams"], s["images"], view_chunk=chunk, state=state)
        _assert_same(got[:3] + (dict(got[3], view_chunk=8),), want, state)
        assert got[3]["view_chunk"] == chunk


def test_a_side_stream_and_a_second_run_give_the_same_bytes():
    import torch
    from mvsnet_amd import mesh_colour
    v, c, f = R.mesh("strip257")
    s = R.scene("three")
    runs = [mesh_colour.colour_mesh(v, c, f, s["cams"], s["images"]) for _ in range(2)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(mesh_colour.colour_mesh(v, c, f, s["cams"], s["images"]))
    side.synchronize()
    for run in runs:
        _assert_same(run, R.case("strip257", "three"))


def test_two_calls_continue_one_set_of_sums():
    from mvsnet_amd import mesh_colour
    v, c, f = R.mesh("grid")
    s = R.scene("nine")
    want = R.case("grid", "nine")
    state = {}
    first = mesh_colour.colour_mesh(v, c, f, s["cams"][:4], s["images"][:4], state=state)
    half = R.colour(v, c, f, s["cams"], s["images"], views=range(4))
    _assert_same(first, half, state)
    again = mesh_colour.colour_mesh(v, c, f, s["cams"][4:], s["images"][4:], state=state)
    _assert_same(again[:3] + (dict(again[3], views=9),), want, state)                              # the sums of one call with all views
    assert again[3]["views"] == 5
    with pytest.raises(ValueError, match="another mesh"):
        mesh_colour.colour_mesh(*R.mesh("tetra"), s["cams"], s["images"], state=state)


def test_other_options_equal_the_reference():
    from mvsnet_amd import mesh_colour
    v, c, f = R.mesh("grid")
    s = R.scene("five")
    for options in (dict(angle_power=0), dict(angle_power=8, min_cos=0.5), dict(occlusion_rel=0.0, min_depth=3.8), dict(min_cos=0.0, angle_power=1)):
        state = {}
        got = mesh_colour.colour_mesh(v, c, f, s["cams"], s["images"], state=state, **options)
        _assert_same(got, R.colour(v, c, f, s["cams"], s["images"], **options), state)
    with pytest.raises(ValueError):
        mesh_colour.colour_mesh(v, c, f, s["cams"], s["images"], angle_power=9)


# ------------------------------------------------------------------------------------------------ mesh.py and the command lines

def test_mesh_depth_maps_with_recolour():
    from mvsnet_amd import mesh, mesh_colour
    sc = M.scene("plane", noisy=False)
    bounds = (np.array(M.SCENE_ORIGIN, np.float64), np.array(M.SCENE_ORIGIN, np.float64) + M.SCENE_VOXEL * (np.array(M.SCENE_DIMS) - 1))
    kw = dict(voxel=M.SCENE_VOXEL, bounds=bounds, num_consistent=0)
    plain = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], **kw)
    off = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], recolour=None, **kw)
    for a, b in zip(off, plain):                                               # without it: the bytes of a call without the argument
        same_bytes(a, b, "recolour None")
    cams = mesh_colour.scale_cams(sc["cams"], sc["depths"].shape[1:3], sc["images"].shape[1:3])
    for recolour, options in ((True, {}), (dict(angle_power=0, min_cos=0.3), dict(angle_power=0, min_cos=0.3))):
        v, c, f = mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], sc["images"], recolour=recolour, **kw)
        want = mesh_colour.colour_mesh(*plain, cams, sc["images"], **options)
        same_bytes(v, plain[0], "vertices")
        same_bytes(f, plain[2], "faces")
        same_bytes(c, want[1], "colours")
        assert (c != plain[1]).any() and want[3]["unseen_vertices"] < len(v) // 2
    vol = mesh.TsdfVolume(M.SCENE_ORIGIN, M.SCENE_VOXEL, M.SCENE_DIMS, 4 * M.SCENE_VOXEL, colour=True)
    vol.integrate(sc["depths"], sc["probs"], sc["cams"], sc["images"])
    v, c, f, rep = vol.extract(clean=dict(min_faces=8), recolour=dict(cams=cams, images=sc["images"]))   # the last stage, after the others
    cleaned = vol.extract(clean=dict(min_faces=8))
    want = mesh_colour.colour_mesh(*cleaned[:3], cams, sc["images"])
    same_bytes(c, want[1], "extract(clean, recolour)")
    assert rep["recolour"] == want[3] and rep["recolour"]["vertices"] == len(v)
    with pytest.raises(ValueError):
        vol.extract(recolour=dict(cams=cams, images=sc["images"], min_cos=2.0))
    with pytest.raises(ValueError, match="needs the images"):
        mesh.mesh_depth_maps(sc["depths"], sc["probs"], sc["cams"], None, recolour=True, **kw)


def test_mesh_and_depthfusion_command_lines_pass_the_options_through(dense, tmp_path):
    from mvsnet_amd import fusion, mesh, mesh_colour
    folder, raw = dense
    out = str(tmp_path / "recoloured.ply")
    code, text = _run("mvsnet_amd.mesh", "--dense_folder", folder, *COMMON, "--out", out, "--recolour", "--recolour_angle_power", "1")
    assert code == 0, text
    _, d, _, cams, im = fusion.load_dense_folder(folder)
    want = mesh_colour.colour_mesh(*raw, mesh_colour.scale_cams(cams, d.shape[1:3], im.shape[1:3]), im, angle_power=1)
    rep = _json_line(text)
    assert rep["recolour"] == want[3] and rep["vertices"] == len(raw[0])
    got = mesh.read_mesh_ply(out)
    same_bytes(got[0], raw[0], "vertices")
    same_bytes(got[2], raw[2], "faces")
    same_bytes(got[1], want[1], "colours")
    code, text = _run("mvsnet_amd.depthfusion", "--dense_folder", folder, "--fusion", "hip", "--mesh", "--mesh_recolour",
                      "--mesh_recolour_min_cos", "0.4")
    assert code == 0, text
    rep = _json_line(text, "meshed: ")
    assert rep["recolour"]["min_cos"] == float(np.float32(0.4)) and rep["recolour"]["vertices"] == rep["vertices"]
    assert rep["recolour"]["unseen_vertices"] < rep["vertices"]


@functools.lru_cache(maxsize=None)
def _wall(cam):
    """A 7 x 6 grid on a wall 600 mm in front of the session's camera 0, overfilling its 48 x 64 image, in metres."""
    from tests import fusion_reference as F
    uu, vv = np.meshgrid(np.linspace(-18.0, 102.0, 7), np.linspace(-10.0, 70.0, 6))
    mm = F._backproject(np.frombuffer(cam, np.float64).reshape(2, 4, 4), uu.reshape(-1), vv.reshape(-1), np.full(42, 600.0))
    return (mm / 1000.0).astype(np.float32), R.plane(7, 6, 0, 1, 0, 1, 0)[1]


def test_command_line_colours_a_mesh_from_a_session(tmp_path):
    from PIL import Image
    from mvsnet_amd import mesh, mesh_colour
    from mvsnet_amd import render as Rn
    session = make_session(str(tmp_path / "s"))
    views = Rn.session_views(session)
    cams = np.stack([v[1] for v in views])
    verts, faces = _wall(np.ascontiguousarray(views[0][1], np.float64).tobytes())
    rgb = np.full((len(verts), 3), 7, np.uint8)
    ply, out, want = str(tmp_path / "m.ply"), str(tmp_path / "out.ply"), str(tmp_path / "want.ply")
    mesh.write_mesh_ply(ply, verts, rgb, faces)
    code, text = _run("mvsnet_amd.mesh_colour", "--mesh", ply, "--out", out, "--session", session, "--mesh_scale", "1000", "--view_chunk", "3")
    assert code == 0, text
    images = [np.asarray(Image.open(os.path.join(session, "images", "%d.jpg" % i)).convert("RGB")) for i in range(4)]
    scaled = (verts.astype(np.float64) * 1000.0).astype(np.float32)
    ref = R.colour(scaled, rgb, faces, cams, images, view_chunk=3)
    rep = _json_line(text)
    assert {k: rep[k] for k in ref[3]} == ref[3] and rep["out"] == out and 0 < rep["unseen_vertices"] < len(verts)
    mesh.write_mesh_ply(want, verts, ref[1], faces)                            # the written positions are the input's own
    assert open(out, "rb").read() == open(want, "rb").read()
    code, text = _run("mvsnet_amd.mesh_colour", "--mesh", ply, "--out", out, "--session", session, "--mesh_scale", "1000")
    assert code != 0 and "--force" in text and "Traceback" not in text         # refused before any GPU work
    code, text = _run("mvsnet_amd.mesh_colour", "--mesh", ply, "--out", out, "--session", session, "--mesh_scale", "1000", "--force",
                      "--write_normals", "--angle_power", "0")
    assert code == 0, text
    gv, gn, gc, gf = mesh_colour.read_mesh_ply_normals(out)
    same_bytes(gv, verts, "vertices")
    same_bytes(gf, faces, "faces")
    same_bytes(gn, R.normals(verts, faces)[0], "normals")
    same_bytes(gc, R.colour(scaled, rgb, faces, cams, images, angle_power=0)[1], "colours")


def test_command_line_colours_a_mesh_from_a_dense_folder(tmp_path):
    from mvsnet_amd import fusion, mesh, mesh_colour
    from tests import raster_reference as RR
    folder = str(tmp_path / "dense")
    _write_dense(folder, M.scene("plane", noisy=False))
    verts, rgb, faces, _ = RR.scene_mesh("plane")
    faces = faces[:600]
    used, faces = np.unique(faces, return_inverse=True)
    verts, rgb, faces = verts[used], rgb[used], faces.reshape(-1, 3).astype(np.int32)
    ply, out, want = str(tmp_path / "m.ply"), str(tmp_path / "out.ply"), str(tmp_path / "want.ply")
    mesh.write_mesh_ply(ply, verts, rgb, faces)
    code, text = _run("mvsnet_amd.mesh_colour", "--mesh", ply, "--out", out, "--dense_folder", folder, "--occlusion_rel", "0.02")
    assert code == 0, text
    _, d, _, cams, im = fusion.load_dense_folder(folder)
    ref = R.colour(verts, rgb, faces, mesh_colour.scale_cams(cams, d.shape[1:3], im.shape[1:3]), list(im), occlusion_rel=0.02)
    rep = _json_line(text)
    assert {k: rep[k] for k in ref[3]} == ref[3] and rep["unseen_vertices"] < len(verts)
    mesh.write_mesh_ply(want, verts, ref[1], faces)
    assert open(out, "rb").read() == open(want, "rb").read()
