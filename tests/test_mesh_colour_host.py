"""Host-side tests of mvsnet_amd.mesh_colour and of its numpy restatement tests/mesh_colour_reference.py, no GPU: known answers
worked out by hand (a constant image, a ramp, the hidden plane, a back view, power 0, the normals of a tetrahedron and of a flat
grid), the placement of the hazards in the case table, the error text of every bad option, the parsers, the PLY with normals, and
one fidelity check that holds the reference to the world."""
import numpy as np
import pytest

from mvsnet_amd import mesh_colour as MCo
from tests import mesh_colour_reference as R

F32 = np.float32


def _triangle_at(pixels, z=2.0):
    """Three vertices that scene "one"'s camera sees at the pixel positions `pixels` (3,2) and depth z, wound towards it."""
    pix = np.asarray(pixels, np.float64)
    v = np.stack([(pix[:, 0] - (R.ONE_W - 1) / 2.0) * z / R.ONE_F, (pix[:, 1] - (R.ONE_H - 1) / 2.0) * z / R.ONE_F, np.full(3, z)], 1)
    return v.astype(F32), np.array([[0, 1, 2]], np.int32)


def _one_camera():
    return R.scene("one")["cams"]


# ------------------------------------------------------------------------------------------------ known answers

def test_a_triangle_in_front_of_one_camera_takes_the_colour_of_a_constant_image():
    v, f = _triangle_at([[5.8, 3.9], [11.1, 16.3], [18.3, 4.8]])               # the pixel nearest to each corner lies inside
    image = np.empty((R.ONE_H, R.ONE_W, 3), np.uint8)
    image[:] = (200, 17, 90)
    _, colours, _, report, state = R.colour(v, None, f, _one_camera(), [image])
    assert (colours == [200, 17, 90]).all() and report["unseen_vertices"] == 0 and (state["seen"] == 1).all()
    assert (state["normals"] == [0, 0, -1]).all()


def test_a_ramp_image_gives_the_hand_computed_bilinear_value():
    """Image value 8 x in every channel.  The vertices sit at x = 8.75, 15.25 and 12, so the samples are 0.25 * 64 + 0.75 * 72
    = 70, 0.75 * 120 + 0.25 * 128 = 122 and 96, whatever y is, and a single view's weighted mean is the sample."""
    v, f = _triangle_at([[8.75, 10.0], [15.25, 12.25], [12.0, 3.75]])
    image = np.repeat((8 * np.arange(R.ONE_W, dtype=np.uint8))[None, :, None], R.ONE_H, 0).repeat(3, 2)
    _, colours, _, _, state = R.colour(v, None, f, _one_camera(), [image])
    assert (state["seen"] == 1).all()
    assert colours.tolist() == [[70] * 3, [122] * 3, [96] * 3]
    assert np.abs(state["acc"][:, 0] / state["acc"][:, 3] - [70.0, 122.0, 96.0]).max() < 1e-4


REAR = slice(63, 88)                                # the rear plane's vertices in the mesh "grid"


def test_the_hidden_plane_keeps_its_colour_until_a_view_sees_it():
    v, c, f = R.mesh("grid")
    s = R.scene("three")
    front = R.colour(v, c, f, s["cams"], s["images"], views=[0, 1])
    assert (front[4]["seen"][REAR] == 0).all() and np.array_equal(front[1][REAR], c[REAR])
    trace = []
    R.colour(v, c, f, s["cams"], s["images"], views=[0, 1], trace=trace)
    assert all(t["hidden"][REAR].all() for t in trace)                         # fully hidden in both, by the depth test
    side = R.colour(v, c, f, s["cams"], s["images"], views=[2])
    every = R.colour(v, c, f, s["cams"], s["images"])
    shown = every[4]["seen"][REAR] == 1                                        # its inner vertices: the pixel next to a border vertex is empty
    assert shown.reshape(5, 5)[1:4, 1:4].all() and (every[4]["seen"][REAR] <= 1).all()
    assert np.array_equal(every[1][REAR], side[1][REAR]) and (every[1][REAR][shown] != c[REAR][shown]).any(1).all()
    assert np.array_equal(every[1][REAR][~shown], c[REAR][~shown])


def test_a_back_view_contributes_nothing():
    v, c, f = R.mesh("grid")
    s = R.scene("five")
    trace = []
    alone = R.colour(v, c, f, s["cams"], s["images"], views=[0])
    both = R.colour(v, c, f, s["cams"], s["images"], views=[0, 1], trace=trace)
    assert trace[1]["back"].any() and not trace[1]["sees"].any()
    assert np.array_equal(alone[4]["acc"], both[4]["acc"]) and np.array_equal(alone[1], both[1])


def test_power_zero_is_the_plain_mean():
    v, c, f = R.mesh("grid")
    s = R.scene("nine")
    got = R.colour(v, c, f, s["cams"], s["images"], angle_power=0)
    acc, seen = got[4]["acc"], got[4]["seen"]
    assert np.array_equal(acc[:, 3], seen.astype(np.float64)) and seen.max() > 3
    total = np.zeros((len(v), 3))
    for k in range(9):                                                         # a single view's sums are its samples
        one = R.colour(v, c, f, s["cams"], s["images"], angle_power=0, views=[k])[4]
        total = total + one["acc"][:, :3]
    assert np.array_equal(total, acc[:, :3])
    took = seen > 0
    assert np.array_equal(got[1][took], np.floor(total[took] / seen[took, None] + 0.5).astype(np.uint8))


def test_normals_of_the_tetrahedron_and_of_a_flat_grid():
    v, _, f = R.mesh("tetra")
    n, info = R.normals(v, f)
    want = ((v.astype(np.float64) - [0, 0, 4.0]) / np.sqrt(0.75)).astype(F32)  # outward: along the vertex from the centre
    assert np.array_equal(n, want) and info["zero_normals"] == 0 and info["invalid_faces"] == 0
    gv, gf = R.plane(9, 7, -1.0, 1.0, -0.75, 0.75, 4.0)
    n, info = R.normals(gv, gf)
    assert (n == [0, 0, -1]).all() and info["zero_normals"] == 0
    n, info = R.normals(*R.mesh("grid")[::2])
    assert info["invalid_faces"] == 4 and info["zero_normals"] == 2 and (n[-2:] == 0).all()
    keys = info["keys"].reshape(-1, 3)
    assert (keys[-4:] == R.DEAD).all() and (keys[0] == (np.array(R.mesh("grid")[2][0], np.int64) << 31)).all()


def test_every_hazard_occurs_in_the_case_table():
    found = set()
    for m in R.MESHES:
        for s in R.SCENES:
            found |= R.hazards(m, s)
    assert found == set(R.HAZARDS), set(R.HAZARDS) - found
    assert {"left", "right", "top", "bottom"} <= R.hazards("grid", "one")       # the four tabs clamp their taps in scene "one"
    assert "hidden then seen" in R.hazards("grid", "three")
    assert [len(R.scene(s)["images"]) for s in R.SCENES] == [1, 3, 5, 4, 9]
    assert len({im.shape for im in R.scene("mixed")["images"]}) == 2 and len(R.scene("nine")["images"]) > R.DEFAULTS["view_chunk"]
    assert [len(R.mesh(m)[0]) for m in R.MESHES if m.startswith("strip")] == [63, 65, 257] and len(R.mesh("none")[0]) == 0


def test_the_reference_and_the_module_share_their_host_formulas():
    for name in R.SCENES:
        cams = R.scene(name)["cams"]
        assert MCo.camera_centres(cams).tobytes() == R.camera_centres(cams).tobytes()
    for rel in (0.0, 0.01, 0.3, 1e-9):
        assert MCo.occlusion_ratio(rel) == float(R.occlusion_ratio(rel))
    assert MCo.REPORT_FIELDS == R.REPORT_FIELDS and MCo.check_options() == tuple(
        float(F32(v)) if k in ("min_cos", "min_depth") else v for k, v in R.DEFAULTS.items())


def test_scale_cams_keeps_pixel_centres_at_integers():
    cams = R.scene("three")["cams"]
    big = MCo.scale_cams(cams, R.LARGE, (58, 74))
    assert MCo.scale_cams(cams, R.LARGE, R.LARGE).tobytes() == np.asarray(cams).tobytes()
    X = np.array([0.3, -0.2, 4.0, 1.0])
    for k in range(3):
        p, q = cams[k, 1, :3, :3] @ (cams[k, 0] @ X)[:3], big[k, 1, :3, :3] @ (big[k, 0] @ X)[:3]
        assert np.allclose((p[:2] / p[2] + 0.5) * 2 - 0.5, q[:2] / q[2], rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------------ options, parsers, files

BAD_OPTIONS = [
    (dict(min_cos=-0.1), "min_cos must lie in [0, 1] as a float32, got -0.1"),
    (dict(min_cos=1.5), "min_cos must lie in [0, 1] as a float32, got 1.5"),
    (dict(min_cos=float("nan")), "min_cos must lie in [0, 1] as a float32, got nan"),
    (dict(min_cos="x"), "min_cos must be a number, got 'x'"),
    (dict(min_cos=True), "min_cos must be a number, got True"),
    (dict(angle_power=9), "angle_power must be an integer 0 .. 8, got 9"),
    (dict(angle_power=-1), "angle_power must be an integer 0 .. 8, got -1"),
    (dict(angle_power=1.5), "angle_power must be an integer 0 .. 8, got 1.5"),
    (dict(angle_power=None), "angle_power must be an integer 0 .. 8, got None"),
    (dict(occlusion_rel=-0.01), "occlusion_rel must be >= 0 with a finite float32(1 + rel), got -0.01"),
    (dict(occlusion_rel=1e39), "occlusion_rel must be >= 0 with a finite float32(1 + rel), got 1e+39"),
    (dict(occlusion_rel=float("nan")), "occlusion_rel must be >= 0 with a finite float32(1 + rel), got nan"),
    (dict(occlusion_rel=None), "occlusion_rel must be a number, got None"),
    (dict(min_depth=-1.0), "min_depth must be >= 0 and finite in float32, got -1.0"),
    (dict(min_depth=1e39), "min_depth must be >= 0 and finite in float32, got 1e+39"),
    (dict(min_depth=float("inf")), "min_depth must be >= 0 and finite in float32, got inf"),
    (dict(view_chunk=0), "view_chunk must be an integer 1 .. 2^31-1, got 0"),
    (dict(view_chunk=2.5), "view_chunk must be an integer 1 .. 2^31-1, got 2.5"),
    (dict(view_chunk=2 ** 31), "view_chunk must be an integer 1 .. 2^31-1, got 2147483648"),
]


@pytest.mark.parametrize("options, text", BAD_OPTIONS, ids=[t for _, t in BAD_OPTIONS])
def test_bad_options_say_what_is_wrong(options, text):
    with pytest.raises(ValueError) as e:
        MCo.check_options(**options)
    assert str(e.value) == text


def test_good_options_come_back_as_the_kernels_take_them():
    assert MCo.check_options(0.25, 0, 0.0, 0.5, 3) == (0.25, 0, 0.0, 0.5, 3)
    assert MCo.check_options(min_cos=0.1)[0] == float(F32(0.1)) and MCo.check_options(min_cos=-0.0)[0] == 0.0
    assert MCo.check_options(angle_power=np.int64(8), view_chunk=np.int32(1))[1::3] == (8, 1)


def test_bad_views_are_refused_before_any_gpu_work():
    v, c, f = R.mesh("tetra")
    s = R.scene("three")
    for cams, images, text in ((s["cams"][:2], s["images"], "3 images for 2 cameras"),
                               (s["cams"], [im[..., :2] for im in s["images"]], "must be (H,W,3) uint8"),
                               (s["cams"], [im.astype(np.float32) for im in s["images"]], "must be (H,W,3) uint8"),
                               (s["cams"][:, :1], s["images"], "cams must be (V,2,4,4)")):
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
            MCo.colour_mesh(v, c, f, cams, images)
    with pytest.raises(ValueError, match="angle_power"):
        MCo.colour_mesh(v, c, f, s["cams"], s["images"], angle_power=9)
    with pytest.raises(ValueError, match="colours must be"):
        MCo.colour_mesh(v, c[:2], f, s["cams"], s["images"])


def test_the_command_line_parser():
    a = MCo.parse_args(["--mesh", "a.ply", "--out", "b.ply", "--session", "s"])
    assert (a.min_cos, a.angle_power, a.occlusion_rel, a.min_depth, a.view_chunk) == MCo.check_options()
    assert a.mesh_scale == 1.0 and a.transform is None and not a.write_normals and not a.force and a.dense_folder is None
    a = MCo.parse_args(["--mesh", "a.ply", "--out", "b.ply", "--dense_folder", "d", "--min_cos", "0.5", "--angle_power", "0",
                        "--occlusion_rel", "0.05", "--min_depth", "2", "--view_chunk", "3", "--mesh_scale", "1000", "--transform", "T.txt",
                        "--write_normals", "--force"])
    assert (a.min_cos, a.angle_power, a.occlusion_rel, a.min_depth, a.view_chunk) == (0.5, 0, 0.05, 2.0, 3)
    assert a.mesh_scale == 1000.0 and a.transform == "T.txt" and a.write_normals and a.force and a.session is None
    for bad, text in ((["--angle_power", "9"], "--angle_power must be an integer 0 .. 8, got 9"), (["--min_cos", "2"], "--min_cos must lie"),
                      (["--view_chunk", "0"], "--view_chunk must be"), (["--mesh_scale", "0"], "--mesh_scale must be positive")):
        with pytest.raises(SystemExit) as e:
            MCo.parse_args(["--mesh", "a.ply", "--out", "b.ply", "--session", "s"] + bad)
        assert text in str(e.value)
    with pytest.raises(SystemExit):
        MCo.parse_args(["--mesh", "a.ply", "--out", "b.ply"])                  # neither a session nor a dense folder
    with pytest.raises(SystemExit):
        MCo.parse_args(["--mesh", "a.ply", "--out", "b.ply", "--session", "s", "--dense_folder", "d"])


def test_mesh_and_depthfusion_take_the_prefixed_options():
    import argparse
    from mvsnet_amd import mesh
    a = mesh.parse_args(["--dense_folder", "d"])
    assert a.stages["recolour"] is None and not a.recolour
    a = mesh.parse_args(["--dense_folder", "d", "--recolour", "--recolour_min_cos", "0.5", "--recolour_angle_power", "4",
                         "--recolour_occlusion_rel", "0.02"])
    assert a.stages["recolour"] == dict(min_cos=0.5, angle_power=4, occlusion_rel=0.02)
    with pytest.raises(SystemExit) as e:
        mesh.parse_args(["--dense_folder", "d", "--recolour_angle_power", "9"])                   # checked without --recolour too
    assert "--recolour_angle_power" in str(e.value) and "0 .. 8" in str(e.value)
    ap = argparse.ArgumentParser()
    MCo.add_options(ap, "mesh_")
    a = ap.parse_args(["--mesh_recolour", "--mesh_recolour_min_cos", "0.3"])
    assert MCo.check_arguments(a, "mesh_") == dict(min_cos=float(F32(0.3)), angle_power=2, occlusion_rel=0.01)
    assert MCo.check_arguments(ap.parse_args([]), "mesh_") is None
    with pytest.raises(ValueError, match="--mesh_recolour_min_cos"):
        MCo.check_arguments(ap.parse_args(["--mesh_recolour_min_cos", "7"]), "mesh_")


def test_the_ply_with_normals_round_trips(tmp_path):
    from mvsnet_amd import mesh
    v, c, f = R.mesh("tetra")
    n = R.normals(v, f)[0]
    path = str(tmp_path / "n.ply")
    MCo.write_mesh_ply_normals(path, v, n, c, f)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode()
    props = [ln.split()[-1] for ln in head.splitlines() if ln.startswith("property")]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "vertex_indices"]
    for got, want in zip(MCo.read_mesh_ply_normals(path), (v, n, c, f)):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    from mvsnet_amd.mesh_sample import read_ply_mesh                           # the general reader skips the normals
    for got, want in zip(read_ply_mesh(path), (v, c, f)):
        assert got.tobytes() == want.tobytes()
    plain = str(tmp_path / "plain.ply")
    mesh.write_mesh_ply(plain, v, c, f)
    with pytest.raises(ValueError, match="not a PLY written by write_mesh_ply_normals"):
        MCo.read_mesh_ply_normals(plain)
    with pytest.raises(ValueError, match="differ in length"):
        MCo.write_mesh_ply_normals(path, v, n[:2], c, f)
    none = np.zeros((0, 3))
    MCo.write_mesh_ply_normals(path, none, none, none, none)
    assert [len(x) for x in MCo.read_mesh_ply_normals(path)] == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the reference against the world

# The worst deviation of the reference's weighted mean from the analytic colour, measured here on the CPU before the final
# rounding, is 0.3887 levels (the images are rounded to bytes, at most half a level per tap, and a bilinear sample of a colour
# that is linear in the world is not exactly linear in the image); the bound is that value plus one level for the final
# rounding to a byte.  After the rounding the test measures 0.5.
FIDELITY_BOUND = 0.39 + 1.0


def _world_colour(x, y):
    """Linear in world x, y, inside 0 .. 255 on the plane's extent."""
    return np.stack([128.0 + 90.0 * x + 20.0 * y, 100.0 - 40.0 * x + 70.0 * y, 60.0 + 30.0 * x - 50.0 * y], -1)


def test_the_reference_recovers_a_colour_that_is_linear_on_a_plane():
    """Images of the plane z = 4 are synthesised from a colour that is linear in world x, y: every pixel's ray is intersected
    with the plane exactly (float64) and the colour there is rounded to a byte.  A 9 x 7 grid on the plane, its colours zeroed,
    is recoloured by the reference from three views, and every vertex is compared with the analytic colour at its position."""
    v, f = R.plane(9, 7, -1.0, 1.0, -0.75, 0.75, 4.0)
    cams = R.scene("three")["cams"][:2]
    cams = np.concatenate([cams, R.look_at((0.2, -1.0, 0.5), R.TARGET, 60.0, *R.LARGE)[None]])
    H, W = R.LARGE
    images = []
    for cam in cams:
        Rm, t, K = cam[0, :3, :3], cam[0, :3, 3], cam[1, :3, :3]
        yy, xx = np.mgrid[0:H, 0:W]
        rays = (np.linalg.inv(K) @ np.stack([xx, yy, np.ones_like(xx)]).reshape(3, -1).astype(np.float64))
        rays = Rm.T @ rays                                                     # world directions; the centre is -R^T t
        centre = -Rm.T @ t
        lam = (4.0 - centre[2]) / rays[2]
        hit = centre[:, None] + lam * rays
        images.append(np.clip(np.floor(_world_colour(hit[0], hit[1]) + 0.5), 0, 255).astype(np.uint8).reshape(H, W, 3))
    _, colours, _, report, state = R.colour(v, np.zeros((len(v), 3), np.uint8), f, cams, images)
    took = state["seen"] > 0                                                   # the pixel next to a border vertex may be empty
    assert (state["seen"].reshape(7, 9)[1:6, 1:8] == 3).all() and took.sum() >= 50
    want = _world_colour(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64))
    worst = float(np.abs(colours.astype(np.float64) - want)[took].max())
    before = float(np.abs(state["acc"][took, :3] / state["acc"][took, 3:] - want[took]).max())
    print("worst deviation: %.4f levels after the final rounding, %.4f before it" % (worst, before))
    assert worst <= FIDELITY_BOUND
