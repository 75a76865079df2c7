"""Host tests (no GPU) of the normal estimation's float64 reference (tests/normals_reference.py) on scenes whose normals are
known, of the PLY with normals, and of the argument checks of mvsnet_amd.fusion / depthfusion that run before any GPU work."""
import inspect
import os

import numpy as np
import pytest

from mvsnet_amd import depthfusion as DF, evaluate as E, fusion as F
from mvsnet_amd.fusion import estimate_normals, read_ply_normals
from tests import normals_reference as NR
from tests import test_gpu_normals as G

# Analytic planes (Z = const, normal (0, 0, -1) towards the cameras).  The reference is float64, but the depth maps are stored
# float32: a depth in [4, 8) is off by up to half an ulp, 2.4e-7, a difference of two by up to 4.8e-7.  The shortest baseline is
# the one-sided one, one pixel = d / f = 4 / 40 = 0.1 in the world, so a tangent's slope is off by up to 4.8e-6 rad and the
# normal, with two tangents, by up to sqrt(2) x 4.8e-6 rad = 3.9e-4 degrees.
PLANE_BOUND_DEG = 4e-4


def _defaults():
    sig = inspect.signature(estimate_normals).parameters
    return dict(prob_threshold=sig["prob_threshold"].default, jump_threshold=sig["jump_threshold"].default)


@pytest.mark.parametrize("name", ["plane", "kat", "step"])
def test_reference_normals_on_analytic_planes(name):
    """plane / kat: one plane; step: two half planes Z = 4 and Z = 3.2, both with normal (0, 0, -1) -- a tangent taken across the
    step (a depth jump of 20 %, above the 5 % limit) would tilt the normal by tens of degrees."""
    s = G._scene(name)
    ref = NR.reference_normals(s["depths"], s["probs"], s["cams"], **_defaults())
    valid = (s["depths"] > 0) & (s["probs"] >= 0.8)
    has = ref["has"]
    assert not has[~valid].any()
    # a valid pixel lacks a normal when both neighbours of an axis are invalid (5 % each) or outside: about 1 %
    assert has.sum() >= 0.98 * valid.sum(), has.sum() / valid.sum()
    ang = NR.angle_deg(ref["normals"][has], np.array([0.0, 0.0, -1.0]))
    print(name, "worst angle to (0, 0, -1): %.3e degrees, %.4f of valid pixels have a normal" % (ang.max(), has.sum() / valid.sum()))
    assert ang.max() <= PLANE_BOUND_DEG, ang.max()
    assert np.array_equal(ref["normals"][~has], np.zeros((int((~has).sum()), 3)))


@pytest.mark.parametrize("name", ["plane", "step", "sphere", "kat"])
def test_reference_normals_are_unit_and_face_the_camera(name):
    s = G._scene(name)
    ref = NR.reference_normals(s["depths"], s["probs"], s["cams"])
    V, H, W = s["depths"].shape
    yy, xx = np.mgrid[0:H, 0:W]
    for v in range(V):
        has = ref["has"][v]
        n = ref["normals"][v][has]
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12
        X = NR._backproject(s["cams"][v], xx[has], yy[has], s["depths"][v][has].astype(np.float64))
        C = -s["cams"][v][0][:3, :3].T @ s["cams"][v][0][:3, 3]
        assert ((n * (X - C)).sum(1) < 0).all()


def test_reference_normals_neighbour_rules():
    """Hand-made 3 x 4 map, identity camera: a pixel with no usable neighbour on one axis has no normal, one-sided
    differences are used at borders and next to holes and jumps, and a jump just under / over the limit switches a neighbour."""
    cam = np.zeros((1, 2, 4, 4))
    cam[0, 0] = np.eye(4)
    cam[0, 1, :3, :3] = np.array([[10.0, 0, 1.5], [0, 10.0, 1.0], [0, 0, 1]])
    d = np.full((1, 3, 4), 2.0, np.float32)
    p = np.ones((1, 3, 4), np.float32)
    ref = NR.reference_normals(d, p, cam)
    assert ref["has"].all() and NR.angle_deg(ref["normals"], np.array([0, 0, -1.0])).max() < 1e-9
    p2 = p.copy()
    p2[0, 1, 0] = p2[0, 1, 2] = 0.3                       # (1, 1) loses both horizontal neighbours
    ref = NR.reference_normals(d, p2, cam)
    assert not ref["has"][0, 1, 1] and not ref["has"][0, 1, 0] and not ref["has"][0, 1, 3] and ref["has"][0, 0, 1]
    d3 = d.copy()
    d3[0, :, 2:] = 2.0 * 1.0499                           # under the 5 % limit: the tangent crosses the jump
    under = NR.reference_normals(d3, p, cam)
    d3[0, :, 2:] = 2.0 * 1.0501                           # over it: columns 0 and 1 take one-sided differences and are flat again
    over = NR.reference_normals(d3, p, cam)
    assert NR.angle_deg(under["normals"][0, 1, 1], np.array([0, 0, -1.0])) > 10
    assert over["has"].all() and NR.angle_deg(over["normals"][0, :, :2], np.array([0, 0, -1.0])).max() < 1e-9
    # the limit is relative to the pixel's own depth: seen from the far side the same jump is 4.8 %, still usable
    assert NR.angle_deg(over["normals"][0, 1, 2], np.array([0, 0, -1.0])) > 10
    assert under["margin"][0, 1, 1] < 3e-3 and over["margin"][0, 1, 1] < 3e-3


def test_float32_evaluation_gives_the_gpu_tests_bound():
    """The constant of tests/test_gpu_normals.py is the worst angle between the float32 and the float64 evaluation of the
    reference on the four scenes (rounded up to two digits)."""
    worst = 0.0
    for name in G.SCENES:
        s = G._scene(name)
        r64 = NR.reference_normals(s["depths"], s["probs"], s["cams"])
        r32 = NR.reference_normals(s["depths"], s["probs"], s["cams"], dtype=np.float32)
        assert r32["normals"].dtype == np.float32 and np.array_equal(r32["has"], r64["has"])
        worst = max(worst, NR.angle_deg(r32["normals"][r64["has"]], r64["normals"][r64["has"]]).max())
    print("worst float32 - float64 angle: %.4e degrees" % worst)
    assert 0.95 * G.FLOAT32_WORST_DEG <= worst <= G.FLOAT32_WORST_DEG
    assert G.ANGLE_BOUND_DEG == 4 * G.FLOAT32_WORST_DEG


def test_reference_fusion_with_threshold_off_is_the_plain_reference():
    from tests import fusion_reference as FR
    s = G._scene("sphere")
    a = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, dedupe=True)
    b = NR.reference_fusion_normals(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, dedupe=True)
    for k in ("xyz", "rgb", "view_index", "pixel", "keep", "count"):
        assert np.array_equal(a[k], b[k])
    assert (b["margin"] <= a["margin"]).all()
    length = np.linalg.norm(b["normals"], axis=1)
    assert ((np.abs(length - 1) < 1e-12) | (length == 0)).all()


def test_ply_with_normals_round_trip(tmp_path):
    rs = np.random.RandomState(0)
    xyz, nrm = rs.randn(7, 3).astype(np.float32), rs.randn(7, 3).astype(np.float32)
    rgb = rs.randint(0, 256, (7, 3)).astype(np.uint8)
    path = str(tmp_path / "n.ply")
    F.write_ply(path, xyz, rgb, normals=nrm)
    data = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
              "property uchar blue\nend_header\n").encode("ascii")
    assert data.startswith(header) and len(data) == len(header) + 7 * 27
    rec = data[len(header) + 27 * 3:len(header) + 27 * 4]
    assert rec == xyz[3].astype("<f4").tobytes() + nrm[3].astype("<f4").tobytes() + rgb[3].tobytes()
    x2, c2, n2 = read_ply_normals(path)
    assert x2.dtype == np.float32 and c2.dtype == np.uint8 and n2.dtype == np.float32
    assert np.array_equal(x2, xyz) and np.array_equal(c2, rgb) and np.array_equal(n2, nrm)
    # the general reader of the evaluation takes the new file
    x3, c3 = E.read_ply_points(path)
    assert np.array_equal(x3, xyz) and np.array_equal(c3, rgb)
    # read_ply stays strict: it reads today's files only, and those are unchanged
    with pytest.raises(ValueError):
        F.read_ply(path)
    plain = str(tmp_path / "p.ply")
    F.write_ply(plain, xyz, rgb)
    assert os.path.getsize(plain) == len(F.PLY_HEADER % 7) + 7 * 15
    out = F.read_ply(plain)
    assert len(out) == 2 and np.array_equal(out[0], xyz) and np.array_equal(out[1], rgb)
    with pytest.raises(ValueError):
        read_ply_normals(plain)
    with pytest.raises(ValueError):
        F.write_ply(path, xyz, rgb, normals=nrm[:5])


@pytest.mark.parametrize("flags", [["--normals"], ["--normal_angle_threshold", "30"], ["--jump_threshold", "0.1"],
                                   ["--write_normal_maps"]])
def test_cli_normal_flags_need_fusion_hip(tmp_path, flags):
    for fusion in ([], ["--fusion", "fusibile"]):
        with pytest.raises(SystemExit) as e:
            DF.main(["--dense_folder", str(tmp_path)] + fusion + flags)
        assert flags[0] in str(e.value) and "--fusion hip" in str(e.value)
    assert not os.path.exists(str(tmp_path / "points_mvsnet"))


@pytest.mark.parametrize("flags", [["--normal_angle_threshold", "0"], ["--normal_angle_threshold", "181"],
                                   ["--normal_angle_threshold", "nan"], ["--jump_threshold", "-1"]])
def test_cli_rejects_bad_normal_values_before_any_work(tmp_path, flags):
    with pytest.raises(SystemExit) as e:
        DF.main(["--dense_folder", str(tmp_path), "--fusion", "hip"] + flags)
    assert flags[0][2:] in str(e.value)
    assert not os.path.exists(str(tmp_path / "points_mvsnet"))


def test_value_errors_come_before_gpu_work():
    s = G._scene("kat")
    for bad in (0, -10, 180.5, float("nan")):
        with pytest.raises(ValueError):
            F.FusionPlan(s["depths"], s["probs"], s["cams"], normal_angle_threshold=bad)
        with pytest.raises(ValueError):
            F.fuse_depth_maps(s["depths"], s["probs"], s["cams"], normal_angle_threshold=bad)
    with pytest.raises(ValueError):
        F.FusionPlan(s["depths"], s["probs"], s["cams"], normals=True, jump_threshold=-0.1)
    with pytest.raises(ValueError):
        estimate_normals(s["depths"], s["probs"], s["cams"], frame="object")
    with pytest.raises(ValueError):
        estimate_normals(s["depths"], s["probs"], s["cams"], jump_threshold=float("nan"))
    with pytest.raises(ValueError):
        estimate_normals([s["depths"][0], s["depths"][1][:, :5]], s["probs"], s["cams"])
    assert F.normal_cos_threshold(None) == -1.0
    assert -1.0 < F.normal_cos_threshold(180) < -0.9999999 and abs(F.normal_cos_threshold(60) - 0.5) < 1e-7
