"""GPU tests of the normal estimation and of the fusion with normals (csrc/fusion.hip through mvsnet_amd.fusion) against the
float64 reference of tests/normals_reference.py, on the scenes of tests/test_gpu_fusion.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_reference as FR
from tests import normals_reference as NR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCENES = {"plane": dict(kind="plane", V=5), "step": dict(kind="step", V=5), "sphere": dict(kind="sphere", V=4),
          "kat": dict(kind="plane", V=5, H=24, W=40, layout="line", f=64.0)}

# Worst angle, in degrees, between the float32 numpy evaluation of the reference formula (NR.reference_normals with
# dtype=np.float32) and its float64 evaluation over the four scenes above: measured 8.366e-5 (on the sphere; plane 2.8e-5,
# step 2.3e-5, kat 0), rounded up.  tests/test_normals_host.py re-measures it on every run.  The device may be FACTOR = 4
# times as far from the float64 reference: it evaluates the same formula in float32, in another order and with fused
# multiply-adds.
FLOAT32_WORST_DEG = 8.4e-5
ANGLE_BOUND_DEG = 4 * FLOAT32_WORST_DEG


@functools.lru_cache(maxsize=None)
def _scene_cached(name, kw):
    args = dict(H=40, W=48, low_prob_fraction=0.05, image_scale=2, seed=7)
    args.update(SCENES[name])
    args.update(dict(kw))
    return FR.make_scene(**args)


def _scene(name, **kw):
    """The cached scene: tests must not modify its arrays."""
    return _scene_cached(name, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def _ref_normals(name):
    s = _scene(name)
    return NR.reference_normals(s["depths"], s["probs"], s["cams"])


@functools.lru_cache(maxsize=None)
def _noisy_sphere():
    s = dict(_scene("sphere"))
    d = s["depths"].copy()
    H, W = d.shape[1:]
    d[1] = (d[1] * (1 + 0.002 * np.random.RandomState(3).randn(H, W))).astype(np.float32)
    s["depths"] = d
    return s


def _plan(s, **kw):
    from mvsnet_amd import fusion as F
    plan = F.FusionPlan(s["depths"], s["probs"], s["cams"], s["images"], **kw)
    plan.enqueue()
    return plan


def _valid(s):
    return (s["depths"] > 0) & np.isfinite(s["depths"]) & (s["probs"] >= 0.8)


@pytest.mark.parametrize("name", ["kat", "plane", "step", "sphere"])
def test_normal_maps_match_reference(name):
    from mvsnet_amd import fusion as F
    s, ref = _scene(name), _ref_normals(name)
    got = F.estimate_normals(s["depths"], s["probs"], s["cams"])
    assert got.shape == s["depths"].shape + (3,) and got.dtype == np.float32
    valid = _valid(s)
    clear = ref["margin"] > 1e-4
    print(name, "clear share of valid pixels %.5f, smallest margin %.4g" % (clear[valid].mean(), ref["margin"][valid].min()))
    assert clear[valid].mean() >= 0.999
    has = (got != 0).any(-1)
    assert not has[~valid].any()
    assert np.array_equal(has[clear], ref["has"][clear])
    both = has & ref["has"] & clear
    assert both.sum() >= 0.95 * valid.sum()
    ang = NR.angle_deg(got[both], ref["normals"][both])
    length = np.linalg.norm(got[both].astype(np.float64), axis=1)
    print(name, "worst angle to the reference %.3e degrees (bound %.3e), |n| - 1 within %.2e" %
          (ang.max(), ANGLE_BOUND_DEG, np.abs(length - 1).max()))
    assert ang.max() <= ANGLE_BOUND_DEG, ang.max()
    assert np.abs(length - 1).max() <= 3e-7                                  # three float32 roundings of a unit vector
    # camera frame: R_v n
    cam = F.estimate_normals(s["depths"], s["probs"], s["cams"], frame="camera")
    want = np.einsum("vij,vhwj->vhwi", s["cams"][:, 0, :3, :3], got.astype(np.float64))
    assert cam.dtype == np.float32 and np.abs(cam - want).max() <= 1e-7
    assert np.array_equal((cam != 0).any(-1), has)
    if name == "kat":                                                           # R = identity: facing the camera is z < 0
        assert (cam[has][:, 2] < 0).all()


def test_normal_maps_take_device_tensors_and_lists():
    import torch
    from mvsnet_amd import fusion as F
    s = _scene("sphere")
    a = F.estimate_normals(s["depths"], s["probs"], s["cams"], jump_threshold=0.02, prob_threshold=0.2)
    b = F.estimate_normals(torch.as_tensor(s["depths"]).cuda(), [torch.as_tensor(p).cuda() for p in s["probs"]], s["cams"],
                           jump_threshold=0.02, prob_threshold=0.2)
    assert a.tobytes() == b.tobytes()
    ref = NR.reference_normals(s["depths"], s["probs"], s["cams"], prob_threshold=0.2, jump_threshold=0.02)
    clear = ref["margin"] > 1e-4
    assert np.array_equal((a != 0).any(-1)[clear], ref["has"][clear])
    assert ref["has"].sum() != _ref_normals("sphere")["has"].sum()             # the thresholds were used


@pytest.mark.parametrize("shape", [(1, 5), (5, 1)])
def test_degenerate_sizes_have_no_normals(shape):
    from mvsnet_amd import fusion as F
    H, W = shape
    s = FR.make_scene("plane", V=3, H=H, W=W, seed=7, image_scale=2)
    n = F.estimate_normals(s["depths"], s["probs"], s["cams"])
    assert n.shape == (3, H, W, 3) and not n.any()
    plain = _plan(s, num_consistent=1, dedupe=False).result(with_pixels=True)
    with_n = _plan(s, num_consistent=1, dedupe=False, normals=True).result(with_pixels=True, with_normals=True)
    assert len(plain[0]) > 0
    for a, b in zip(plain, with_n[:4]):
        assert a.tobytes() == b.tobytes()
    assert with_n[4].shape == (len(plain[0]), 3) and not with_n[4].any()
    # with a threshold no pixel is valid
    assert len(_plan(s, num_consistent=0, dedupe=False, normal_angle_threshold=90).result()[0]) == 0
    assert len(_plan(s, num_consistent=0, dedupe=False).result()[0]) == int(_valid(s).sum())


def _compare_fused_normals(s, ref, got):
    """got: result(with_pixels=True, with_normals=True).  Points kept by both, where every decision was clear: zero normals
    coincide and the others lie within the bound."""
    V, H, W = s["depths"].shape
    xyz, rgb, view, pix, nrm = got
    key = view.astype(np.int64) * H * W + pix
    ref_key = ref["view_index"].astype(np.int64) * H * W + ref["pixel"]
    common, gi, ri = np.intersect1d(key, ref_key, return_indices=True)
    c = (ref["margin"].reshape(-1) > 1e-4)[common]
    assert c.sum() >= 0.99 * len(ref_key)
    g, r = nrm[gi][c], ref["normals"][ri][c]
    gz, rz = ~g.any(1), ~r.any(1)
    assert np.array_equal(gz, rz)
    ang = NR.angle_deg(g[~gz], r[~rz])
    length = np.linalg.norm(g[~gz].astype(np.float64), axis=1)
    print("fused normals: %d compared, %d zero, worst angle %.3e degrees (bound %.3e)" % (len(g), gz.sum(), ang.max(), ANGLE_BOUND_DEG))
    assert ang.max() <= ANGLE_BOUND_DEG, ang.max()
    assert np.abs(length - 1).max() <= 3e-7
    return int(gz.sum())


@pytest.mark.parametrize("name", ["kat", "plane", "step", "sphere"])
def test_fusion_threshold_off_is_todays_fusion_plus_normals(name):
    s = _scene(name)
    V, H, W = s["depths"].shape
    for N in (1, 3):
        plain = _plan(s, num_consistent=N, dedupe=False).result(with_pixels=True)
        got = _plan(s, num_consistent=N, dedupe=False, normals=True).result(with_pixels=True, with_normals=True)
        assert len(got) == 5 and len(plain[0]) > 0.3 * V * H * W
        for a, b in zip(plain, got[:4]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        ref = NR.reference_fusion_normals(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=N, dedupe=False)
        _compare_fused_normals(s, ref, got)


def test_fusion_kept_points_without_a_normal():
    s = _scene("sphere")
    ref = NR.reference_fusion_normals(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, dedupe=False)
    assert int((~ref["normals"].any(1)).sum()) == 29
    got = _plan(s, num_consistent=2, dedupe=False, normals=True).result(with_pixels=True, with_normals=True)
    zeros = _compare_fused_normals(s, ref, got)
    assert 0 < zeros <= 29


def test_fusion_with_normal_angle_threshold():
    s = _noisy_sphere()
    V, H, W = s["depths"].shape
    kw = dict(num_consistent=2, dedupe=False)
    ref = NR.reference_fusion_normals(s["depths"], s["probs"], s["cams"], s["images"], normal_angle_threshold=10, **kw)
    assert ref["rejected_pairs"] == 440 and ref["geometric_pairs"] == 18211 and len(ref["xyz"]) == 6234
    plan = _plan(s, normal_angle_threshold=10, **kw)
    assert plan.normals                                                         # implied by the threshold
    got = plan.result(with_pixels=True, with_normals=True)
    off = _plan(s, normals=True, **kw).result()
    print("kept with the threshold %d (reference %d), without %d" % (len(got[0]), len(ref["xyz"]), len(off[0])))
    assert len(got[0]) != len(off[0]) and len(got[0]) < len(off[0])
    key = got[2].astype(np.int64) * H * W + got[3]
    assert (np.diff(key) > 0).all()
    dev_keep = np.zeros(V * H * W, bool)
    dev_keep[key] = True
    clear = ref["margin"].reshape(-1) > 1e-4
    print("clear share of valid pixels %.5f" % clear[_valid(s).reshape(-1)].mean())
    assert clear[_valid(s).reshape(-1)].mean() >= 0.995
    assert np.array_equal(dev_keep[clear], ref["keep"].reshape(-1)[clear])
    assert got[4].any(1).all()                                                  # no kept point has a zero normal
    assert _compare_fused_normals(s, ref, got) == 0


def test_dedupe_with_normals_on_kat():
    s = _scene("kat", low_prob_fraction=0.0)
    V, H, W = s["depths"].shape
    for N in (2, 3):
        ref = NR.reference_fusion_normals(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=N, dedupe=True)
        xyz, rgb, view, pix, nrm = _plan(s, num_consistent=N, dedupe=True, normals=True).result(with_pixels=True, with_normals=True)
        assert np.array_equal(view, ref["view_index"]) and np.array_equal(pix, ref["pixel"])
        assert len(xyz) == FR.plane_kat_counts(V, H, W, 4, N)[1]
        ang = NR.angle_deg(nrm, np.array([0.0, 0.0, -1.0]))
        assert ang.max() <= ANGLE_BOUND_DEG, ang.max()
        plain = _plan(s, num_consistent=N, dedupe=True).result(with_pixels=True)
        for a, b in zip(plain, (xyz, rgb, view, pix)):
            assert a.tobytes() == b.tobytes()


def test_reproducible_ply_bytes_with_normals(tmp_path):
    from mvsnet_amd import fusion as F
    s = _scene("sphere", V=6, H=64, W=80)
    for dedupe in (True, False):
        paths = []
        for k in range(2):
            xyz, rgb, _, nrm = F.fuse_depth_maps(s["depths"], s["probs"], s["cams"], s["images"], dedupe=dedupe, num_consistent=2,
                                                 normals=True)
            paths.append(str(tmp_path / ("%d_%d.ply" % (dedupe, k))))
            F.write_ply(paths[-1], xyz, rgb, nrm)
        data = open(paths[0], "rb").read()
        assert data == open(paths[1], "rb").read()
        x2, c2, n2 = F.read_ply_normals(paths[0])
        assert len(x2) > 1000 and n2.any(1).mean() > 0.9


def test_graph_capture_replays_eager_result_with_normals():
    import torch
    from mvsnet_amd import fusion as F
    s = _scene("sphere", V=5)
    for dedupe, thr in ((True, None), (False, 20.0)):
        plan = F.FusionPlan(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, dedupe=dedupe, normals=True,
                            normal_angle_threshold=thr)
        plan.enqueue()
        eager = plan.result(with_pixels=True, with_normals=True)
        # every output overwritten with values the replay has to replace: a stale buffer cannot pass
        n = len(eager[0])
        assert n > 1000
        plan.xyz.fill_(float("nan"))
        plan.nrm.fill_(float("nan"))
        plan.rgb[:n] = 255 - torch.as_tensor(eager[1]).to(plan.rgb.device)
        plan.view_index.fill_(-1)
        plan.pixel_index.fill_(-1)
        plan.count.zero_()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(g, stream=stream):
                plan.enqueue()
        g.replay()
        torch.cuda.synchronize()
        replay = plan.result(with_pixels=True, with_normals=True)
        assert len(replay) == 5
        for a, b in zip(eager, replay):
            assert a.tobytes() == b.tobytes()


def test_plan_interface_and_c_abi_errors():
    import torch
    from mvsnet_amd import _lib, fusion as F
    s = _scene("kat")
    plan = _plan(s, num_consistent=2)
    assert not plan.normals and plan.nrm is None and len(plan.result()) == 3
    with pytest.raises(ValueError):
        plan.result(with_normals=True)
    out = F.fuse_depth_maps(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, normals=True)
    assert len(out) == 4 and out[3].shape == out[0].shape and out[3].dtype == np.float32
    assert len(F.fuse_depth_maps(s["depths"], s["probs"], s["cams"], num_consistent=2, normal_angle_threshold=30)) == 4
    lib = _lib.load()
    p = _plan(s, num_consistent=2, normals=True)
    V, H, W = s["depths"].shape
    small = lib.mvs_fusion_workspace_bytes(V, H, W, p.max_sources, 1)
    assert lib.mvs_fusion_normals_workspace_bytes(V, H, W, p.max_sources, 1) > small
    assert lib.mvs_fusion_normals_workspace_bytes(0, H, W, p.max_sources, 1) == 0
    args = lambda nrm, wsb, cos: (_lib.ptr(p.depth), _lib.ptr(p.prob), V, H, W, _lib.ptr(p.tables), _lib.ptr(p.src_offsets),
                                  _lib.ptr(p.src_index), p.max_sources, 0.8, 1.0, 0.01, 2.0, 1, 0.05, cos, None, 0, 0, _lib.ptr(p.xyz),
                                  _lib.ptr(p.rgb), nrm, _lib.ptr(p.view_index), _lib.ptr(p.pixel_index), _lib.ptr(p.count),
                                  _lib.ptr(p.workspace), wsb, _lib.stream_ptr())
    assert lib.mvs_fusion_normals_f32(*args(None, p.workspace.numel(), -1.0)) == -1          # MVS_E_BADARG
    assert lib.mvs_fusion_normals_f32(*args(_lib.ptr(p.nrm), p.workspace.numel(), 1.0)) == -1
    assert lib.mvs_fusion_normals_f32(*args(_lib.ptr(p.nrm), small, -1.0)) == -3             # MVS_E_WORKSPACE
    assert lib.mvs_depth_normals_f32(_lib.ptr(p.depth), _lib.ptr(p.prob), V, H, W, _lib.ptr(p.tables), 0.8, 0.05, None,
                                     _lib.stream_ptr()) == -1
    torch.cuda.synchronize()


def _write_dense(folder, s):
    from mvsnet_amd import predictlib
    out = os.path.join(folder, "depths_mvsnet")
    os.makedirs(out)
    for i in range(s["depths"].shape[0]):
        predictlib.write_output_slice(out, s["depths"][i], s["probs"][i], s["images"][i][:, :, ::-1], s["cams"][i], i)


def test_cli_end_to_end_with_normals(tmp_path):
    from mvsnet_amd import fusion as F, preprocess as pp
    s = _scene("sphere", V=5, image_scale=1)
    dense = str(tmp_path / "hip")
    _write_dense(dense, s)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "mvsnet_amd.depthfusion", "--dense_folder", dense,
                        "--fusion", "hip", "--normals", "--num_consistent", "2", "--write_normal_maps"], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    found = [os.path.join(b, f) for b, _, fs in os.walk(os.path.join(dense, "points_mvsnet")) for f in fs
             if f == "final3d_model.ply"]
    assert len(found) == 1
    idx, d, p, c, im = F.load_dense_folder(dense)
    xyz, rgb, _, nrm = F.fuse_depth_maps(d, p, c, im, num_consistent=2, normals=True)
    F.write_ply(str(tmp_path / "lib.ply"), xyz, rgb, normals=nrm)
    assert len(xyz) > 1000 and nrm.any(1).mean() > 0.9
    assert open(found[0], "rb").read() == open(str(tmp_path / "lib.ply"), "rb").read()
    maps = F.estimate_normals(d, p, c, frame="camera")
    names = sorted(f for f in os.listdir(os.path.join(dense, "depths_mvsnet")) if f.endswith("_normal.pfm"))
    assert names == sorted("%d_normal.pfm" % i for i in idx)
    for k, i in enumerate(idx):
        m = pp.load_pfm(os.path.join(dense, "depths_mvsnet", "%d_normal.pfm" % i))
        assert m.shape == maps[k].shape and m.tobytes() == maps[k].tobytes()
