"""CPU tests of the depth-map fusion (mvsnet_amd/fusion.py): the float64 reference against hand-worked counts
and analytic scenes, the PLY bytes, the argument checks of the mvs_fusion_* entry points (no GPU call), host helpers, and
the depthfusion CLI's --fusion switch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_reference as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kat(V=5, H=24, W=40):
    # f = 64, b = 0.25, Z = 4: f b / Z = 4 pixels, every correspondence lands on a pixel centre
    return FR.make_scene("plane", V=V, H=H, W=W, layout="line", f=64.0, baseline=0.25)


def test_reference_plane_kat_counts_by_hand():
    s = _kat()
    V, H, W = s["depths"].shape
    for N in (1, 2, 3, 4):
        ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=N, dedupe=False)
        per_view, union = FR.plane_kat_counts(V, H, W, 4, N)
        assert ref["keep"].sum(axis=(1, 2)).tolist() == per_view
        assert len(ref["xyz"]) == sum(per_view)
        # every pixel whose correspondences all stay in the image is kept, at its exact plane point
        for i in range(V):
            inside = [x for x in range(W) if all(0 <= x + (i - j) * 4 < W for j in range(V))]
            assert ref["keep"][i][:, inside].all()
        np.testing.assert_allclose(ref["xyz"][:, 2], 4.0, rtol=1e-12)
        assert (ref["margin"] >= 0.25 - 1e-12).all()           # KAT: nothing near a threshold or a rounding boundary
        # de-duplication emits each surface pixel once: the union of the views, not their sum
        dd = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=N, dedupe=True)
        assert len(dd["xyz"]) == union < sum(per_view)
        g = np.round((dd["xyz"][:, 0] * 64.0 / 4.0)).astype(int) * 1000 + np.round(dd["xyz"][:, 1] * 16).astype(int)
        assert len(np.unique(g)) == len(g)                     # distinct world points


def test_reference_output_order_and_colours():
    s = FR.make_scene("step", V=4, H=20, W=24, image_scale=3, seed=2)
    ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=1, dedupe=False)
    key = ref["view_index"].astype(np.int64) * 20 * 24 + ref["pixel"]
    assert (np.diff(key) > 0).all()                            # view ascending, then row-major
    v, p = ref["view_index"], ref["pixel"]
    x, y = p % 24, p // 24
    assert np.array_equal(ref["rgb"], s["images"][v, (2 * y + 1) * 60 // 40, (2 * x + 1) * 72 // 48])


def test_reference_rejects_occluded_band():
    s = FR.make_scene("sphere", V=4, H=40, W=48)
    V = 4
    ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], num_consistent=V - 1, dedupe=False)
    # analytic visibility: a reference pixel's surface point is occluded in source s when s's ray-cast depth at its
    # projection is clearly in front of it
    occluded_any = np.zeros((V, 40, 48), bool)
    for r in range(V):
        yy, xx = np.mgrid[0:40, 0:48]
        d = s["depths"][r].astype(np.float64)
        X = FR._backproject(s["cams"][r], xx.reshape(-1), yy.reshape(-1), d.reshape(-1))
        for src in range(V):
            if src == r:
                continue
            u, v, w = FR._project(s["cams"][src], X).T
            qx, qy = np.floor(u / w + 0.5).astype(int), np.floor(v / w + 0.5).astype(int)
            ok = (qx >= 0) & (qx < 48) & (qy >= 0) & (qy < 40)
            ds = np.where(ok, s["depths"][src][np.clip(qy, 0, 39), np.clip(qx, 0, 47)], np.inf)
            occluded_any[r].reshape(-1)[:] |= ok & (ds < 0.9 * w)
    assert occluded_any.sum() > 50                              # the band exists
    assert not (ref["keep"] & occluded_any).any()               # and none of it is kept
    assert ref["keep"].sum() > 0.5 * (s["depths"] > 0).sum()


def test_reference_never_emits_corrupted_pixels():
    s = FR.make_scene("sphere", V=5, H=40, W=48, corrupt_fraction=0.3, corrupt_view=2, seed=3)
    assert s["corrupt"].sum() > 100
    for N in (2, 3, 4):
        for dedupe in (False, True):
            ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], num_consistent=N, dedupe=dedupe)
            assert not (ref["keep"][2] & s["corrupt"]).any()
            kept = ref["view_index"] == 2
            assert kept.any()


def test_reference_sources_and_probability_filter():
    s = FR.make_scene("plane", V=4, H=20, W=24, low_prob_fraction=0.2, seed=4)
    ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], num_consistent=1, dedupe=False, sources=[[1], [0], [], [3, 2]])
    assert not (ref["keep"] & (s["probs"] < 0.8)).any()
    assert not ref["keep"][2].any() and ref["keep"][3].any()    # view 2 has no sources; view 3's list reduces to [2]
    assert (ref["count"] <= 1).all()


def test_ply_bytes_and_round_trip(tmp_path):
    from mvsnet_amd import fusion as F
    rs = np.random.RandomState(0)
    xyz = rs.standard_normal((7, 3)).astype(np.float32)
    rgb = rs.randint(0, 256, (7, 3)).astype(np.uint8)
    path = str(tmp_path / "a.ply")
    F.write_ply(path, xyz, rgb)
    raw = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\n"
              b"property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert raw.startswith(header) and len(raw) == len(header) + 15 * 7
    assert raw[len(header):len(header) + 12] == xyz[0].astype("<f4").tobytes()
    assert raw[len(header) + 12:len(header) + 15] == rgb[0].tobytes()
    x2, c2 = F.read_ply(path)
    assert np.array_equal(x2, xyz) and np.array_equal(c2, rgb)
    F.write_ply(str(tmp_path / "e.ply"), np.zeros((0, 3)), np.zeros((0, 3)))
    assert F.read_ply(str(tmp_path / "e.ply"))[0].shape == (0, 3)


def test_camera_tables_compose_projection():
    from mvsnet_amd import fusion as F
    s = FR.make_scene("sphere", V=3, H=20, W=24)
    V = 3
    t = F.camera_tables(s["cams"]).astype(np.float64)
    M, B = t[:V * V * 12].reshape(V, V, 3, 4), t[V * V * 12:].reshape(V, 3, 4)
    x, y, d = 5.0, 7.0, 3.7
    a = np.array([x * d, y * d, d, 1.0])
    X = FR._backproject(s["cams"][0], np.array([x]), np.array([y]), np.array([d]))[0]
    np.testing.assert_allclose(B[0] @ a, X, rtol=1e-6)
    np.testing.assert_allclose(M[0, 2] @ a, FR._project(s["cams"][2], X[None])[0], rtol=1e-6)


def test_source_lists_and_shape_checks():
    from mvsnet_amd import fusion as F
    assert F.source_lists(3) == [[1, 2], [0, 2], [0, 1]]
    assert F.source_lists(3, [[2, 1, 1, 0], [], [0]]) == [[1, 2], [], [0]]
    with pytest.raises(ValueError):
        F.source_lists(3, [[1], [0]])
    with pytest.raises(ValueError):
        F.source_lists(2, [[5], [0]])
    d = [np.ones((4, 5), np.float32), np.ones((4, 6), np.float32)]
    with pytest.raises(ValueError, match="one size"):
        F.fuse_depth_maps(d, d, np.zeros((2, 2, 4, 4)))


def test_fusion_entry_points_check_arguments_without_gpu(lib_built):
    from mvsnet_amd import _lib
    h = _lib.load()
    BADARG, SHAPE = -1, -2
    assert h.mvs_fusion_workspace_bytes(4, 20, 24, 3, 1) > h.mvs_fusion_workspace_bytes(4, 20, 24, 3, 0) > 0
    assert h.mvs_fusion_workspace_bytes(0, 20, 24, 3, 1) == 0
    assert h.mvs_fusion_workspace_bytes(70000, 20, 24, 3, 1) == 0
    nz = ctypes_ptr = 4096                     # never dereferenced: the checks return before any HIP call
    args = lambda **kw: [kw.get("depth", nz), kw.get("prob", nz), kw.get("V", 4), kw.get("H", 20), kw.get("W", 24), nz, nz, nz,
                         kw.get("ms", 3), 0.8, kw.get("reproj", 1.0), 0.01, 3.0, 1, kw.get("img", None), kw.get("ih", 0),
                         kw.get("iw", 0), nz, nz, nz, None, nz, kw.get("ws", nz), 1 << 20, None]
    assert h.mvs_fusion_f32(*args(depth=None)) == BADARG
    assert h.mvs_fusion_f32(*args(ws=None)) == BADARG
    assert h.mvs_fusion_f32(*args(V=0)) == BADARG
    assert h.mvs_fusion_f32(*args(W=-3)) == BADARG
    assert h.mvs_fusion_f32(*args(ms=-1)) == BADARG
    assert h.mvs_fusion_f32(*args(reproj=0.0)) == BADARG
    assert h.mvs_fusion_f32(*args(img=ctypes_ptr, ih=0, iw=10)) == BADARG
    assert h.mvs_fusion_f32(*args(V=70000)) == SHAPE
    assert h.mvs_fusion_f32(*args(V=60000, H=200, W=200)) == SHAPE     # V*H*W beyond int32 indices


def _dense_folder(tmp_path, V=3, H=12, W=16):
    from PIL import Image
    from mvsnet_amd import preprocess as pp
    s = FR.make_scene("plane", V=V, H=H, W=W, low_prob_fraction=0.3, seed=5)
    dense = str(tmp_path / "dense")
    out = os.path.join(dense, "depths_mvsnet")
    os.makedirs(out)
    for i in range(V):
        pp.write_pfm(os.path.join(out, "%d_init.pfm" % i), s["depths"][i])
        pp.write_pfm(os.path.join(out, "%d_prob.pfm" % i), s["probs"][i])
        cam = s["cams"][i].copy()
        pp.write_cam(os.path.join(out, "%d.txt" % i), cam)
        Image.fromarray(s["images"][i]).save(os.path.join(out, "%d.jpg" % i))
    return dense, s


def _tree(folder):
    out = {}
    for base, _, files in os.walk(folder):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, folder)] = open(p, "rb").read()
    return out


def test_cli_default_is_fusibile_and_hand_off_unchanged(tmp_path):
    from mvsnet_amd import depthfusion as DF
    dense, _ = _dense_folder(tmp_path)
    DF.main(["--dense_folder", dense])
    default = _tree(dense)
    assert "points_mvsnet/2333__0/disp.dmb" in default and not any("consistencyCheck" in k for k in default)
    # the same run through the pre-existing steps, called one by one, gives the same bytes
    dense2, _ = _dense_folder(tmp_path / "b")
    pf = os.path.join(dense2, "points_mvsnet")
    os.makedirs(pf)
    DF.probability_filter(dense2, 0.8)
    DF.mvsnet_to_gipuma(dense2, pf)
    assert _tree(dense2) == default
    DF.main(["--dense_folder", dense, "--fusion", "fusibile"])
    assert _tree(dense) == default


def test_load_dense_folder_and_listed_sources(tmp_path):
    import json
    from mvsnet_amd import fusion as F
    dense, s = _dense_folder(tmp_path, V=3)
    idx, d, p, c, im = F.load_dense_folder(dense)
    assert idx == [0, 1, 2] and np.array_equal(d, s["depths"]) and np.array_equal(p, s["probs"])
    np.testing.assert_allclose(c, s["cams"], rtol=1e-6, atol=1e-9)
    assert im.shape == (3, 12, 16, 3) and im.dtype == np.uint8
    with pytest.raises(FileNotFoundError):
        F.listed_sources(dense, idx)
    with open(os.path.join(dense, "pair.txt"), "w") as f:
        f.write("3\n0\n2 1 10.0 2 5.0\n1\n1 0 3.0\n2\n0\n")
    assert F.listed_sources(dense, idx) == [[1, 2], [0], []]
    with open(os.path.join(dense, "covisibility.json"), "w") as f:
        json.dump({"0": {"views": [2, 7]}, "1": {"views": []}, "2": {"views": [1, 0]}}, f)
    # both files: covisibility.json, the precedence of mvs_data_generation.make_generator (the neighbours of inference)
    assert F.listed_sources(dense, idx) == [[2], [], [1, 0]]


def test_cli_hip_without_gpu_fails_clearly(tmp_path):
    dense, _ = _dense_folder(tmp_path)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-m", "mvsnet_amd.depthfusion", "--dense_folder", dense, "--fusion", "hip"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--fusion hip needs a GPU" in r.stderr and "Traceback" not in r.stderr
    assert not os.path.isdir(os.path.join(dense, "points_mvsnet"))
