"""GPU tests of the depth-map fusion (csrc/fusion.hip through mvsnet_amd.fusion) against the float64 reference of
tests/fusion_reference.py on analytic scenes, plus source lists, reproducibility, graph capture and the CLI route."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import fusion_reference as FR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 99.9 % of pixels clear a margin of 1e-4 on these scenes (plane / step 5 views, sphere 4 views at 40 x 48)
SCENES = {"plane": dict(kind="plane", V=5), "step": dict(kind="step", V=5), "sphere": dict(kind="sphere", V=4),
          "kat": dict(kind="plane", V=5, H=24, W=40, layout="line", f=64.0)}


def _scene(name, **kw):
    args = dict(H=40, W=48, low_prob_fraction=0.05, image_scale=2, seed=7)
    args.update(SCENES[name])
    args.update(kw)
    return FR.make_scene(**args)


def _run(s, with_pixels=True, **kw):
    from mvsnet_amd import fusion as F
    plan = F.FusionPlan(s["depths"], s["probs"], s["cams"], s["images"], **kw)
    plan.enqueue()
    return plan.result(with_pixels=with_pixels)


def _compare_exact_where_margin(s, ref, got, H, W):
    xyz, rgb, view, pix = got
    V = s["depths"].shape[0]
    key = view.astype(np.int64) * H * W + pix
    assert (np.diff(key) > 0).all()                                    # view ascending, row-major
    dev_keep = np.zeros(V * H * W, bool)
    dev_keep[key] = True
    ref_keep = ref["keep"].reshape(-1)
    clear = ref["margin"].reshape(-1) > 1e-4
    assert clear.mean() >= 0.999, clear.mean()
    assert np.array_equal(dev_keep[clear], ref_keep[clear])
    # points kept by both: position within 1e-5 x depth (where every decision was clear), colour and view exact
    ref_key = ref["view_index"].astype(np.int64) * H * W + ref["pixel"]
    common, gi, ri = np.intersect1d(key, ref_key, return_indices=True)
    c = clear[common]
    depth = s["depths"].reshape(-1)[common].astype(np.float64)
    err = np.abs(xyz[gi].astype(np.float64) - ref["xyz"][ri]).max(axis=1)
    assert (err[c] <= 1e-5 * depth[c]).all(), (err[c] / depth[c]).max()
    assert np.array_equal(rgb[gi], ref["rgb"][ri]) and np.array_equal(view[gi], ref["view_index"][ri])


@pytest.mark.parametrize("name", ["kat", "plane", "step", "sphere"])
def test_device_matches_reference_without_dedupe(name):
    s = _scene(name)
    V, H, W = s["depths"].shape
    for N in (1, 3):
        ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=N, dedupe=False)
        got = _run(s, num_consistent=N, dedupe=False)
        assert len(got[0]) > 0.3 * V * H * W
        _compare_exact_where_margin(s, ref, got, H, W)


def test_device_corrupted_view_and_looser_thresholds():
    s = _scene("sphere", V=5, corrupt_fraction=0.3, corrupt_view=2)
    V, H, W = s["depths"].shape
    ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, reproj_threshold=1.5,
                              depth_rel_threshold=0.02, prob_threshold=0.5, dedupe=False)
    got = _run(s, num_consistent=2, reproj_threshold=1.5, depth_rel_threshold=0.02, prob_threshold=0.5, dedupe=False)
    xyz, rgb, view, pix = got
    key = view.astype(np.int64) * H * W + pix
    dev_keep = np.zeros(V * H * W, bool)
    dev_keep[key] = True
    clear = ref["margin"].reshape(-1) > 1e-4
    assert np.array_equal(dev_keep[clear], ref["keep"].reshape(-1)[clear])
    assert not dev_keep.reshape(V, H, W)[2][s["corrupt"]].any()


@pytest.mark.parametrize("name", ["kat", "step"])
def test_device_dedupe_exact_on_kats(name):
    s = _scene(name, low_prob_fraction=0.0) if name == "kat" else _scene("step", layout="line", f=64.0, H=24, W=40,
                                                                             low_prob_fraction=0.0)
    V, H, W = s["depths"].shape
    for N in (2, 3):
        ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=N, dedupe=True)
        xyz, rgb, view, pix = _run(s, num_consistent=N, dedupe=True)
        assert np.array_equal(view, ref["view_index"]) and np.array_equal(pix, ref["pixel"])
        assert np.array_equal(rgb, ref["rgb"])
        depth = s["depths"].reshape(-1)[view.astype(np.int64) * H * W + pix].astype(np.float64)
        assert (np.abs(xyz - ref["xyz"]).max(axis=1) <= 1e-5 * depth).all()
        if name == "kat":
            assert len(xyz) == FR.plane_kat_counts(V, H, W, 4, N)[1]


def test_device_dedupe_sphere_count_and_surface():
    s = _scene("sphere", V=5, low_prob_fraction=0.0)
    ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, dedupe=True)
    xyz, rgb, view, pix = _run(s, num_consistent=2, dedupe=True)
    assert abs(len(xyz) - len(ref["xyz"])) <= 0.001 * len(ref["xyz"])
    nodedupe = _run(s, num_consistent=2, dedupe=False)
    assert len(xyz) < 0.6 * len(nodedupe[0])                           # union, not sum
    depth = np.array([FR._project(s["cams"][v], x[None].astype(np.float64))[0, 2] for v, x in zip(view, xyz)])
    assert (s["surface_distance"](xyz) <= 1e-3 * depth).all()


def test_device_explicit_source_lists():
    s = _scene("plane")
    V, H, W = s["depths"].shape
    sources = [[1, 2], [0], [4, 3, 1, 1], [], [0, 1, 2, 3]]
    for dedupe in (False, True):
        ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=1, sources=sources,
                                  dedupe=dedupe)
        got = _run(s, num_consistent=1, sources=sources, dedupe=dedupe)
        if not dedupe:
            _compare_exact_where_margin(s, ref, got, H, W)
        else:
            assert abs(len(got[0]) - len(ref["xyz"])) <= 0.001 * len(ref["xyz"])
        assert not (got[2] == 3).any()                                 # view 3 has no sources


# V x H x W with V*H*W = one pixel; one below, exactly and one above a compaction block of 1024 pixels; and 263 blocks, past the
# 256 block counts that the single-workgroup scan takes per round
COMPACTION_SHAPES = {1: (1, 1, 1), 1023: (3, 11, 31), 1024: (2, 16, 32), 1025: (5, 5, 41), 268800: (5, 240, 224)}


@pytest.mark.parametrize("pixels", sorted(COMPACTION_SHAPES))
def test_compaction_at_block_boundaries(pixels):
    """With num_consistent = 0 a pixel is kept exactly when it is valid, whatever its sources say, so the probabilities place
    the survivors: the first and the last pixel, about 30 % of the rest, and (263 blocks) none in blocks 1, 100 and 261."""
    V, H, W = COMPACTION_SHAPES[pixels]
    s = FR.make_scene(kind="plane", V=V, H=H, W=W, layout="line", f=64.0, seed=pixels)
    keep = np.random.RandomState(pixels).rand(pixels) < 0.3
    keep[0] = keep[-1] = True
    blocks = -(-pixels // 1024)
    for b in ((1, 100, blocks - 2) if blocks > 3 else ()):
        keep[b * 1024:(b + 1) * 1024] = False
    s["probs"] = np.where(keep, 1.0, 0.3).astype(np.float32).reshape(V, H, W)
    ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=0, dedupe=False)
    assert np.array_equal(ref["keep"].reshape(-1), keep)
    got = _run(s, num_consistent=0, dedupe=False)
    assert np.array_equal(got[2].astype(np.int64) * H * W + got[3], np.nonzero(keep)[0])
    _compare_exact_where_margin(s, ref, got, H, W)


def test_reproducible_bytes(tmp_path):
    from mvsnet_amd import fusion as F
    s = _scene("sphere", V=6, H=64, W=80)
    for dedupe in (True, False):
        paths = []
        for k in range(2):
            xyz, rgb, _ = F.fuse_depth_maps(s["depths"], s["probs"], s["cams"], s["images"], dedupe=dedupe, num_consistent=2)
            paths.append(str(tmp_path / ("%d_%d.ply" % (dedupe, k))))
            F.write_ply(paths[-1], xyz, rgb)
        assert open(paths[0], "rb").read() == open(paths[1], "rb").read()


def test_graph_capture_replays_eager_result():
    import torch
    from mvsnet_amd import fusion as F
    s = _scene("sphere", V=5)
    for dedupe in (True, False):
        plan = F.FusionPlan(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=2, dedupe=dedupe)
        plan.enqueue()
        eager = plan.result(with_pixels=True)
        # every output overwritten with values the replay has to replace: a stale buffer cannot pass
        n = len(eager[0])
        plan.xyz.fill_(float("nan"))
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
        replay = plan.result(with_pixels=True)
        for a, b in zip(eager, replay):
            assert a.tobytes() == b.tobytes()


def _write_dense(folder, s):
    from mvsnet_amd import predictlib
    out = os.path.join(folder, "depths_mvsnet")
    os.makedirs(out)
    for i in range(s["depths"].shape[0]):
        predictlib.write_output_slice(out, s["depths"][i], s["probs"][i], s["images"][i][:, :, ::-1], s["cams"][i], i)


def _cli(dense, *extra):
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "mvsnet_amd.depthfusion", "--dense_folder", dense,
                        "--fusion", "hip"] + list(extra), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    found = [os.path.join(b, f) for b, _, fs in os.walk(os.path.join(dense, "points_mvsnet")) for f in fs
             if f == "final3d_model.ply"]
    assert len(found) == 1 and os.path.basename(os.path.dirname(found[0])).startswith("consistencyCheck-")
    return found[0]


def test_cli_end_to_end_matches_library(tmp_path):
    from mvsnet_amd import depthfusion as DF, fusion as F, preprocess as pp
    s = _scene("sphere", V=5, image_scale=1)
    dense = str(tmp_path / "hip")
    _write_dense(dense, s)
    shutil.copytree(dense, str(tmp_path / "fusibile"))
    ply = _cli(dense, "--num_consistent", "2")
    idx, d, p, c, im = F.load_dense_folder(dense)
    xyz, rgb, _ = F.fuse_depth_maps(d, p, c, im, num_consistent=2)
    F.write_ply(str(tmp_path / "lib.ply"), xyz, rgb)
    assert len(xyz) > 1000
    assert open(ply, "rb").read() == open(str(tmp_path / "lib.ply"), "rb").read()
    DF.main(["--dense_folder", str(tmp_path / "fusibile")])
    for i in idx:
        a = open(os.path.join(dense, "depths_mvsnet", "%d_prob_filtered.pfm" % i), "rb").read()
        b = open(os.path.join(str(tmp_path / "fusibile"), "depths_mvsnet", "%d_prob_filtered.pfm" % i), "rb").read()
        assert a == b
    assert np.array_equal(pp.load_pfm(os.path.join(dense, "depths_mvsnet", "0_prob_filtered.pfm")),
                          np.where(s["probs"][0] < 0.8, 0, s["depths"][0]))


def test_cli_listed_sources(tmp_path):
    from mvsnet_amd import fusion as F
    s = _scene("plane", V=4, image_scale=1)
    listed = [[1, 2], [0, 3], [1], [0, 1, 2]]
    for kind in ("pair", "covis"):
        dense = str(tmp_path / kind)
        _write_dense(dense, s)
        if kind == "pair":
            with open(os.path.join(dense, "pair.txt"), "w") as f:
                f.write("4\n" + "".join("%d\n%d %s\n" % (r, len(l), " ".join("%d 1.0" % v for v in l)) for r, l in enumerate(listed)))
        else:
            with open(os.path.join(dense, "covisibility.json"), "w") as f:
                json.dump({str(r): {"views": l, "min_depth": 1, "max_depth": 9} for r, l in enumerate(listed)}, f)
        ply = _cli(dense, "--fusion_sources", "listed", "--num_consistent", "1", "--no_dedupe")
        idx, d, p, c, im = F.load_dense_folder(dense)
        assert F.listed_sources(dense, idx) == listed
        xyz, rgb, _ = F.fuse_depth_maps(d, p, c, im, num_consistent=1, sources=listed, dedupe=False)
        F.write_ply(str(tmp_path / "lib.ply"), xyz, rgb)
        assert open(ply, "rb").read() == open(str(tmp_path / "lib.ply"), "rb").read()
        every = F.fuse_depth_maps(d, p, c, im, num_consistent=1, dedupe=False)[0]
        assert len(every) != len(xyz)
