"""The files `compute_depth_maps` writes for a whole session, held to the float64 restatement of tests/session_reference.py
(oracle/mvsnet_oracle.py composed in numpy; it takes the decoded / resized / cropped uint8 images and the scaled cameras as
given and restates everything after them).  Unlike test_session_pipeline_equals_the_per_reference_view_calls, nothing of
the library is on the expected side: a mistake in the uint8 upload, the on-device standardisation, the per-image feature
cache, the grouped tower pass, the batched recurrent sweep, the refinement's guide image, the values read from the camera
row or the nearest-neighbour probability upsampling shows here as a number.

Every case writes a session, runs `compute_depth_maps` once, reads back EVERY <idx>_init.pfm / <idx>_prob.pfm and checks
that the other files agree with them (16-bit PNGs, camera, the exact set of indices).

Tolerances follow tests/test_gpu_full_size.py: multiples of what the float32 ORACLE lands at against the float64 oracle on
the same inputs, computed in the test (never from the library's output); every case prints measured value, floor and bound.
  * depth, unrefined: mean abs-rel <= 3 x the float32 oracle's; worst pixel < 1e-4;
  * refined depth (the seeded towers give residuals as large as the depth, the result crosses zero): the same two,
    normalised by the sweep's span (D-1) * interval: mean <= 3 x, worst pixel <= 10 x the float32 oracle's worst;
  * probability: |p - p64| > 1e-3 on at most 5e-4 of the pixels;
  * recurrent sweep: another winning plane on at most 0.5 % of the session's pixels (the float32 oracle: on none); on the
    agreeing pixels the probability as check_sweep of test_gpu_full_size.py: worst relative distance <= 2 x the float32
    oracle's own worst, 5e-5 on average.

The `unet` refinement tower halves its input four times, so the map it refines must have sides divisible by 16, in the
reference as here: the refinement cases run at 128 x 128 (32 x 32 at a quarter) on 132 x 132 images.

Measured on an MI355X (library / float32 oracle / bound) in the docstrings of the cases.  In every case the probability
map is off by more than 1e-3 on 0 pixels (worst 5.3e-6 .. 1.0e-5; float32 oracle 8.3e-6 .. 2.0e-5).
"""
import json
import os

import numpy as np
import pytest
import torch

from mvsnet_amd import predictlib as pl, preprocess as pp, synthetic as S
from tests import session_reference as R

pytestmark = pytest.mark.gpu
SUFFIXES = ("_init.pfm", "_prob.pfm", "_depth.png", "_prob.png", ".jpg", ".txt")


def write_session(path, size=(100, 132), n_images=7):
    return S.write_session(str(path), n_images=n_images, height=size[0], width=size[1], view_num=3, depth_num=24,
                           interval=10.0)


def config(sess, out, width=128, height=96, **kw):
    return pl.InferenceConfig(input_dir=sess, output_dir=str(out), view_num=3, max_d=24, width=width, height=height,
                              base_image_size=8, **kw)


def run_session(sess, cfg, extractor="hip", gru_views=4):
    """compute_depth_maps once -> ({index: (depth, prob) read back from the .pfm files}, float64 oracle, float32 oracle);
    the other files of every index are checked against the .pfm pair and the oracle's camera on the way."""
    from PIL import Image
    from mvsnet_amd.inference import build_weights, compute_depth_maps
    device = torch.device("cuda", 0)
    weights = build_weights(cfg, device, extractor=extractor)
    n = compute_depth_maps(sess, cfg, weights, device, gru_views=gru_views)
    params = R.make_params(cfg)                           # the seeded dictionaries build_weights made its weights from
    e64, e32 = R.expected_outputs(sess, cfg, params, np.float64), R.expected_outputs(sess, cfg, params, np.float32)
    assert n == len(e64)
    assert sorted(os.listdir(cfg.output_dir)) == sorted("%d%s" % (i, s_) for i in e64 for s_ in SUFFIXES)
    got = {}
    for i in sorted(e64):
        path = lambda s_: os.path.join(cfg.output_dir, "%d%s" % (i, s_))
        d, p = pp.load_pfm(path("_init.pfm")), pp.load_pfm(path("_prob.pfm"))
        assert d.dtype == np.float32 and d.shape == p.shape == e64[i]["depth"].shape == e64[i]["prob"].shape, (i, d.shape)
        assert np.isfinite(d).all() and np.isfinite(p).all()
        np.testing.assert_array_equal(np.asarray(Image.open(path("_depth.png"))), pp.depth_to_uint16(d))
        np.testing.assert_array_equal(np.asarray(Image.open(path("_prob.png"))), pp.confidence_to_uint16(p))
        np.testing.assert_array_equal(pp.load_cam(path(".txt")), e64[i]["cam"])
        with Image.open(path(".jpg")) as im:
            assert im.size == (d.shape[1], d.shape[0])
        got[i] = (d.astype(np.float64), p.astype(np.float64))
    return got, e64, e32


def pooled(fn, got, e64, e32):
    """fn(depth, prob, expectation) -> per-pixel array; evaluated for the library and for the float32 oracle, all views pooled."""
    lib = np.concatenate([np.ravel(fn(got[i][0], got[i][1], e64[i])) for i in sorted(e64)])
    flo = np.concatenate([np.ravel(fn(e32[i]["depth"].astype(np.float64), e32[i]["prob"].astype(np.float64), e64[i]))
                          for i in sorted(e64)])
    return lib, flo


def check_probability(tag, got, e64, e32):
    lib, flo = pooled(lambda d, p, e: np.abs(p - e["prob"]), got, e64, e32)
    share = float((lib > 1e-3).mean())
    print("%s: probability off by > 1e-3 on %.5f of %d pixels (bound 5e-4), worst %.3e (float32 oracle worst %.3e)"
          % (tag, share, lib.size, float(lib.max()), float(flo.max())))
    assert share <= 5e-4, share


def check_soft_argmin(tag, got, e64, e32, span=None):
    """span None: unrefined depth, error by value; else refined depth, error by the sweep's span."""
    lib, flo = pooled(lambda d, p, e: np.abs(d - e["depth"]) / (e["depth"] if span is None else span), got, e64, e32)
    mean, worst, f_mean, f_worst = float(lib.mean()), float(lib.max()), float(flo.mean()), float(flo.max())
    worst_bound = 1e-4 if span is None else 10.0 * f_worst
    print("%s: depth error (%s) mean %.3e (float32 oracle %.3e, bound %.3e), worst pixel %.3e (float32 oracle %.3e, bound %.3e)"
          % (tag, "by value" if span is None else "by span", mean, f_mean, 3.0 * f_mean, worst, f_worst, worst_bound))
    check_probability(tag, got, e64, e32)
    assert mean <= 3.0 * f_mean, (mean, f_mean)
    assert worst < worst_bound if span is None else worst <= worst_bound, (worst, worst_bound)


def check_recurrent(tag, got, e64, e32):
    other = lambda d, p, e: np.abs(d - e["depth"]) > 1e-6 * e["depth"]
    lib_o, flo_o = pooled(other, got, e64, e32)
    rel = lambda d, p, e: (np.abs(p - e["prob"]) / e["prob"])[~other(d, p, e)]
    lib_r, flo_r = pooled(rel, got, e64, e32)
    planes = len(np.unique(np.concatenate([np.ravel(e64[i]["depth"]) for i in e64])))
    print("%s: another plane on %.5f of %d pixels (float32 oracle %.5f, bound 0.005; %d planes in use), probability rel worst "
          "%.3e mean %.3e (float32 oracle worst %.3e, bound %.3e)"
          % (tag, float(lib_o.mean()), lib_o.size, float(flo_o.mean()), planes, float(lib_r.max()), float(lib_r.mean()),
             float(flo_r.max()), 2.0 * float(flo_r.max())))
    assert float(lib_o.mean()) <= 0.005, float(lib_o.mean())
    assert float(lib_r.max()) <= 2.0 * float(flo_r.max()) and float(lib_r.mean()) < 5e-5, (float(lib_r.max()), float(lib_r.mean()))


@pytest.mark.parametrize("inverse_depth", [False, True])
@pytest.mark.parametrize("extractor", ["hip", "torch"])
def test_3dcnn_session_files_match_the_oracle(tmp_path, lib_built, extractor, inverse_depth):
    """7 images, 3 views per cluster: the one tower group holds all seven reference views and the feature cache serves every
    image to up to three clusters.  hip: uint8 upload + standardisation inside the towers; torch: center_images_device.

    Measured, mean abs-rel (library / float32 oracle / bound) and worst pixel (bound 1e-4):
      hip                  2.21e-7 / 2.90e-7 / 8.70e-7, worst 1.80e-6      torch                  1.92e-7, worst 1.87e-6
      hip, inverse depth   2.19e-7 / 2.83e-7 / 8.50e-7, worst 1.36e-6      torch, inverse depth   1.90e-7, worst 1.37e-6"""
    sess = write_session(tmp_path / "sess")
    cfg = config(sess, tmp_path / "out", inverse_depth=inverse_depth)
    got, e64, e32 = run_session(sess, cfg, extractor)
    assert sorted(got) == list(range(7)) and got[0][0].shape == (24, 32)
    check_soft_argmin("3DCNN %s inverse_depth=%s" % (extractor, inverse_depth), got, e64, e32)


@pytest.mark.parametrize("inverse_depth", [False, True])
@pytest.mark.parametrize("gru_views", [1, 3])
def test_gru_session_files_match_the_oracle(tmp_path, lib_built, gru_views, inverse_depth):
    """gru_views 3: _GruBatcher sends two full sweeps and a ragged last one of a single view; 1: one call per view.

    Measured (the same for gru_views 1 and 3): another plane on 0 of 5376 pixels (bound 0.5 %), 24 planes in use; probability
    on the agreeing pixels, worst relative distance (library / float32 oracle / bound) 1.26e-5 / 2.22e-5 / 4.44e-5, mean
    1.6e-6 (bound 5e-5); inverse depth 1.38e-5 / 1.65e-5 / 3.30e-5."""
    sess = write_session(tmp_path / "sess")
    cfg = config(sess, tmp_path / "out", regularization="GRU", inverse_depth=inverse_depth)
    got, e64, e32 = run_session(sess, cfg, gru_views=gru_views)
    assert sorted(got) == list(range(7)) and got[0][0].shape == (24, 32)
    check_recurrent("GRU gru_views=%d inverse_depth=%s" % (gru_views, inverse_depth), got, e64, e32)


@pytest.mark.parametrize("extractor", ["hip", "torch"])
@pytest.mark.parametrize("upsample,confidence", [(False, False), (True, True), (False, True)])
@pytest.mark.parametrize("network", ["original", "unet"])
def test_refined_session_files_match_the_oracle(tmp_path, lib_built, network, upsample, confidence, extractor):
    """--refinement: the guide image is the STANDARDISED reference image.  Before the guide was fixed the hip rows handed the
    decoded 0..255 image to the tower: refined depth off by tens to hundreds of spans (tests/test_session_reference_host.py
    shows the same on the oracle).

    Measured, error by span: mean (library / float32 oracle / bound = 3 x), worst pixel (library / bound = 10 x the oracle's):
      original F,F  hip 6.45e-7 torch 5.77e-7 / 3.65e-6 / 1.10e-5   worst 5.28e-6, 5.15e-6 / 4.05e-4
      original T,T  hip 5.82e-7 torch 5.23e-7 / 6.10e-6 / 1.83e-5   worst 5.89e-6, 6.78e-6 / 7.82e-4
      original F,T  hip 7.29e-7 torch 6.38e-7 / 6.66e-6 / 2.00e-5   worst 4.68e-6, 5.22e-6 / 6.79e-4
      unet     F,F  hip 5.61e-7 torch 4.97e-7 / 2.87e-6 / 8.61e-6   worst 4.20e-6, 3.29e-6 / 3.29e-4
      unet     T,T  hip 4.96e-7 torch 4.52e-7 / 2.02e-6 / 6.05e-6   worst 4.80e-6, 4.58e-6 / 2.81e-4
      unet     F,T  hip 6.49e-7 torch 5.91e-7 / 2.52e-6 / 7.55e-6   worst 4.62e-6, 3.88e-6 / 2.21e-4
    (F,F = upsample, confidence.)  With the raw guide the six hip rows measured a MEAN error of 189, 327, 319 (original) and
    30, 38, 41 (unet) spans; the torch rows were right then too."""
    sess = write_session(tmp_path / "sess", size=(132, 132), n_images=4)
    cfg = config(sess, tmp_path / "out", width=128, height=128, refinement=True, refinement_network=network,
                 upsample_before_refinement=upsample, refine_with_confidence=confidence)
    got, e64, e32 = run_session(sess, cfg, extractor)
    assert sorted(got) == list(range(4)) and got[0][0].shape == ((128, 128) if upsample else (32, 32))
    for i in got:
        assert e64[i]["cam"][1, 0, 2] == pytest.approx(64.0 if upsample else 16.0)      # full-size or quarter-size camera
    check_soft_argmin("refinement %s upsample=%s confidence=%s %s" % (network, upsample, confidence, extractor), got, e64, e32,
                      span=23 * 10.0)


def test_gru_with_refinement_set_refines_nothing_and_max_clusters_limits_the_indices(tmp_path, lib_built):
    """GRU + --refinement: no refinement in the reference (predictlib.py:93-96) or here (this path takes one view per sweep);
    max_clusters_per_session = 3: exactly the indices 0, 1, 2 are written.

    Measured: another plane on 0 of 2304 pixels; probability worst 1.06e-5 (float32 oracle 2.22e-5, bound 4.44e-5)."""
    sess = write_session(tmp_path / "sess")
    cfg = config(sess, tmp_path / "out", regularization="GRU", refinement=True, max_clusters_per_session=3)
    got, e64, e32 = run_session(sess, cfg)
    assert sorted(got) == [0, 1, 2] and got[0][0].shape == (24, 32)
    check_recurrent("GRU with refinement set, 3 clusters", got, e64, e32)


@pytest.mark.parametrize("regularization", ["3DCNN", "GRU"])
def test_clusters_with_their_own_depth_ranges(tmp_path, lib_built, regularization):
    """Odd reference views sweep 450 .. 450 + 23 * 8 mm, even ones 425 .. 425 + 23 * 10: start, interval and end are read per
    cluster from the camera row (a recurrent sweep of three views carries three ranges).

    Measured: 3DCNN mean abs-rel 2.09e-7 (float32 oracle 2.65e-7, bound 7.96e-7), worst pixel 1.61e-6; GRU another plane on 0
    of 5376 pixels (48 distinct depths in use), probability worst 1.20e-5 (float32 oracle 2.22e-5, bound 4.44e-5)."""
    sess = write_session(tmp_path / "sess")
    covis_path = os.path.join(sess, "covisibility.json")
    with open(covis_path) as f:
        covis = json.load(f)
    for k in covis:
        if int(k) % 2:
            covis[k]["min_depth"], covis[k]["max_depth"] = 450.0, 450.0 + 23 * 8.0
    with open(covis_path, "w") as f:
        json.dump(covis, f)
    cfg = config(sess, tmp_path / "out", regularization=regularization)
    got, e64, e32 = run_session(sess, cfg, gru_views=3)
    np.testing.assert_array_equal(e64[1]["cam"][1, 3], [450.0, 8.0, 24, 634.0])
    np.testing.assert_array_equal(e64[2]["cam"][1, 3], [425.0, 10.0, 24, 655.0])
    (check_soft_argmin if regularization == "3DCNN" else check_recurrent)("%s, per-cluster depth ranges" % regularization,
                                                                          got, e64, e32)


def pair_project_from_session(sess, path, plane_counts):
    """The session's images and cameras as an upstream project (images/%08d.jpg, cams/%08d_cam.txt, pair.txt) whose camera
    files are the 30-word form: depth_min, interval AND a plane count of their own."""
    import shutil
    from mvsnet_amd.mvs_data_generation import Cluster
    os.makedirs(os.path.join(path, "images")); os.makedirs(os.path.join(path, "cams"))
    n = len(plane_counts)
    for i, count in enumerate(plane_counts):
        shutil.copy(os.path.join(sess, "images", "%d.jpg" % i), os.path.join(path, "images", "%08d.jpg" % i))
        cam = Cluster(sess, i, [], 425.0, 655.0, 3, depth_num=24).load_camera(i)
        with open(os.path.join(path, "cams", "%08d_cam.txt" % i), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in cam[0]) + "\n\n")
            f.write("intrinsic\n" + "\n".join(" ".join(repr(float(v)) for v in row[:3]) for row in cam[1][:3]) + "\n\n")
            f.write("425.0 10.0 %d\n" % count)
    with open(os.path.join(path, "pair.txt"), "w") as f:
        f.write("%d\n" % n)
        for i in range(n):
            near = sorted((j for j in range(n) if j != i), key=lambda j: (abs(j - i), j))
            f.write("%d\n%d %s\n" % (i, len(near), " ".join("%d %.1f" % (j, 100.0 - abs(j - i)) for j in near)))
    return path


def test_pair_txt_project_with_plane_counts_of_its_own(tmp_path, lib_built):
    """Upstream project format: host-standardised float32 images go up (the oracle starts from the same), and the 30-word
    camera files give reference views 1 and 3 sixteen planes while max_d says 24: the plane count is the camera row's.

    Measured: mean abs-rel 1.96e-7 (float32 oracle 1.58e-7, bound 4.73e-7), worst pixel 1.56e-6 (bound 1e-4)."""
    sess = write_session(tmp_path / "sess", n_images=5)
    proj = pair_project_from_session(sess, str(tmp_path / "proj"), [24, 16, 24, 16, 24])
    cfg = config(proj, tmp_path / "out")
    got, e64, e32 = run_session(proj, cfg)
    assert sorted(got) == list(range(5))
    np.testing.assert_array_equal(e64[1]["cam"][1, 3], [425.0, 10.0, 16, 585.0])
    assert max(got[i][0].max() for i in (1, 3)) <= 425.0 + 15 * 10.0 + 1e-3 < max(got[i][0].max() for i in (0, 2, 4))
    check_soft_argmin("3DCNN, pair.txt project, 16 / 24 planes", got, e64, e32)
