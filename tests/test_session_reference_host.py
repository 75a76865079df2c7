"""CPU tests of tests/session_reference.py, the float64 restatement of a whole session that tests/test_gpu_session_oracle.py
holds `compute_depth_maps` to:

  * float32 against float64 on the session the GPU tests use: the rounding-noise floor is small and the inputs are well
    conditioned (no near-ties in the recurrent sweep, every plane in use), so the GPU bounds -- multiples of this floor --
    are tight;
  * sensitivity: each mistake the session pipeline could make unnoticed (raw 0..255 guide image, source views out of order,
    `inverse_depth` dropped, `max_d` instead of the camera row's plane count) moves the expectation far beyond the bound
    that guards it -- the proof that the GPU tests can fail;
  * the refinement's guide image: `depth_refine` refuses a non-floating guide, `get_depth_and_prob_map` standardises a uint8
    slice itself.
"""
import numpy as np
import pytest

from mvsnet_amd import predictlib as pl, synthetic as S
from tests import session_reference as R

D, INTERVAL = 24, 10.0
SPAN = (D - 1) * INTERVAL


def config(**kw):
    return pl.InferenceConfig(view_num=3, max_d=D, width=128, height=96, base_image_size=8, **kw)


@pytest.fixture(scope="module")
def session(tmp_path_factory):
    return S.write_session(str(tmp_path_factory.mktemp("session") / "sess"), n_images=7, height=100, width=132, view_num=3,
                           depth_num=D, interval=INTERVAL)


def depth_floor(e64, e32, normalise):
    """(mean, worst) of |float32 oracle - float64 oracle| over all views, by value (unrefined) or by the sweep's span."""
    err = [np.abs(e32[i]["depth"] - e64[i]["depth"]) / (e64[i]["depth"] if normalise == "value" else SPAN) for i in e64]
    return float(np.mean([e.mean() for e in err])), float(max(e.max() for e in err))


def test_float32_oracle_floor_3dcnn(session):
    """Measured: depth mean abs-rel 2.9e-7, worst pixel 2.8e-6; probability worst 9.1e-6.  The asserted ceilings are float32
    reasoning, not these figures: a few ulps (6e-8) through a well-conditioned soft-argmin."""
    cfg = config()
    P = R.make_params(cfg)
    e64, e32 = R.expected_outputs(session, cfg, P, np.float64), R.expected_outputs(session, cfg, P, np.float32)
    assert sorted(e64) == list(range(7))
    mean, worst = depth_floor(e64, e32, "value")
    pworst = max(float(np.abs(e32[i]["prob"] - e64[i]["prob"]).max()) for i in e64)
    print("3DCNN float32 floor: depth mean %.3e worst %.3e, prob worst %.3e" % (mean, worst, pworst))
    assert mean < 1e-6 and worst < 1e-5 and pworst < 5e-5
    for i in e64:
        assert e64[i]["depth"].shape == e64[i]["prob"].shape == (24, 32) and e32[i]["depth"].dtype == np.float32
        assert e64[i]["depth"].min() >= 425.0 and e64[i]["depth"].max() <= 425.0 + SPAN
        assert np.ptp(e64[i]["depth"]) > 5 * INTERVAL                      # a depth map with structure, not a constant
        np.testing.assert_array_equal(e64[i]["cam"][1, 3], [425.0, INTERVAL, D, 425.0 + SPAN])


@pytest.mark.parametrize("network,upsample,conf", [("original", False, False), ("unet", True, True), ("original", False, True)])
def test_float32_oracle_floor_refinement(session, network, upsample, conf):
    """The seeded refinement weights give residuals as large as the depth (refined values cross zero), so the error is
    normalised by the sweep's span (D-1) * interval.  Measured: mean 1.4e-6 / worst 1.4e-5 (original), mean 9e-7 / worst
    1.4e-5 (unet, upsampled, with confidence)."""
    cfg = config(refinement=True, refinement_network=network, upsample_before_refinement=upsample, refine_with_confidence=conf,
                 max_clusters_per_session=3)
    P = R.make_params(cfg)
    e64, e32 = R.expected_outputs(session, cfg, P, np.float64), R.expected_outputs(session, cfg, P, np.float32)
    assert sorted(e64) == [0, 1, 2]
    mean, worst = depth_floor(e64, e32, "span")
    print("refinement %s float32 floor (by span): mean %.3e worst %.3e" % (network, mean, worst))
    assert mean < 5e-6 and worst < 1e-4
    plain = R.expected_outputs(session, config(max_clusters_per_session=3), P, np.float64)
    for i in e64:
        size = (96, 128) if upsample else (24, 32)
        assert e64[i]["depth"].shape == e64[i]["prob"].shape == size
        # the probability map is the unrefined one, repeated 4 x 4 when the depth was refined at input resolution
        np.testing.assert_array_equal(e64[i]["prob"][::4, ::4] if upsample else e64[i]["prob"], plain[i]["prob"])
        if upsample:
            np.testing.assert_array_equal(e64[i]["prob"][3::4, 3::4], plain[i]["prob"])
            assert e64[i]["cam"][1, 0, 0] == pytest.approx(4.0 * plain[i]["cam"][1, 0, 0])      # full-size intrinsics
        refined = e64[i]["depth"][::4, ::4] if upsample else e64[i]["depth"]
        assert float(np.abs(refined - plain[i]["depth"]).max()) > INTERVAL                      # the tower does something


def test_float32_oracle_floor_gru_and_gru_ignores_refinement(session):
    """Recurrent sweep: the float32 oracle picks the float64 oracle's plane on every one of the 7 x 768 pixels, with all 24
    planes in use (no near-ties for a wrong kernel to hide behind).  With `refinement` set the GRU branch refines nothing."""
    cfg = config(regularization="GRU")
    P = R.make_params(cfg)
    e64, e32 = R.expected_outputs(session, cfg, P, np.float64), R.expected_outputs(session, cfg, P, np.float32)
    differ = sum(int((np.abs(e32[i]["depth"] - e64[i]["depth"]) > 1e-6 * e64[i]["depth"]).sum()) for i in e64)
    planes = np.unique(np.rint((np.concatenate([e64[i]["depth"].ravel() for i in e64]) - 425.0) / INTERVAL).astype(int))
    prel = max(float((np.abs(e32[i]["prob"] - e64[i]["prob"]) / e64[i]["prob"]).max()) for i in e64)
    print("GRU float32 floor: %d of %d pixels on another plane, %d planes in use, prob rel worst %.3e"
          % (differ, 7 * 768, len(planes), prel))
    assert differ == 0 and len(planes) == D and prel < 1e-4
    cfg_r = config(regularization="GRU", refinement=True, max_clusters_per_session=2)
    e_r = R.expected_outputs(session, cfg_r, R.make_params(cfg_r), np.float64)
    for i in (0, 1):
        np.testing.assert_array_equal(e_r[i]["depth"], e64[i]["depth"])
        np.testing.assert_array_equal(e_r[i]["prob"], e64[i]["prob"])


def _one_cluster(session, cfg, index=3):
    gen, clusters = R.session_clusters(session, cfg)
    return R.cluster_inputs(gen, clusters[index])


@pytest.mark.parametrize("network", ["original", "unet"])
def test_a_raw_guide_image_moves_the_refined_depth_far_beyond_the_bound(session, network):
    """The bug this oracle was written for: the decoded 0..255 image as the refinement's guide instead of the standardised
    one.  Bound that guards it: mean span-normalised error <= 3 x the float32 oracle's (~4e-6).  Measured: the raw guide
    moves the mean by tens to hundreds of spans."""
    # the unet tower halves its input four times: at 96 x 128 it runs on the upsampled depth (24 rows do not divide by 16)
    cfg = config(refinement=True, refinement_network=network, upsample_before_refinement=network == "unet")
    P = R.make_params(cfg)
    images, out_cams, full_cams, _ = _one_cluster(session, cfg)
    assert images.dtype == np.uint8
    good = R.cluster_outputs(images, out_cams, full_cams, cfg, P, np.float64)
    f32 = R.cluster_outputs(images, out_cams, full_cams, cfg, P, np.float32)
    bad = R.cluster_outputs(images, out_cams, full_cams, cfg, P, np.float64, guide=images[0])
    bound = 3.0 * float(np.mean(np.abs(f32["depth"] - good["depth"])) / SPAN)
    moved = float(np.mean(np.abs(bad["depth"] - good["depth"])) / SPAN)
    print("raw guide (%s): mean change %.3e spans, bound %.3e" % (network, moved, bound))
    assert moved > 1.0 and moved > 1e4 * bound
    assert float(np.mean(np.abs(bad["depth"] - good["depth"]) / np.abs(good["depth"]))) > 10.0


@pytest.mark.parametrize("regularization", ["3DCNN", "GRU"])
def test_each_injected_mistake_exceeds_its_bound(session, regularization):
    """Source views out of order (features of view 2 with the camera of view 1), `inverse_depth` dropped, and `max_d` in place
    of the camera row's plane count: each moves the expectation beyond the bound of the GPU test -- 3DCNN: mean abs-rel
    <= 3 x the float32 oracle's; GRU: another winning plane on <= 0.5 % of the pixels."""
    cfg = config(regularization=regularization)
    P = R.make_params(cfg)
    images, out_cams, full_cams, _ = _one_cluster(session, cfg)

    def distance(a, b):
        if regularization == "GRU":
            return float((np.abs(a["depth"] - b["depth"]) > 1e-6 * b["depth"]).mean())
        return float(np.mean(np.abs(a["depth"] - b["depth"]) / b["depth"]))

    good = R.cluster_outputs(images, out_cams, full_cams, cfg, P, np.float64)
    f32 = R.cluster_outputs(images, out_cams, full_cams, cfg, P, np.float32)
    bound = 0.005 if regularization == "GRU" else 3.0 * distance(f32, good)
    assert distance(f32, good) < bound or regularization == "GRU" and distance(f32, good) == 0.0
    swapped = R.cluster_outputs(images[[0, 2, 1]], out_cams, full_cams, cfg, P, np.float64)
    cfg_inv = config(regularization=regularization, inverse_depth=True)
    inv = R.cluster_outputs(images, out_cams, full_cams, cfg_inv, P, np.float64)
    # a camera row that says 16 planes while max_d says 24: same start and interval, the sweep ends earlier
    cams16 = np.array(out_cams); cams16[:, 1, 3, 2] = 16; cams16[:, 1, 3, 3] = 425.0 + 15 * INTERVAL
    by_row = R.cluster_outputs(images, cams16, full_cams, cfg, P, np.float64)
    by_max_d = R.cluster_outputs(images, cams16, full_cams, cfg, P, np.float64, depth_num=cfg.max_d)
    assert by_row["depth"].max() <= 425.0 + 15 * INTERVAL + 1e-9
    for name, d_ in (("swapped source views", distance(swapped, good)), ("inverse_depth dropped", distance(good, inv)),
                     ("max_d for the row's plane count", distance(by_max_d, by_row))):
        print("%s, %s: moved %.3e, bound %.3e" % (regularization, name, d_, bound))
        assert d_ > 20.0 * bound, (name, d_, bound)


def test_depth_refine_refuses_a_uint8_guide_and_predictlib_standardises_one(monkeypatch):
    """`torch.cat` would promote a decoded 0..255 guide silently (refined depth wrong by orders of magnitude).
    refine.depth_refine raises TypeError; predictlib.get_depth_and_prob_map, which takes slice 0 of `full_images` as the guide
    when none is given, standardises a uint8 slice: same refined depth as with host-standardised float images, and the float64
    oracle's."""
    import types
    import torch
    from oracle import mvsnet_oracle as O
    from mvsnet_amd import model as M
    from mvsnet_amd.mvs_data_generation import center_image
    from mvsnet_amd.refine import RefineNet, depth_refine, make_refine_params
    rs = np.random.RandomState(5)
    N, H, W, Dn, start, interval = 3, 32, 48, 8, 425.0, 20.0
    u8 = rs.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)
    d0 = (start + (Dn - 1) * interval * rs.rand(1, H // 4, W // 4, 1)).astype(np.float32)
    p0 = rs.rand(1, H // 4, W // 4, 1).astype(np.float32)
    params = make_refine_params("original", "normal", 5, seed=4)
    net = RefineNet(params, "original", device="cpu")
    with pytest.raises(TypeError, match="standardised"):
        depth_refine(torch.as_tensor(d0), torch.as_tensor(u8[0:1]), torch.as_tensor(p0), Dn, start, interval, net,
                     refine_with_confidence=True)
    with pytest.raises(TypeError, match="stereo_image"):
        depth_refine(torch.as_tensor(d0), torch.as_tensor(center_image(u8[0]))[None], torch.as_tensor(p0), Dn, start, interval,
                     net, refine_with_confidence=True, stereo_image=torch.as_tensor(u8[1:2]))
    seen = []

    def fake_inference_mem(images, *a, **k):            # the plane sweep is the GPU library's: not under test here
        seen.append(images.dtype)
        return torch.as_tensor(d0), torch.as_tensor(p0)
    monkeypatch.setattr(M, "inference_mem", fake_inference_mem)
    cfg = pl.InferenceConfig(view_num=N, max_d=Dn, refinement=True, refine_with_confidence=True)
    weights = types.SimpleNamespace(refine=net)
    cams = torch.zeros((1, N, 2, 4, 4))
    host = np.stack([center_image(im) for im in u8])
    want = O.depth_refine(d0[0], O.standardise_image(u8[0], np.float64), p0[0], Dn, start, interval, params, "original",
                          refine_with_confidence=True, dtype=np.float64)[0]
    raw = O.depth_refine(d0[0], u8[0], p0[0], Dn, start, interval, params, "original", refine_with_confidence=True,
                         dtype=np.float64)[0]
    span = (Dn - 1) * interval
    assert float(np.mean(np.abs(raw - want))) / span > 1.0              # what the silent promotion would have given
    for images in (torch.as_tensor(u8)[None], torch.as_tensor(u8), torch.as_tensor(host)[None]):
        d, p, residual = pl.get_depth_and_prob_map(images, cams, start, interval, cfg, weights, depth_num=Dn)
        err = float(np.max(np.abs(d.numpy()[0] - want))) / span
        assert err < 1e-5, err
        assert torch.equal(p, torch.as_tensor(p0)) and residual.shape == d.shape
    assert seen == [torch.uint8, torch.uint8, torch.float32]           # the towers still get the decoded images
