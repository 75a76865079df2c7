"""The reference side of the every-voxel rule of the forward warp and cost volume (tests/forward_warp_reference.py), on the CPU
alone: the float32 oracle stays within BOUND / 3 units at every voxel of every case the GPU file runs -- the condition that makes
the bound legitimate --, the case table reaches what it claims to reach (all four wave-tile votes, samples inside the image, the
hand-made transforms' sign change, saturation and exact zero), and faults planted into a numpy copy of the sweep kernel's
block-and-weights scheme are caught at some voxel."""
import warnings

import numpy as np
import pytest

from oracle import mvsnet_oracle as O

from tests import forward_warp_reference as F

CASES = F.all_cases()
CAMERA_CASES = F.camera_cases()
ids = lambda c: c.tag
f32 = np.float32


@pytest.fixture(autouse=True)
def _quiet():
    """The float32 oracle divides by the exact zero of exact_zero on purpose."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        yield


def test_the_bound_is_three_times_the_oracles_worst_rounded_up():
    assert F.BOUND == np.ceil(F.MARGIN * F.ORACLE_WORST) == 4.0


@pytest.mark.parametrize("case", [F._camera_case("random3", 26.5), F.hand_cases(16)[0], F.hand_cases(16)[3]], ids=ids)
def test_the_float64_sample_is_the_oracles(case):
    """warp64 is O.image_projective_transform_bilinear in float64, non-finite pixels included."""
    p = F.problem(case)
    for v in range(p.T.shape[0]):
        for d in range(p.T.shape[1]):
            exp = O.image_projective_transform_bilinear(p.features[v + 1], p.T[v, d].astype(np.float64), np.float64)
            got = F.warp64(p.features[v + 1], p.T[v, d])[0]
            assert np.array_equal(np.isfinite(got), np.isfinite(exp))
            np.testing.assert_allclose(got, exp, rtol=0, atol=1e-13, equal_nan=True)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_float32_oracle_stays_within_a_third_of_the_bound(case):
    """mem and eager variants (the negated eager one included: a sign), every plane of every view through the warp, and the
    numpy copy of the sweep's scheme, which the planted faults below start from.  Measured worst over the table: mem 0.93,
    eager 1.06, warp 0.48, scheme 1.04 / 1.16."""
    p = F.problem(case)
    ref, unit = F.reference(case)
    third = F.BOUND / F.MARGIN
    for variant in ("mem", "eager"):
        F.check_every_voxel(F.oracle_volume(p.features, p.T, variant), ref, unit, "float32 %s %s" % (variant, case.tag), third)
    F.check_every_voxel(F.oracle_volume(p.features, p.T, "eager", negate=True), -ref, unit, "float32 -eager " + case.tag, third)
    worst = 0.0
    for v in range(p.T.shape[0]):
        for d in range(p.T.shape[1]):
            wr, wu = F.warp_reference(p.features[v + 1], p.T[v, d])
            got = O.image_projective_transform_bilinear(p.features[v + 1], p.T[v, d], f32)
            assert np.array_equal(np.isnan(got), np.isnan(wr))
            worst = max(worst, float(F.ratio(got, wr, wu).max()))
    print("float32 warp %s: worst %.3f units" % (case.tag, worst))
    assert worst <= third
    for variant in ("mem", "eager"):
        F.check_every_voxel(F.sweep_scheme(p.features, p.T, variant), ref, unit, "scheme %s %s" % (variant, case.tag), third)


def test_sub_range_reference_is_the_planes_of_the_whole():
    """The GPU file compares a launch of planes 3, 4 with those planes of the reference: the reference has no state across planes."""
    case = F._camera_case("roll60", 2.65)
    p = F.problem(case)
    ref, unit = F.reference(case)
    r2, u2 = F.volume_reference(p.features, p.T[:, 3:5])
    assert np.array_equal(r2, ref[3:5]) and np.array_equal(u2, unit[3:5])


# ---- what the case table reaches ---------------------------------------------------------------------------------------------
def test_every_tile_shape_is_voted_by_some_case():
    votes = {}
    for case in CAMERA_CASES:
        if F.takes_sweep(case):
            p = F.problem(case)
            votes.setdefault(F.vote(p.T, case.height, case.width, case.channels), []).append(case.tag)
    print({k: len(v) for k, v in votes.items()})
    assert sorted(votes) == [0, 1, 2, 3], votes
    by_name = {(nm, iv): F.vote(F.problem(F._camera_case(nm, iv)).T, F.H, F.W, F.C) for nm in F.FAMILIES for iv in F.INTERVALS}
    assert [by_name[v] for v in F.VOTERS] == [0, 1, 2, 3]
    assert {nm for (nm, iv), t in by_name.items() if t == 1} == {"roll60"}
    # 64 channels: a wave holds 4 pixels, the vote is capped at 2
    assert F.vote(F.problem(F._camera_case("zoom2", 26.5, channels=64)).T, F.H, F.W, 64) == 2


@pytest.mark.parametrize("case", CAMERA_CASES, ids=ids)
def test_every_source_view_keeps_a_hundred_samples_inside_the_image(case):
    p = F.problem(case)
    counts = [sum(F.in_image(p.T[v, d], case.height, case.width) for d in range(case.planes)) for v in range(case.views - 1)]
    assert min(counts) >= 100, counts


def test_the_long_interval_moves_the_samples_across_many_taps():
    """At interval 2.65 a sample travels at most a few pixels over the 8 planes; at 26.5 tens: the tap cache refetches."""
    travel = {}
    for iv in F.INTERVALS:
        worst = 0.0
        for nm in F.FAMILIES:
            T = F.problem(F._camera_case(nm, iv)).T
            for v in range(T.shape[0]):
                a, b = F.sample_points(T[v, 0], F.H, F.W), F.sample_points(T[v, -1], F.H, F.W)
                worst = max(worst, float(np.hypot(b[1] - a[1], b[2] - a[2]).max()))
        travel[iv] = worst
    print(travel)
    assert travel[2.65] < 8 and travel[26.5] > 20


def test_hand_made_transforms_do_what_their_names_say():
    Hh, Ww = F.HAND_H, F.HAND_W
    T = F.hand_transforms("horizon")
    for d in range(4):
        p, sx, _sy, _dx, _dy = F.sample_points(T[1, d], Hh, Ww)
        assert (p[:, :11] > 0).all() and (p[:, 11:] < 0).all() and np.abs(p).min() >= 0.047
        assert sx[:, 10].min() > 10 * Ww and sx[:, 11].max() < -10 * Ww      # tens of image widths, both sides
    T = F.hand_transforms("far_out")
    p, sx, sy, _dx, _dy = F.sample_points(T[1, 0], Hh, Ww)
    assert sx.min() > 2.0 ** 31 and F._cvt_i32(np.floor(sx).astype(f32)).min() == 2 ** 31 - 1
    p, sx, sy, _dx, _dy = F.sample_points(T[1, 1], Hh, Ww)
    assert sx.max() < -2.0 ** 31 and sy.max() < -2.0 ** 31 and F._cvt_i32(np.floor(sx).astype(f32)).max() == -2 ** 31
    x0 = np.floor(F.sample_points(T[1, 2], Hh, Ww)[1]).astype(f32)
    assert (x0 >= 2.0 ** 24).all() and (x0[:, 0] + f32(1) == x0[:, 0]).all()
    T = F.hand_transforms("near_zero")
    for d in range(4):
        p = F.sample_points(T[1, d], Hh, Ww)[0]
        assert (p[:, 8] == 2.0 ** -20).all() and np.abs(np.delete(p, 8, axis=1)).min() >= 0.124
        x = np.arange(Ww, dtype=f32)
        assert ((T[1, d, 6] * x + f32(1))[8] == f32(2.0 ** -20))                  # in float32 as well
    T = F.hand_transforms("exact_zero")
    x = np.arange(Ww, dtype=f32)
    for d in range(4):
        p, sx, sy, _dx, _dy = F.sample_points(T[1, d], Hh, Ww)
        assert (p[:, 8] == 0).all() and (np.delete(p, 8, axis=1) != 0).all()
        assert (T[1, d, 6] * x + f32(1))[8] == 0
        if d < 2:
            assert np.isinf(sx[:, 8]).all() and np.isinf(sy[:, 8]).all()
        else:
            assert np.isnan(sx[:, 8]).all() and np.isnan(sy[:, 8]).all()
    ref, _unit = F.reference(F.hand_cases(16)[3])                 # +-inf contributes 0, 0 / 0 is NaN (include/mvsnet_hip.h)
    assert np.isnan(ref[2:, :, 8]).all() and np.isfinite(ref[:2]).all() and np.isfinite(np.delete(ref, 8, axis=2)).all()
    for case in F.hand_cases(16)[:3]:
        assert np.isfinite(F.reference(case)[0]).all()
    # the benign views stay in the image on every plane of every hand-made case
    for v in (0, 2):
        assert min(F.in_image(T[v, d], Hh, Ww) for d in range(4)) >= 100


def test_a_view_outside_the_image_does_not_disturb_the_others():
    """far_out's middle view samples nothing: the reference is the variance of the other views and a zero, exactly."""
    case = F.hand_cases(16)[1]
    p = F.problem(case)
    ref, _unit = F.reference(case)
    zeros = np.zeros_like(p.features[2])
    exp = np.stack([O.variance_cost_mem(p.features[0], [O.image_projective_transform_bilinear(p.features[1], p.T[0, d], np.float64), zeros,
                                                        O.image_projective_transform_bilinear(p.features[3], p.T[2, d], np.float64)],
                                        4, np.float64) for d in range(4)])
    np.testing.assert_allclose(ref, exp, rtol=0, atol=1e-12)


def test_far_worlds_keep_the_homographies_and_strain_the_float32_chain():
    """The float64 homographies move by rounding of the float32 cameras only; the float32 chain's distance from float64 grows
    with the shift.  Measured on random0: 2.3e-6 at home, then 4.4e-6 and 1.9e-5 (largest |T32 - T64| over the 8-vectors)."""
    cams = F.family_cams("random0")
    start, interval = float(cams[0, 1, 3, 0]), float(cams[0, 1, 3, 1])
    dist = []
    for world in (cams,) + tuple(F.far_world(cams, sh, deg) for sh, deg in F.FAR_WORLDS):
        T64, _H64, _bT, _bH, e = F.homography_reference(world, F.D, start, interval, 0.0, False)
        dist.append(e)
        if world is not cams:
            print("moved world, float64 8-vectors from home:", float(np.abs(T64 - home).max()))
            assert np.abs(T64 - home).max() < 1e-2          # the same geometry up to the float32 rounding of the moved cameras
        else:
            home = T64
    print("float32 chain from float64:", dist)
    assert dist[0] < dist[1] < dist[2]


# ---- planted faults ----------------------------------------------------------------------------------------------------------
FAULTS = [("weights_x", "roll30", 2.65), ("weights_x", "tilt20", 26.5), ("weights_corner", "roll30", 2.65),
          ("weights_corner", "random3", 26.5), ("stale_row", "roll90", 26.5), ("stale_row", "tilt20", 26.5),
          ("offset", "zoom0.5", 26.5), ("offset", "random3", 26.5), ("rcp18", "zoom0.5", 26.5), ("rcp18", "roll60", 26.5)]


@pytest.mark.parametrize("fault,name,interval", FAULTS, ids=["%s-%s-i%g" % f for f in FAULTS])
def test_planted_fault_in_the_sweeps_scheme_fails_the_rule(fault, name, interval):
    """Measured: the weights left behind by a clamped block and the stale tap block are off by 1e5 .. 1e7 units at hundreds to
    thousands of voxels, a sample point off by 1e-3 px by 100 .. 800 units, a reciprocal good to 2^-18 by 9 .. 10 units."""
    case = F._camera_case(name, interval)
    p = F.problem(case)
    ref, unit = F.reference(case)
    F.check_every_voxel(F.sweep_scheme(p.features, p.T, "mem"), ref, unit, "unplanted " + case.tag)
    with pytest.raises(AssertionError, match="units > 4"):
        F.check_every_voxel(F.sweep_scheme(p.features, p.T, "mem", fault=fault), ref, unit, "%s %s" % (fault, case.tag))


@pytest.mark.parametrize("ty_log2", [0, 1, 2])
def test_planted_tile_with_x_and_y_swapped_fails_the_rule(ty_log2):
    case = F._camera_case("roll60", 2.65)
    p = F.problem(case)
    ref, unit = F.reference(case)
    good = F.oracle_volume(p.features, p.T, "mem")
    assert np.array_equal(F.swap_tile(good, case.channels, 3), good)          # 8 x 1: one column, nothing to swap
    bad = F.swap_tile(good, case.channels, ty_log2)
    if ty_log2 == 0:                                                          # 1 x 8: one row, nothing to swap either
        assert np.array_equal(bad, good)
        return
    with pytest.raises(AssertionError, match="units > 4"):
        F.check_every_voxel(bad, ref, unit, "tile swapped, %d rows" % (1 << ty_log2))


def test_planted_transform_of_the_neighbouring_view_on_the_last_plane_fails_the_rule():
    case = F._camera_case("random3", 2.65, views=5)
    p = F.problem(case)
    ref, unit = F.volume_reference(p.features, p.T)
    Tf = p.T.copy()
    Tf[1:, -1] = p.T[:-1, -1]
    bad = F.oracle_volume(p.features, Tf, "mem")
    F.check_every_voxel(bad[:-1], ref[:-1], unit[:-1], "planes before the last")
    with pytest.raises(AssertionError, match="units > 4"):
        F.check_every_voxel(bad, ref, unit, "last plane with view v's transform for view v + 1")


def test_a_voxel_finite_on_one_side_only_fails_the_rule():
    """proj == 0: a +-inf sample point contributes 0 and a 0 / 0 one makes the voxel NaN (include/mvsnet_hip.h).  A result that
    is NaN at the +-inf voxels too (tf.contrib.image.transform's inf - inf weights, the per-plane kernel before it was brought
    to the sweep's behaviour) fails, and so does one that is finite at the 0 / 0 voxels."""
    case = F.hand_cases(16)[3]
    p = F.problem(case)
    ref, unit = F.reference(case)
    got = F.oracle_volume(p.features, p.T, "mem")
    F.check_every_voxel(got, ref, unit, "oracle " + case.tag)
    tf_like = got.copy(); tf_like[:, :, 8] = np.nan
    with pytest.raises(AssertionError, match="finite on one side only"):
        F.check_every_voxel(tf_like, ref, unit, "NaN at a +-inf sample point")
    finite = np.where(np.isfinite(got), got, f32(0))
    with pytest.raises(AssertionError, match="finite on one side only"):
        F.check_every_voxel(finite, ref, unit, "finite at 0 / 0")
