"""The reference side of the every-pixel rule of the recurrent sweep (tests/sweep_reference.py), on the CPU alone: the oracle's
optional per-plane scores change nothing else, the float32 evaluations of the reference stay inside the 4 E bound on every case the
GPU file runs -- the condition that makes the bound legitimate -- and the faults a sweep kernel can have do not."""
import numpy as np
import pytest

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S

from tests import sweep_reference as R

CASES = R.all_cases()
ids = lambda k: "%s-%dx%d-D%d-v%d" % k


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("inverse", [False, True])
def test_return_scores_changes_nothing_and_reproduces_the_outputs(dtype, inverse):
    w = S.make_workload("toy")
    gp = S.make_gru_params("normal", seed=2, in_channels=w.channels, random_affine=True)
    args = (w.features, w.cams, w.depth_num, w.depth_start, w.depth_end, gp, inverse, dtype)
    d0, p0 = O.inference_winner_take_all_from_features(*args)
    out = O.inference_winner_take_all_from_features(*args, return_scores=True)
    assert len(out) == 3
    d1, p1, reg = out
    assert np.array_equal(d0, d1) and np.array_equal(p0, p1) and d1.dtype == dtype and p1.dtype == dtype
    assert reg.shape == (w.depth_num, w.height, w.width) and reg.dtype == dtype
    # the arg-max (first maximum) and max / sum of the scores, evaluated as the loop does, are the outputs
    e = np.exp(reg).astype(dtype)
    depths = O.wta_depths(w.depth_num, w.depth_start, w.depth_end, inverse, dtype)
    assert np.array_equal(depths[e.argmax(0)], d1)
    s = np.zeros_like(e[0])
    for d in range(w.depth_num):
        s = s + e[d]
    assert np.array_equal((e.max(0) / (s + dtype(1e-7))).astype(dtype), p1)
    # and the restated sweep of sweep_reference.py is the oracle's, with its hooks engaged but idle as well
    d2, p2, r2 = R.sweep(*args[:6], inverse, dtype, act=lambda x: x)
    assert np.array_equal(d2, d1) and np.array_equal(p2, p1) and np.array_equal(r2, reg)


def test_plane_scores_are_cached_and_read_only():
    c, ref = R.case_scores("normal", 5, 11, 17)
    assert R.plane_scores(c["features"].copy(), c["cams"], c["D"], c["start"], c["end"], c["gp"], False) is ref
    assert ref.E > 0 and ref.reg64.shape == (17, 5, 11) and ref.depths.shape == (17,)
    with pytest.raises(ValueError):
        ref.reg32[0, 0, 0] = 0


@pytest.mark.parametrize("key", CASES, ids=ids)
def test_float32_reference_stays_inside_the_bound(key):
    """The float32 oracle, and a float32 sweep whose every sigmoid, tanh and cell output is off by up to 4 ulp (twice the device's
    documented activation error), on every case of the GPU file.  Measured here: no winner differs (regret 0 E), prob within
    0.92 E on the plain float32 oracle and 0.93 E perturbed, the perturbed scores within 1.07 E."""
    c, ref = R.case_scores(*key)
    R.check_every_pixel(ref.depth32, ref.prob32, ref, "float32 " + ids(key))
    rs = np.random.RandomState(11)
    d, p, reg = R.sweep(c["features"], c["cams"], c["D"], c["start"], c["end"], c["gp"], False, np.float32, act=R.perturb_ulps(rs, 4))
    score = float(np.abs(reg.astype(np.float64) - ref.reg64).max()) / ref.E
    print("perturbed scores: %.2f E" % score)
    assert score <= 2.0, score                       # the sweep's rule for a score (tests/test_gpu_full_size.py)
    R.check_every_pixel(d, p, ref, "float32 +-4 ulp " + ids(key))


@pytest.mark.parametrize("name", R.CAMERA_FAMILIES)
def test_float32_reference_stays_inside_the_bound_under_camera_families(name):
    """The two camera cases of tests/test_gpu_forward_cameras.py: the same two evaluations under roll90 and random3."""
    c, ref = R.case_scores("normal", *R.CAMERA_SHAPE, cams=R.family_cams(name))
    assert not np.array_equal(c["cams"], R.small_cams())
    R.check_every_pixel(ref.depth32, ref.prob32, ref, "float32 " + name)
    rs = np.random.RandomState(11)
    d, p, reg = R.sweep(c["features"], c["cams"], c["D"], c["start"], c["end"], c["gp"], False, np.float32, act=R.perturb_ulps(rs, 4))
    score = float(np.abs(reg.astype(np.float64) - ref.reg64).max()) / ref.E
    print("perturbed scores: %.2f E" % score)
    assert score <= 2.0, score
    R.check_every_pixel(d, p, ref, "float32 +-4 ulp " + name)


def test_default_cameras_of_a_case_are_unchanged():
    c = R.case("normal", 5, 11, 17)
    assert np.array_equal(c["cams"], R.small_cams())
    assert R.case_scores("normal", 5, 11, 17)[1] is R.case_scores("normal", 5, 11, 17, cams=R.small_cams())[1]


# ---- planted faults ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    c, ref = R.case_scores("normal", 27, 41, 16)
    R.check_every_pixel(ref.depth32, ref.prob32, ref, "passing result")
    return c, ref


def _run(c, **hooks):
    return R.sweep(c["features"], c["cams"], c["D"], c["start"], c["end"], c["gp"], False, np.float32, **hooks)


def test_planted_dropped_halo_in_the_last_column_fails_the_new_rule_and_what_the_old_one_saw(base):
    """Cell 1 convolves the right-hand image column as a tile of its own whose halo (the column to its left) reads as zeros; that
    column of the result is taken from the faulty sweep: 27 of 1107 pixels, 2.4 %.

    What the rule the sweep tests had (97 % of the winners, prob of THOSE to 5e-4) makes of it, measured here: 12 of the 27
    pixels change their winner, the share of equal winners stays at 98.9 % and those 12 are never looked at again; the fault is
    noticed only because the other 15 keep their plane with a prob 2 - 26 % off.  Take the 12 alone -- a fault that moves every
    winner it touches, or one in a map with closer scores -- and the old rule passes while every one of them is wrong.  The new
    rule fails both."""
    c, ref = base
    W = c["features"].shape[2]

    def conv1(x, w, b):
        y = O.conv2d_same(x, w, 1, b, np.float32)
        cut = x.copy(); cut[:, W - 2] = 0
        y[:, W - 1] = O.conv2d_same(cut, w, 1, b, np.float32)[:, W - 1]
        return y
    fd, fp, _ = _run(c, conv1=conv1)
    ed, ep, _ = R.sweep(c["features"], c["cams"], c["D"], c["start"], c["end"], c["gp"], False, np.float64)
    assert R.old_rule(ref.depth32, ref.prob32, ed, ep, 0.97, 5e-4)
    column = np.zeros(fd.shape, bool); column[:, W - 1] = True
    flipped = column & (fd != ref.depth32)
    assert 0 < flipped.sum() < column.sum() == 27
    for name, where, old_passes in (("whole column", column, False), ("its flipped winners", flipped, True)):
        depth, prob = np.where(where, fd, ref.depth32), np.where(where, fp, ref.prob32)
        same = np.abs(depth - ed) <= 1e-6 * np.abs(ed)
        print("%s: %d pixels, equal winners %.4f, old rule passes: %s" % (name, where.sum(), same.mean(), R.old_rule(depth, prob, ed, ep)))
        assert same.mean() > 0.97                                       # the old winner clause never objects
        assert R.old_rule(depth, prob, ed, ep, 0.97, 5e-4) == old_passes
        with pytest.raises(AssertionError, match="winner regret .* E > 4 E"):
            R.check_every_pixel(depth, prob, ref, "dropped halo, " + name)


def test_planted_column_written_one_plane_late_passes_the_old_rule_and_fails_the_new(base):
    """The right-hand column holds the depth value of the plane after the winner (a masked lane that stored anyway): all 27 winners
    differ, the old rule drops them (97.6 % > 97 %) and passes.  The gap this file closes."""
    c, ref = base
    ed, ep, _ = R.sweep(c["features"], c["cams"], c["D"], c["start"], c["end"], c["gp"], False, np.float64)
    plane = R.measure(ref.depth32, ref.prob32, ref)[0]
    depth = ref.depth32.copy()
    depth[:, -1] = ref.depths[(plane[:, -1] + 1) % c["D"]]
    assert R.old_rule(depth, ref.prob32, ed, ep, 0.97, 5e-4)
    with pytest.raises(AssertionError, match="winner regret .* E > 4 E"):
        R.check_every_pixel(depth, ref.prob32, ref, "column one plane late")


def test_planted_layernorm_count_of_padded_tiles_fails(base):
    c, ref = base
    H, W = c["features"].shape[1:3]
    padded = (-(-H // 8) * 8) * (-(-W // 16) * 16)               # the fused sweep's 8 x 16 pixel tiles
    assert padded != H * W
    d, p, _ = _run(c, ln_count=lambda F: float(padded * F))
    with pytest.raises(AssertionError, match="E > 4 E"):
        R.check_every_pixel(d, p, ref, "LayerNorm count")
    d, p, _ = _run(c, ln_count=lambda F: float(H * W * F))       # the same form with the right count passes
    R.check_every_pixel(d, p, ref, "LayerNorm sums / (H W F)")


def test_planted_depth_values_one_plane_late_fail(base):
    c, ref = base
    plane = R.measure(ref.depth32, ref.prob32, ref)[0]
    interval = ref.depths[1] - ref.depths[0]
    shifted = np.where(plane + 1 < c["D"], ref.depths[np.minimum(plane + 1, c["D"] - 1)], ref.depths[-1] + interval).astype(np.float32)
    with pytest.raises(AssertionError):
        R.check_every_pixel(shifted, ref.prob32, ref, "depth values shifted")
    inside = np.where(plane + 1 < c["D"], shifted, ref.depth32)  # without the pixels pushed past the last plane: the regret alone
    with pytest.raises(AssertionError, match="winner regret"):
        R.check_every_pixel(inside, ref.prob32, ref, "depth values shifted, inside the range")


def test_planted_last_plane_missing_from_exp_sum_fails(base):
    c, ref = base
    e = np.exp(ref.reg32)
    s = np.zeros_like(e[0])
    for d in range(c["D"] - 1):
        s = s + e[d]
    with pytest.raises(AssertionError, match="prob .* E > 4 E"):
        R.check_every_pixel(ref.depth32, e.max(0) / (s + np.float32(1e-7)), ref, "exp_sum without the last plane")


def _wta(reg, depths, take):
    mp = np.zeros(reg.shape[1:], np.float32); di = np.zeros_like(mp); s = np.zeros_like(mp)
    for d in range(reg.shape[0]):
        p = np.exp(reg[d])
        upd = take(mp, p)
        mp = np.where(upd, p, mp); di = np.where(upd, depths[d], di); s = s + p
    return di, mp / (s + np.float32(1e-7))


def test_planted_non_strict_update_on_bit_equal_planes_fails():
    """A hand-made map: planes 2 and 5 hold the same, largest, score bit for bit.  '<' keeps plane 2; '<=' takes plane 5 -- the
    same score, zero regret, the same prob: only the first-maximum clause of the rule sees it."""
    rs = np.random.RandomState(3)
    reg = rs.uniform(-3, -1, size=(8, 4, 6)).astype(np.float32)
    reg[2] = reg[5] = rs.uniform(0, 1, size=(4, 6)).astype(np.float32)
    depths = (425 + 60 * np.arange(8)).astype(np.float32)
    ref = R.Scores(reg.astype(np.float64) + 1e-7 * rs.standard_normal(reg.shape[1:]), reg, depths)
    assert ref.E > 0 and np.array_equal(ref.reg64[2], ref.reg64[5])
    d, p = _wta(reg, depths, lambda mp, pr: mp < pr)
    assert np.all(d == depths[2])
    R.check_every_pixel(d, p, ref, "strict update")
    d, p = _wta(reg, depths, lambda mp, pr: mp <= pr)
    assert np.all(d == depths[5])
    with pytest.raises(AssertionError, match="later one of bit-equal planes"):
        R.check_every_pixel(d, p, ref, "non-strict update")
