"""tests/value_cases.py on the CPU: every family has the property it is named for, every floor E is positive, the float32
restatements stay inside the bound the kernels are held to, the Winograd restatement is the direct one on integers, the ratio of
ratio_weights is pinned, and the model of float32 per-lane BatchNorm sums behaves as its run length says."""
import numpy as np
import pytest

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S

from tests import value_cases as V

SHAPE = (6, 10, 34, 32)


# ---- families and affines ------------------------------------------------------------------------------------------------------
def test_families_have_the_property_they_are_named_for():
    x = {f: V.family(f, SHAPE, 3) for f in V.FAMILIES}
    for f, a in x.items():
        assert a.dtype == np.float32 and a.shape == SHAPE and np.isfinite(a).all(), f
        assert np.array_equal(a, V.family(f, SHAPE, 3)), f                      # named and fixed
    flat = {f: a.reshape(-1, 32).astype(np.float64) for f, a in x.items()}
    assert abs(flat["normal"].mean()) < 0.02 and abs(flat["normal"].std() - 1) < 0.02
    r = np.abs(flat["offset"].mean(0)) / flat["offset"].std(0)
    assert r.min() > 55 and r.max() < 75                                           # mean / deviation = 64
    v = flat["variance-like"]
    assert v.min() >= 0
    scale = v.mean(0)
    assert scale.max() / scale.min() > 300                                          # channel scales over decades
    kurt = ((v - v.mean(0)) ** 4).mean(0) / v.var(0) ** 2
    assert kurt.min() > 8                                                           # chi-square(1): 15; a normal: 3
    dev = flat["range"].std(0)
    k = np.log2(dev)
    assert k.max() - k.min() >= 16 and k.max() <= 12.2 and k.min() >= -12.2
    d = flat["dead"]
    assert not d[:, 0::4].any() and all(d[:, j].any() for j in range(32) if j % 4)
    assert (d == 0).mean() == 0.25
    s = flat["sparse"]
    assert 0.045 < (s != 0).mean() < 0.055 and 40 < s[s != 0].std() < 60


def test_affines_do_what_they_are_named_for():
    for fam in V.FUSED_FAMILIES:
        x = V.family(fam, SHAPE, 4)
        mean = V.OFFSET if fam == "offset" else 0.0
        sc, sh = V.affines("near-identity", 32, 5, mean)
        assert abs(sc.mean() - 1) < 0.2 and np.abs(sh).max() < 1
        y = V.fold(x, V.affines("emptying", 32, 5, mean), np.float32).reshape(-1, 32)
        assert not y[:, 0::4].any() and all(y[:, j].any() for j in range(32) if j % 4), fam
        sc, sh = V.affines("steep", 32, 5, mean)
        assert 100 < np.abs(sc).min() and np.abs(sc).max() < 700 and abs(np.median(np.abs(sc)) - 316) < 80
        y = V.fold(x, (sc, sh), np.float64).reshape(-1, 32)
        live = (y > 0).mean(0)
        assert live.min() > 0.3 and live.max() < 0.7, fam                        # the shift matches: the channel is centred
        assert 50 < y.std(0).min()


# ---- the floor -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", V.FAMILIES)
def test_conv_floor_is_positive_and_the_restatements_meet_the_bound(fam):
    """The reference alone meets the bound the kernels are held to: each float32 restatement within BOUND x the OTHER one's distance
    from float64 (E is the larger of the two, so within E trivially)."""
    worst = 0.0
    for case, tr in [(c, False) for c in V.CONV_CASES] + [(c, True) for c in V.DECONV_CASES]:
        for aff in (None,) + (V.AFFINES if fam in V.FUSED_FAMILIES else ()):
            c = V.conv_case(case, fam, aff, tr)
            x32 = V.conv_input(c["x"], c["aff"], c["x2"], c["aff2"], np.float32)
            d = [V.dist(y, c["e64"]) for y in V.conv_restatements32(x32, c["w"], c["stride"], tr)]
            assert c["E"] == max(d) and min(d) > 0, (case, aff)
            assert d[1] <= V.BOUND * d[0] and d[0] <= V.BOUND * d[1], (case, aff, d)       # oracle and per-tap matmuls: alike
            worst = max(worst, d[2] / min(d))
            assert c["E"] < 1e-5 * np.abs(c["e64"]).max(), (case, aff)            # a float32 floor, not a loose one
            assert c["E_bn"] >= V.floor("bn", c["e64"], c["gamma"], c["beta"])[1] > 0
    print("%s: the running accumulator stands at up to %.1f x the matmul restatements" % (fam, worst))


@pytest.mark.parametrize("fam", V.FAMILIES)
def test_pair_floor_and_the_winograd_restatement(fam):
    for shape in V.PAIR_SHAPES:
        c = V.pair_case(shape, fam)
        assert c["E1"] > 0 and c["E2"] > 0 and c["E_bn1"] > 0 and c["E_bn2"] > 0
        print("pair %s %-13s: E1 %.3g, float32 F(2,3) restatement %.2f E" % (shape, fam, c["E1"], c["wino_over_E"]))
        assert c["wino_over_E"] <= V.BOUND                                          # the formula itself can meet the bound


def test_winograd_restatement_equals_the_direct_one_on_integers():
    rs = np.random.RandomState(9)
    x = rs.randint(-3, 4, (4, 6, 10, 32)).astype(np.float32)
    w = (2 * rs.randint(-2, 3, (3, 3, 3, 32, 8))).astype(np.float32)            # even: the halved sums stay integers
    e = O.conv3d_same(x, w, 1, np.float64)
    assert np.array_equal(V.conv_winograd32(x, w), e) and all(np.array_equal(y, e) for y in V.conv_restatements32(x, w, 1))
    wt = np.ascontiguousarray(np.swapaxes(w, 3, 4))
    et = O.conv3d_transpose_same(x, wt, 2, np.float64)
    assert all(np.array_equal(y, et) for y in V.conv_restatements32(x, wt, 2, True))


def test_other_floors_are_positive():
    for fam in V.FAMILIES:
        for mode, shape in (("normal", (8, 16, 16)),):
            params = S.make_regnet_params(mode, seed=11, random_affine=True)
            cost = V.family(fam, shape + (32,), 12)
            e64, E = V.floor("regnet", cost, params)
            assert E > 0 and np.isfinite(e64).all()
            print("regnet %-13s: E %.3g, rms %.3g" % (fam, E, float(np.sqrt((e64 ** 2).mean()))))
    for D in (8, 64, 481):
        reg = V.softargmin_columns(D)
        for inverse in (False, True):
            (d64, p64, ok), (Ed, Ep) = V.floor("softargmin", reg, 100.0, 2.0, inverse)
            assert np.isfinite(d64).all() and np.isfinite(p64).all() and Ed > 0
            assert (p64 > 0).all() and 0 < Ep < 1e-5 and ok.sum() >= 6, (D, inverse, Ep, int(ok.sum()))
            if not inverse:
                assert not ok[0, :4].any()          # the one-hot columns sit ON a plane: their buckets hang on a rounding
    for fam in ("offset", "range"):
        f = V.family(fam, (3, 9, 20, 32), 2)
        for variant in ("mem", "eager"):
            e64, E = V.floor("variance", f[0], [f[1], f[2]], 3, variant)
            assert E > 0 and e64.min() > -1e-6 * np.abs(e64).max()


def test_softargmin_columns_hold_the_hand_cases():
    for D in (8, 64, 481):
        reg = V.softargmin_columns(D).astype(np.float64)
        assert reg.shape == (D, 3, 5)
        for j, k in enumerate((0, D // 2, D - 1)):
            assert reg[:, 0, j].argmin() == k and np.sort(reg[:, 0, j])[1] - reg[k, 0, j] > 90
        assert np.ptp(reg[:, 0, 4]) == 0 and np.ptp(reg[:, 1, 4]) == 0 and reg[0, 1, 4] == 1e4
        for j, (a, b) in enumerate(((0, 1), (D // 2 - 1, D // 2), (D - 2, D - 1), (0, D - 1))):
            col = reg[:, 1, j]
            assert col[a] == col[b] == col.min() and (col == col.min()).sum() == 2
        assert reg[:, 2, 0].min() > 9990 and np.abs(reg[:, 2, 2]).max() > 40
        # the oracle is exact on the one-hot and the tied columns: a plane 100 (50) lower leaves exp(-100) for the others
        d64, p64 = O.softargmin_and_prob(reg, D, 100.0, 2.0, False, np.float64)
        assert abs(d64[0, 3] - (100.0 + 2.0 * (D // 2))) < 1e-12 and abs(d64[1, 0] - 101.0) < 1e-12
        assert abs(d64[1, 3] - (100.0 + (D - 1))) < 1e-9
        assert abs(d64[0, 4] - (100.0 + (D - 1))) < 1e-9                          # all equal: the mean depth


# ---- ratio weights -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,cout", [((8, 8, 16, 32), 8), ((6, 16, 32, 16), 16), ((12, 8, 32, 32), 8)])
def test_ratio_weights_ratio_is_pinned(shape, cout):
    x, w, ratio = V.ratio_case(shape, cout, 17)
    y = O.conv3d_same(x, w, 1, np.float64)
    r = V.channel_ratio(y)
    print("ratio %s -> %d: median %.2f, channels %.2f .. %.2f, offset %.3f" % (shape, cout, ratio, r.min(), r.max(), float(x.mean())))
    assert abs(ratio - 16.0) <= 4.0                                                 # 16 +- 25 %
    assert r.min() > 8.4                                                            # every channel beyond the largest observed
    assert np.abs(w[1, 1, 1]).sum() > 5 * (np.abs(w).sum() - np.abs(w[1, 1, 1]).sum()) / 26


# ---- BatchNorm sum model -------------------------------------------------------------------------------------------------------
def test_partial_sum_model_grows_with_run_length_and_ratio():
    rs = np.random.RandomState(5)
    y0 = rs.standard_normal((32, 16, 32, 8))
    gamma, beta = np.ones(8, np.float32), np.zeros(8, np.float32)
    err = {}
    for ratio in (0.0, 16.0):
        y = y0 + ratio
        bn64 = O.batch_norm_train(y, gamma, beta, V.BN_EPS, True, np.float64)
        for planes in (2, 32):
            err[ratio, planes] = V.dist(V.partial_sum_model(y, planes, 2, gamma, beta), bn64)
        # sums carried in float64 throughout reproduce the float64 BatchNorm
        flat = y.reshape(-1, 8)
        assert V.dist(V.bn_from_sums(y, flat.sum(0), (flat ** 2).sum(0), gamma, beta), bn64) < 1e-9
    print("partial-sum model, error on the BatchNorm output:", {k: "%.3g" % v for k, v in err.items()})
    assert err[16.0, 32] > err[16.0, 2] and err[16.0, 32] > 10 * err[0.0, 32]
    assert err[0.0, 2] < 2e-7
    full = V.full_size_planes()                 # the launchers' own rule at 192 x 128 x 160 (and 96 x 64 x 80), ported
    assert full == {"c8": 64, "pair_direct": 64, "wino": 64, "s1_16_16": 16}
