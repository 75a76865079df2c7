"""Hot-path kernels on ill-conditioned values, each held to the float32 floor of its very input (tests/value_cases.py):

    max |got - e64| <= 4 E,      e64 the float64 oracle,  E = max |e32 - e64| of a float32 restatement of the same operation.

The parity tests draw N(0, 1) data with affines near (1, 0) and sit 30-100 E above the floor; here the inputs carry a common offset,
channel scales over decades, dead and sparse channels, emptying and steep producer affines, saturating gates, dominating and tied
soft-argmin planes -- and the bound is the floor's.  Everything goes through the C ABI.  Every test prints got / E (pytest -s); the
table in EXPERIMENTS.md ("Value conditioning") is filled from that output."""
import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S
from mvsnet_amd import _lib as L

from tests import sweep_reference as SR
from tests import value_cases as V

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(DEV)      # (a copy: the cached inputs are read-only)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def taff(a):
    return None if a is None else (t(a[0]), t(a[1]))


def induced_bn(stats, e64, gamma, beta):
    """The BatchNorm output the kernel's float64 sums induce: mvs_bn_finalize_f32 on them, applied to the float64 raw output."""
    from mvsnet_amd.model import bn_finalize
    scale, shift = bn_finalize(stats, e64.size // e64.shape[-1], t(gamma), t(beta))
    return np.maximum(e64 * n(scale).astype(np.float64) + n(shift).astype(np.float64), 0.0)


# ---- 1. convolutions and transposed convolutions ----------------------------------------------------------------------------------
def run_conv(c, impl, hooks=None):
    from mvsnet_amd.model import conv3d
    cout = c["e64"].shape[-1]
    stats = torch.zeros((2, cout), dtype=torch.float64, device=DEV)
    L.set_conv_impl(impl)
    try:
        with L.test_hooks(**(hooks or {})):
            y = n(conv3d(t(c["x"]), t(c["w"]), c["stride"], taff(c["aff"]), None if c["x2"] is None else t(c["x2"]), taff(c["aff2"]),
                         stats, transpose=c["transpose"]))
    finally:
        L.set_conv_impl("auto")
    return y, stats


CONV_IDS = ["conv-%dx%dx%d-%dto%d-s%d" % c for c in V.CONV_CASES] + ["deconv-%dx%dx%d-%dto%d" % c for c in V.DECONV_CASES]


@pytest.mark.parametrize("impl", ["scalar", "auto"])
@pytest.mark.parametrize("case", [(c, False) for c in V.CONV_CASES] + [(c, True) for c in V.DECONV_CASES], ids=CONV_IDS)
def test_conv_value_families(case, impl):
    """Every family plain; `normal` and `offset` with every producer affine folded on load, with the additive skip input.  The raw
    output at 4 E, and the float64 sums through the BatchNorm output they induce at 4 E of the float32 BatchNorm.

    Measured on an MI355X (EXPERIMENTS.md, value-conditioning addendum): every raw output at 0.1 - 2.2 E.  With float32 per-lane
    partials and a float32 lane fold (stats_commit) the induced BatchNorm output stood at 4.6 E on conv 4x4x8 16 -> 32 stride 2,
    auto, offset (|mean| / deviation 6.4) and, on the scalar kernel, at 6.0 E on conv 6x10x14 64 -> 32 stride 2, offset /
    near-identity; both keep their sums in double now."""
    case, transpose = case
    runs = [(f, None) for f in V.FAMILIES] + [(f, a) for f in V.FUSED_FAMILIES for a in V.AFFINES]
    worst = []
    for fam, aff in runs:
        c = V.conv_case(case, fam, aff, transpose)
        y, stats = run_conv(c, impl)
        tag = "%s %s %s %s/%s" % ("deconv" if transpose else "conv", case, impl, fam, aff or "plain")
        assert y.shape == c["e64"].shape, tag
        try:
            V.hold(tag + " raw", y, c["e64"], c["E"])
            V.hold(tag + " bn ", induced_bn(stats, c["e64"], c["gamma"], c["beta"]), c["bn64"], c["E_bn"])
        except AssertionError as e:
            worst.append(str(e))
    assert not worst, "\n".join(worst)


# ---- 2. the fused pair ---------------------------------------------------------------------------------------------------------------
def run_pair(c, hooks):
    from mvsnet_amd.model import conv3d_pair
    s1 = torch.zeros((2, 8), dtype=torch.float64, device=DEV)
    s2 = torch.zeros((2, 16), dtype=torch.float64, device=DEV)
    with L.test_hooks(**hooks):
        y1, y2 = conv3d_pair(t(c["x"]), t(c["w1"]), t(c["w2"]), s1, s2)
        return n(y1), n(y2), s1, s2


PAIR_ROUTES = (("winograd", {}), ("direct", {"pair_direct": 1}), ("waves4", {"pair_waves4": 1}))


@pytest.mark.parametrize("fam", V.FAMILIES)
@pytest.mark.parametrize("shape", V.PAIR_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_pair_value_families(shape, fam):
    """3dconv0_1 + 1_0 on the Winograd route (default), the direct kernel and the four-wave Winograd instantiation: outputs and induced
    BatchNorm outputs at 4 E, and Winograd's got / E at most twice the direct route's.

    Measured on an MI355X: y1 at 0.38 - 0.92 E on the Winograd route against 0.72 - 1.28 E on the direct one (ratio 0.47 - 0.81 on
    every family).  3dconv1_0's induced BatchNorm output stood at 4.7 E on the Winograd routes at 6x10x34 / offset while the
    stride-2 waves kept float32 partials; they are doubles now."""
    c = V.pair_case(shape, fam)
    r = {}
    fails = []
    for name, hooks in PAIR_ROUTES:
        y1, y2, s1, s2 = run_pair(c, hooks)
        tag = "pair %s %s %s" % (shape, fam, name)
        r[name] = V.in_units(y1, c["e1"], c["E1"])
        for what, got, e64, E in (("y1", y1, c["e1"], c["E1"]), ("y2", y2, c["e2"], c["E2"]),
                                  ("bn1", induced_bn(s1, c["e1"], c["gamma1"], c["beta1"]), c["bn1"], c["E_bn1"]),
                                  ("bn2", induced_bn(s2, c["e2"], c["gamma2"], c["beta2"]), c["bn2"], c["E_bn2"])):
            try:
                V.hold("%s %s" % (tag, what), got, e64, E)
            except AssertionError as e:
                fails.append(str(e))
    print("pair %s %s: got/E winograd %.3f, direct %.3f, ratio %.2f; the float32 F(2,3) restatement %.3f"
          % (shape, fam, r["winograd"], r["direct"], r["winograd"] / r["direct"], c["wino_over_E"]))
    assert not fails, "\n".join(fails)
    assert r["winograd"] <= 2.0 * r["direct"], (r["winograd"], r["direct"])
    assert r["waves4"] == r["winograd"]                       # the same bits (include/mvsnet_hip.h)


# ---- 3. BatchNorm sums at ratio 16 ---------------------------------------------------------------------------------------------------
_RATIO = {}


def ratio_case(shape, cout, seed, target=16.0):
    key = (shape, cout, seed, target)
    if key not in _RATIO:
        x, w, ratio = V.ratio_case(shape, cout, seed, target=target)
        rs = np.random.RandomState(seed + 3)
        gamma = (1 + 0.2 * rs.standard_normal(cout)).astype(np.float32); beta = (0.1 * rs.standard_normal(cout)).astype(np.float32)
        e64, E_raw, bn64, E = V.floor("conv", x, w, 1, gamma=gamma, beta=beta)
        _RATIO[key] = dict(x=x, w=w, ratio=ratio, e64=e64, E_raw=E_raw, gamma=gamma, beta=beta, bn64=bn64, E=E, aff=None, x2=None, aff2=None,
                           stride=1, transpose=False, target=target)
    return _RATIO[key]


def hold_sums(tag, c, stats, planes, per_plane, floor_only):
    got = induced_bn(stats, c["e64"], c["gamma"], c["beta"])
    P = V.dist(V.partial_sum_model(c["e64"], planes, per_plane, c["gamma"], c["beta"]), c["bn64"])
    err = V.dist(got, c["bn64"])
    print("%s: ratio %.1f, run %d (%d planes x %d): got/E = %.3f, got/P = %.3f  (E = %.3g, P = %.3g)"
          % (tag, c["ratio"], planes * per_plane, planes, per_plane, err / c["E"], err / P, c["E"], P))
    assert abs(c["ratio"] - c["target"]) <= 0.25 * c["target"]
    bound = V.BOUND * (c["E"] if floor_only else max(c["E"], P))
    assert err <= bound, "%s: induced BatchNorm output off by %.3g = %.2f E = %.2f P" % (tag, err, err / c["E"], err / P)


@pytest.mark.parametrize("target", [16.0, 8.4], ids=["ratio16", "ratio8.4"])
@pytest.mark.parametrize("forced", [False, True], ids=["launcher", "full-size"])
@pytest.mark.parametrize("kernel", ["c8", "s1_16_16", "wino", "pair_direct"])
def test_batchnorm_sums_at_ratio_16(kernel, forced, target):
    """ratio_weights + an offset chosen so that |mean| / deviation of the pre-BatchNorm output is 16 (twice the largest the regulariser
    shows): the float32 per-lane partials (conv3d_c8.hip, conv3d_mfma.hip, conv3d_c8_wino.hip) against partial_sum_model at the
    kernel's run length -- the launcher's own planes per workgroup at this size, and the most the full-size workload takes, forced
    with MVS_HOOK_S1_PLANES / MVS_HOOK_PAIR_PLANES.  Bound: 4 max(E, P), P the model's own error.  The same at ratio 8.4, the largest
    the regulariser shows on any family: there the full-size run length is held to 4 E alone -- beyond it float32 partials would be
    a defect of the kernels, not of the test's input.

    Measured on an MI355X, got / E with float32 per-lane partials and a float32 lane fold, the parent's kernels (got / P):
                      launcher's planes at this size        the full-size planes, forced
                      ratio 8.4        ratio 16             ratio 8.4         ratio 16
      c8              0.66 (1.16)      2.23 (1.76)          6.03 (1.36)       7.07 (0.70)       run 1 / 64
      s1_16_16        1.68 (1.29)      3.51 (1.44)          5.53 (0.73)      10.38 (0.57)       run 2 / 32
      wino            0.90 (1.03)      1.35 (0.51)          7.66 (1.33)      21.06 (1.93)       run 4 / 128
      pair_direct     0.57 (0.90)      1.35 (0.94)          5.16 (1.62)      12.08 (1.20)       run 2 / 64
    The model explained every figure (got / P 0.5 - 1.9), and the four full-size cases at ratio 8.4 missed 4 E.  The kernels now keep
    their per-lane sums and the fold in double: 0.33 - 0.69 E in all sixteen cases, whatever the run length."""
    full = V.full_size_planes()[kernel]
    per_plane = V.PER_PLANE["c8" if kernel == "pair_direct" else kernel]
    if kernel in ("c8", "s1_16_16"):
        cin, cout = (32, 8) if kernel == "c8" else (16, 16)
        D = full if kernel == "c8" else 2 * full
        shape = (D, 8, 16, cin)
        c = ratio_case(shape, cout, 17, target)
        # the launcher's own choice at this size (conv_pick_planes: one tile, `groups` = 1 -> 1 workgroup per chunk)
        planes = full if forced else V.pick_planes(D, 1)
        y, stats = run_conv(c, "auto", {"s1_planes": full} if forced else {})
        V.hold("ratio %s raw" % kernel, y, c["e64"], c["E_raw"])
    else:
        shape = (full, 8, 32, 32)
        c = ratio_case(shape, 8, 17, target)
        tiles = 2 if kernel == "pair_direct" else 1
        planes = full if forced else V.pick_planes(full, tiles, even=True)
        w2 = V.ratio_weights(32, 16, 19)
        hooks = dict({"pair_direct": 1} if kernel == "pair_direct" else {}, **({"pair_planes": full} if forced else {}))
        y1, _y2, stats, _s2 = run_pair(dict(x=c["x"], w1=c["w"], w2=w2), hooks)
        V.hold("ratio %s raw" % kernel, y1, c["e64"], c["E_raw"])
    hold_sums("sums %s %s %s" % (kernel, shape, "forced" if forced else "launcher"), c, stats, planes, per_plane,
              floor_only=forced and target < 16.0)


# ---- 4. RegNetUS0 --------------------------------------------------------------------------------------------------------------------
_REGNET = {}


def regnet_case(mode, shape, fam, dead_gamma=False):
    key = (mode, shape, fam, dead_gamma)
    if key not in _REGNET:
        params = S.make_regnet_params(mode, seed=11, random_affine=True)
        if dead_gamma:
            params = {k: dict(v) for k, v in params.items()}
            g = params["3dconv1_0"]["gamma"].copy(); g[3] = 0.0
            params["3dconv1_0"]["gamma"] = g
        cost = V.family(fam, shape + (4 * S.base_filter(mode),), 12 + V.FAMILIES.index(fam))
        _REGNET[key] = (params, cost) + V.floor("regnet", cost, params)
    return _REGNET[key]


@pytest.mark.parametrize("fam", V.FAMILIES)
@pytest.mark.parametrize("mode,shape", [("normal", (8, 16, 16)), ("lite", (8, 16, 16)), ("normal", (16, 8, 24)), ("lite", (16, 8, 24))])
def test_regnet_value_families(mode, shape, fam):
    from mvsnet_amd.model import RegNetWeights, regnet_us0
    params, cost, e64, E = regnet_case(mode, shape, fam)
    got = n(regnet_us0(t(cost), RegNetWeights(params, DEV, pad_to_mfma=True)))
    V.hold("regnet %s %s %s" % (mode, shape, fam), got, e64, E)


def test_regnet_with_a_dead_channel():
    """gamma = 0 on one channel of 3dconv1_0: its BatchNorm output is beta everywhere, a constant channel -- variance 0 after the
    ReLU in every consumer's view -- through the consumer-side fold of 3dconv1_1 and 3dconv2_0."""
    from mvsnet_amd.model import RegNetWeights, regnet_us0
    params, cost, e64, E = regnet_case("normal", (8, 16, 16), "normal", dead_gamma=True)
    got = n(regnet_us0(t(cost), RegNetWeights(params, DEV)))
    V.hold("regnet, gamma = 0 on 3dconv1_0[3]", got, e64, E)


# ---- 5. soft-argmin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["linear", "inverse"])
@pytest.mark.parametrize("D", [8, 64, 481])
def test_softargmin_columns(D, inverse):
    """Dominating, tied, offset, wide and constant columns (value_cases.softargmin_columns) on both sides of the 480-plane switch
    between the two kernels of softargmin.hip.  Depth at 4 E on every column; probability at 4 E on the columns whose buckets do
    not hang on a rounding (value_cases.softargmin_well_posed).  Start and interval are dyadic, so with linear depths the one-hot
    and the tied columns are exact in float32 and must come out exactly, probability included."""
    from mvsnet_amd.model import softargmin_prob
    start, interval = 100.0, 2.0
    reg = V.softargmin_columns(D)
    (d64, p64, ok), (Ed, Ep) = V.floor("softargmin", reg, start, interval, inverse)
    depth, prob = softargmin_prob(t(reg), start, interval, inverse)
    depth, prob = n(depth), n(prob)
    tag = "softargmin D=%d %s" % (D, "inverse" if inverse else "linear")
    fails = []
    assert ok.sum() >= 6
    for what, got, e64, E in (("depth", depth, d64, Ed), ("prob, %d well-posed columns" % ok.sum(), prob[ok], p64[ok], Ep)):
        try:
            V.hold("%s %s" % (tag, what), got, e64, E)
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
    if not inverse:
        # the one-hot columns (row 0, columns 0-3) and the ties (row 1, columns 0-3): every product and sum is exact in float32
        exact = np.zeros((3, 5), bool); exact[0, :4] = True; exact[1, :4] = True
        assert np.array_equal(depth[exact], d64[exact].astype(np.float32)), (depth[exact], d64[exact])
        z = lambda k: np.float32(start + interval * k)
        assert depth[0, 3] == z(D // 2) and depth[1, 0] == z(0.5) and depth[1, 3] == z((D - 1) / 2)
        exact[1, 3] = False                 # the tie at both ends leaves exp(-50) in its four buckets: held by E above
        assert np.array_equal(prob[exact], p64[exact].astype(np.float32)), (prob[exact], p64[exact])
        assert prob[0, 3] == 2.0 and prob[0, 0] == 3.0 and prob[1, 0] == 1.5 and prob[1, 1] == 1.0      # clamped buckets repeat the end planes


# ---- 6. variance cost ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["offset", "range"])
@pytest.mark.parametrize("views", [2, 5])
@pytest.mark.parametrize("variant", ["mem", "eager"])
def test_variance_cost_value_families(variant, views, fam):
    """Q / N - S^2 / N^2 with features that carry a common offset of 64 deviations, or channel scales over seven decades.  The
    source views are shifted by whole pixels (another shift per view and plane), so the warp is exact and the bound is the
    variance formula's alone."""
    from mvsnet_amd.model import cost_volume
    H, W, Cn, D = 9, 20, 32, 4
    f = V.family(fam, (views, H, W, Cn), 40 + views)
    T = np.zeros((views - 1, D, 8), np.float32)
    T[:, :, 0] = 1; T[:, :, 4] = 1
    for v in range(views - 1):
        for d in range(D):
            T[v, d, 2], T[v, d, 5] = (d + v) % 3 - 1, (2 * d + v) % 3 - 1
    got = n(cost_volume(t(f[0]), t(f[1:]), t(T), variant=variant))
    worst = 0.0
    for d in range(D):
        warped = [O.image_projective_transform_bilinear(f[v + 1], T[v, d].astype(np.float64), np.float64) for v in range(views - 1)]
        assert all(np.array_equal(w_, w_.astype(np.float32)) for w_ in warped)          # whole-pixel shifts: exact
        e64, E = V.floor("variance", f[0], warped, views, variant)
        worst = max(worst, V.hold("variance %s N=%d %s plane %d" % (variant, views, fam, d), got[d], e64, E))
    print("variance %s N=%d %s: worst got/E %.3f" % (variant, views, fam, worst))


# ---- 7. saturating gates ---------------------------------------------------------------------------------------------------------------
SAT_SHAPE = (5, 11, 8)                      # (H, W, D): test_gpu_sweep_every_pixel's smallest size, D = 8


def saturating_params():
    """sweep_reference.gru_params with every layer-norm gain x 32 and the layer-norm biases at +-20: pre-activations of deviation 32
    around +-20, far beyond where exp2's cap and both saturation ends of the fast sigmoid / tanh begin."""
    if "saturating" not in SR._PARAMS:
        gp = SR.gru_params(32, (16, 4, 2), seed=9)
        rs = np.random.RandomState(10)
        for k in ("gru1", "gru2", "gru3"):
            for nm in ("reset", "update", "out"):
                gp[k][nm + "_gamma"] = (32.0 * gp[k][nm + "_gamma"]).astype(np.float32)
                gp[k][nm + "_beta"] = (20.0 * rs.choice([-1.0, 1.0], size=gp[k][nm + "_beta"].shape)).astype(np.float32)
        c = dict(features=SR.features(SAT_SHAPE[0], SAT_SHAPE[1], 32, 0), cams=SR.small_cams())
        _d, _p, reg = SR.sweep(c["features"], c["cams"], SAT_SHAPE[2], SR.DEPTH_START, SR.depth_end(SAT_SHAPE[2]), gp, False, np.float64)
        top = float(np.abs(reg).max())
        if top > 60.0:                      # reg is linear in the last convolution: exp(reg) stays finite as in the reference
            gp["prob_w"] = (gp["prob_w"] * (60.0 / top)).astype(np.float32); gp["prob_b"] = (gp["prob_b"] * (60.0 / top)).astype(np.float32)
        SR._PARAMS["saturating"] = (32, gp)
    return SR._PARAMS["saturating"][1]


def gate_share(gp):
    """Share of reset / update gate values of the float64 sweep beyond sigmoid(+-30), and whether anything is NaN."""
    seen = []
    calls = [0]

    def act(v):
        if calls[0] % 4 < 2:                # _cell calls act on r, u, tanh, output in that order
            seen.append(np.asarray(v, np.float64).ravel())
        calls[0] += 1
        return v
    H, W, D = SAT_SHAPE
    _d, _p, reg = SR.sweep(SR.features(H, W, 32, 0), SR.small_cams(), D, SR.DEPTH_START, SR.depth_end(D), gp, False, np.float64, act=act)
    g = np.concatenate(seen)
    lo = 1.0 / (1.0 + np.exp(30.0))
    return float(((g < lo) | (g > 1.0 - lo)).mean()), reg


SAT_ROUTES = [dict(), dict(gru_one_stream=1), dict(form=1), dict(form=2), dict(form=1, gru_one_stream=1), dict(impl="scalar")]


@pytest.mark.parametrize("route", SAT_ROUTES, ids=["fused", "fused-one-stream", "wavefront1", "wavefront2", "wavefront1-one-stream", "scalar"])
def test_saturating_gates_in_the_sweep(route):
    from tests import test_gpu_sweep_every_pixel as SP
    gp = saturating_params()
    share, reg = gate_share(gp)
    print("saturating gates: %.1f %% of gate values beyond +-30, max |reg| %.2f" % (100 * share, np.abs(reg).max()))
    assert share >= 0.20 and np.isfinite(reg).all() and np.abs(reg).max() <= 60.0
    H, W, D = SAT_SHAPE
    d, p = SP.hold("saturating", H, W, D, tag="saturating %s" % (route,), **route)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(p).all())


# ---- 8. GroupNorm tower layer ------------------------------------------------------------------------------------------------------------
def gn_fold(x, gamma, beta, dtype, eps=1e-5):
    """relu(group norm) as the tower kernels apply it (and as the oracle's BatchNorm does): group moments in float64, then
    x * scale + shift in `dtype`.  O.group_norm_nhwc subtracts the mean in float64 BEFORE it rounds, which no float32 kernel that
    folds the normalisation into one multiply-add can do: at a common offset the fold's cancellation is part of the float32 floor."""
    Hh, W, Cc = x.shape
    xg = x.astype(np.float64).reshape(Hh, W, Cc // 8, 8)
    mean = np.repeat(xg.mean(axis=(0, 1, 3)), 8); var = np.repeat(xg.var(axis=(0, 1, 3)), 8)
    inv = np.asarray(gamma, np.float64) / np.sqrt(var + eps)
    y = np.asarray(x, dtype) * inv.astype(dtype) + (np.asarray(beta, np.float64) - mean * inv).astype(dtype)
    return np.maximum(y, dtype(0))


@pytest.mark.parametrize("persistent", [1, 0])
@pytest.mark.parametrize("fam", ["offset", "dead-group"])
@pytest.mark.parametrize("case", [(2, 16, 32, 16, 32, 3, 2), (1, 16, 32, 16, 32, 5, 2)], ids=["3x3s2", "5x5s2"])      # V,H,W,C1,Cout,k,stride
def test_groupnorm_layer_value_families(case, fam, persistent):
    """mvs_conv2d_gn_f32 with the producer's GroupNorm + ReLU folded on load: an input with a common offset, and one whose second
    group of 8 channels is zero everywhere (variance 0: scale = gamma / sqrt(eps), output beta)."""
    lib = L.load()
    Vn, H, W, C1, Cout, k, stride = case
    rs = np.random.RandomState(sum(case))
    if fam == "offset":
        x = V.family("offset", (Vn, H, W, C1), 50)
    else:
        x = V.family("dead", (Vn, H, W, C1), 51)
        x[..., 8:16] = 0.0
    w = (rs.standard_normal((k, k, C1, Cout)) / np.sqrt(k * k * C1)).astype(np.float32)
    g = (1 + 0.3 * rs.standard_normal(C1)).astype(np.float32); b = (0.2 * rs.standard_normal(C1)).astype(np.float32)
    SL = lib.mvs_gn_stat_slots()
    xs = x.reshape(Vn, -1, C1 // 8, 8).astype(np.float64)
    sums = np.zeros((Vn, C1 // 8, SL, 2)); sums[:, :, 0] = np.stack([xs.sum((1, 3)), (xs ** 2).sum((1, 3))], -1)
    s1 = torch.as_tensor(sums).to(DEV)
    wp = torch.empty(lib.mvs_conv2d_prepared_floats(k, C1, 0, Cout), dtype=torch.float32, device=DEV)
    tw, tx, tg, tb = t(w), t(x), t(g), t(b)
    L.check(lib.mvs_conv2d_prepare_f32(L.ptr(tw), k, C1, 0, Cout, L.ptr(wp), L.stream_ptr()), "prepare")
    y = torch.empty((Vn, -(-H // stride), -(-W // stride), Cout), dtype=torch.float32, device=DEV)
    so = torch.zeros((Vn, Cout // 8, SL, 2), dtype=torch.float64, device=DEV)
    with L.test_hooks(unet_persistent=persistent):
        L.check(lib.mvs_conv2d_gn_f32(L.ptr(tx), L.ptr(s1), L.ptr(tg), L.ptr(tb), C1, 1, None, None, None, None, 0, 0,
                                      L.ptr(wp), Vn, H, W, Cout, k, stride, L.ptr(y), L.ptr(so), L.stream_ptr()), "conv2d")
        got = n(y)
    for v in range(Vn):
        e64 = O.convnd_same(gn_fold(x[v], g, b, np.float64), w, stride, np.float64)
        x32 = gn_fold(x[v], g, b, np.float32)
        E = max(V.dist(y32, e64) for y32 in V.conv_restatements32(x32, w, stride))
        V.hold("conv2d_gn %s %s persistent=%d view %d" % (case, fam, persistent, v), got[v], e64, E)


# ---- 7b. saturating gates in the training cell (gru_train.hip) -----------------------------------------------------------------------------
def test_saturating_gates_in_the_training_cell():
    """mvs_gru_train_cell_fwd_f32 / _bwd_f32 with cell 1 of the saturating parameters, through the machinery of
    test_gpu_backward.test_hip_conv_gru_sweep_matches_the_float64_cell_chain: states and every gradient against the float64 cell
    chain of the checker, E = the same chain (and its autograd) in float32.  tanh_fast = 1 - 2 rcp(exp(2x) + 1) and the sigmoid
    meet both saturation ends here; nothing may be NaN."""
    from mvsnet_amd import gru_train as G
    from oracle import torch_grad as TG
    D, H, W, Cin, Fn = 4, 9, 20, 32, 16
    p = {k: np.asarray(v, np.float32) for k, v in saturating_params()["gru1"].items()}
    rs = np.random.RandomState(21)
    x = rs.standard_normal((D, H, W, Cin)).astype(np.float32)
    gh = rs.standard_normal((D, H, W, Fn)).astype(np.float32)

    def chain(dtype):
        cast = lambda a, g=False: torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(g)
        xx, pp = cast(x, True), {k: cast(v, True) for k, v in p.items()}
        h = torch.zeros((1, Fn, H, W), dtype=dtype)
        states = []
        for d in range(D):
            h = TG.conv_gru_cell(xx[d].permute(2, 0, 1)[None], h, pp)
            states.append(h[0].permute(1, 2, 0))
        want = torch.stack(states, 0)
        (want * cast(gh)).sum().backward()
        return want.detach().numpy().astype(np.float64), dict({k: v.grad.numpy().astype(np.float64) for k, v in pp.items()},
                                                                x=xx.grad.numpy().astype(np.float64))
    s64, g64 = chain(torch.float64)
    s32, g32 = chain(torch.float32)
    # the share of saturated gates, from the numpy restatement of the same chain
    seen, calls = [], [0]

    def act(v):
        if calls[0] % 4 < 2:
            seen.append(np.asarray(v, np.float64).ravel())
        calls[0] += 1
        return v
    h = np.zeros((H, W, Fn))
    for d in range(D):
        h = SR._cell(x[d].astype(np.float64), h, p, np.float64, act, None, lambda a, w, b: O.conv2d_same(a, w, 1, b, np.float64))
    gates = np.concatenate(seen)
    lo = 1.0 / (1.0 + np.exp(30.0))
    share = float(((gates < lo) | (gates > 1.0 - lo)).mean())
    print("training cell: %.1f %% of gate values beyond +-30; chain distance numpy / torch %.3g" % (100 * share, V.dist(h, s64[-1])))
    assert share >= 0.20 and V.dist(h, s64[-1]) < 1e-9
    xt = t(x).requires_grad_(True)
    pt = {k: t(v).requires_grad_(True) for k, v in p.items()}
    got = G.conv_gru_sweep_hip(xt, pt)
    (got * t(gh)).sum().backward()
    fails = []
    for name, dev, e64, e32 in [("states", n(got), s64, s32), ("grad x", n(xt.grad), g64["x"], g32["x"])] + \
                               [("grad " + k, n(pt[k].grad), g64[k], g32[k]) for k in sorted(p)]:
        try:
            V.hold("training cell %s" % name, dev, e64, V.dist(e32, e64))
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)
