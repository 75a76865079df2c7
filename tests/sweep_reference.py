"""Per-plane scores of the recurrent winner-take-all sweep from the numpy oracle, the every-pixel rule the device is held to,
and the inputs the sweep tests share (tests/test_sweep_reference_host.py on the CPU, tests/test_gpu_sweep_every_pixel.py and the
sweep tests of tests/test_gpu_parity.py on the GPU).

The sweep's result per pixel is an arg-max over D plane scores reg[d] (prob_conv of cell 3's state, mvsnet/model.py:701-703) and
max exp(reg) / (sum exp(reg) + 1e-7).  Comparing the arg-max with the oracle's pixel by pixel needs an allowance for near-ties,
and an allowance in PIXELS (the older tests let 2-3 % of them differ) also lets a whole wrong image column through.  The scores
make the allowance a matter of arithmetic instead:

    E = max |reg32 - reg64|      the float32 CPU oracle's worst distance from the float64 one, over all planes and pixels

and a device score may stand up to 2 E from float64 (the sweep's rule, tests/test_gpu_full_size.py; measured 1.8 at c3).  With
every score within 2 E,

  * winner:  the plane p the device chose (its depth value identifies it) has  max_d reg64[d] - reg64[p] <= 4 E  -- the chosen
    plane's device score is at least the true winner's device score, and each of the two is off by at most 2 E;
  * prob:    log(max/sum) moves by at most 2 E for the maximum and 2 E for the log-sum, so |prob - p64| / p64 <= 4 E to first
    order, and max/sum is continuous across a flip of the winner: no pixel needs excluding.

The bound comes from the reference alone.  tests/test_sweep_reference_host.py shows that the float32 oracle and a float32 sweep
whose sigmoid, tanh and cell outputs are perturbed by up to 4 ulp (the device's v_exp / v_rcp activations are ~2 ulp) stay
inside it on every case below, and that planted faults do not."""
from __future__ import annotations

import numpy as np

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S

BOUND = 4.0                       # multiples of E, both assertions
DEPTH_START = 425.0
DEPTH_RANGE = 480.0               # the 'small' workload's total range (16 planes x 30): samples stay inside the image


# ---- shared inputs ---------------------------------------------------------------------------------------------------------
def depth_end(D, depth_range=DEPTH_RANGE):
    return DEPTH_START + depth_range * (D - 1) / D


def small_cams():
    return S.make_workload("small").cams


def features(H, W, C=32, seed=0):
    """S.make_features at the 'small' workload's 3 x 32 x 48, cropped: seed 0, C = 32 are that workload's own maps."""
    return np.ascontiguousarray(S.make_features(3, 32, 48, C, seed)[:, :H, :W])


def gru_params(cin, filters, seed=7):
    """As S.make_gru_params(random_affine=True) builds them, for any three filter counts."""
    rs = np.random.RandomState(seed)
    params = {}
    he = lambda shape, fan_in: (rs.standard_normal(shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)
    for i, F in enumerate(filters, start=1):
        c = cin + F
        p = {"gates_w": he((3, 3, c, 2 * F), 9 * c), "out_w": he((3, 3, c, F), 9 * c)}
        for nm, n in (("gates_b", 2 * F), ("out_b", F)):
            p[nm] = (0.05 * rs.standard_normal(n)).astype(np.float32)
        for nm in ("reset", "update", "out"):
            p[nm + "_gamma"] = (1 + 0.2 * rs.standard_normal(F)).astype(np.float32)
            p[nm + "_beta"] = (0.1 * rs.standard_normal(F)).astype(np.float32)
        params["gru%d" % i] = p
        cin = F
    params["prob_w"] = he((3, 3, cin, 1), 9 * cin)
    params["prob_b"] = (0.05 * rs.standard_normal(1)).astype(np.float32)
    return params


# width -> (feature channels, GRU parameters).  'lite' and 'fat' are what S.make_gru_params gives those modes (model.py:641-645
# halves the filter counts for every mode but 'normal': 8 / 2 / 1); 'wide' is the fat variant of include/mvsnet_hip.h, 32 / 8 / 4;
# 'odd' is hand-made: no cell has a specialised kernel and prob_conv goes through the generic convolution + mvs_wta_update_f32.
_PARAMS = {}


def width_params(width):
    if width not in _PARAMS:
        if width in ("normal", "lite", "fat"):
            C = 4 * S.base_filter(width)
            _PARAMS[width] = (C, S.make_gru_params(width, seed=7, in_channels=C, random_affine=True))
        elif width == "wide":
            _PARAMS[width] = (64, gru_params(64, (32, 8, 4)))
        elif width == "odd":
            _PARAMS[width] = (16, gru_params(16, (12, 6, 3)))
        else:
            raise KeyError(width)
    return _PARAMS[width]


# (H, W, D) of the 'normal' width, one view, feature seed 0 -- what each reaches is in test_gpu_sweep_every_pixel.py
NORMAL_SHAPES = [(27, 41, 16), (9, 47, 16), (31, 17, 16), (5, 11, 17), (21, 37, 19), (19, 35, 2), (19, 35, 3), (19, 35, 4),
                 (19, 35, 70), (19, 35, 83), (17, 33, 130)]
WIDTH_SHAPES = [(27, 41, 16), (19, 35, 19)]          # 'lite' and 'fat', views 0 and 1
VIEW_RANGES = (480.0, 420.0, 360.0)                  # several views per sweep: view v has feature seed v and this depth range


def case(width, H, W, D, view=0, cams=None):
    """-> dict(features, cams, D, start, end, gp, C): view v of a case has feature seed v and depth range VIEW_RANGES[v].
    `cams`: other cameras than the 'small' workload's (3 views at 32 x 48, as family_cams gives them)."""
    C, gp = width_params(width)
    return dict(features=features(H, W, C, seed=view), cams=small_cams() if cams is None else cams, D=D, start=DEPTH_START,
                end=depth_end(D, VIEW_RANGES[view]), gp=gp, C=C, key=(width, H, W, D, view))


CAMERA_FAMILIES = ("roll90", "random3")              # tests/camera_families.py: the sweep under a turned image and a random pose
CAMERA_SHAPE = (27, 41, 16)


def family_cams(name):
    """The family's cameras at the 'small' workload's 3 views and 32 x 48 pixels."""
    from tests import camera_families as CF
    return CF.make_family_cams(name, 3, 32, 48, 16)


def all_cases():
    """Every (width, H, W, D, view) the GPU file runs; the host file proves the reference inside the bound on each."""
    out = [("normal", H, W, D, 0) for H, W, D in NORMAL_SHAPES]
    out += [("normal", 27, 41, 16, v) for v in (1, 2)]
    out += [(m, H, W, D, v) for m in ("lite", "fat") for H, W, D in WIDTH_SHAPES for v in (0, 1)]
    out += [("odd", 27, 41, 16, 0), ("wide", 27, 41, 16, 0), ("wide", 27, 41, 16, 1), ("normal", 19, 35, 1, 0)]
    return out


# ---- the sweep, restated with the places a kernel can go wrong exposed ------------------------------------------------------
def perturb_ulps(rs, ulps=4):
    """-> f(x): every float32 element moved by a random whole number of ulps in [-ulps, ulps]."""
    def f(x):
        x = np.ascontiguousarray(x, np.float32)
        k = rs.randint(-ulps, ulps + 1, size=x.shape).astype(np.int32)
        return (x.view(np.int32) + k).view(np.float32)
    return f


def _layer_norm(x, gamma, beta, dtype, count):
    if count is None:
        return O.layer_norm(x, gamma, beta, dtype=dtype)
    x64 = np.asarray(x, dtype).astype(np.float64)               # the kernels' form: sums over the pixels, divided by a count
    mean = x64.sum() / count
    var = max((x64 * x64).sum() / count - mean * mean, 0.0)
    inv = np.asarray(gamma, np.float64) / np.sqrt(var + 1e-12)
    return (x * inv.astype(dtype) + (np.asarray(beta, np.float64) - mean * inv).astype(dtype)).astype(dtype)


def _cell(x, h, p, dtype, act, count, conv):
    """O.conv_gru_cell (convgru.py:82-122) with hooks: act(values) after each sigmoid / tanh / cell output, count(F) = the
    element count the LayerNorm moments are divided by, conv(inputs, w, b) = the convolution."""
    F = h.shape[-1]
    n = None if count is None else count(F)
    g = conv(np.concatenate([x, h], axis=-1), p["gates_w"], p["gates_b"])
    r = act(O._sigmoid(_layer_norm(g[..., :F], p["reset_gamma"], p["reset_beta"], dtype, n)).astype(dtype))
    u = act(O._sigmoid(_layer_norm(g[..., F:], p["update_gamma"], p["update_beta"], dtype, n)).astype(dtype))
    c = conv(np.concatenate([x, r * h], axis=-1), p["out_w"], p["out_b"])
    y = act(np.tanh(_layer_norm(c, p["out_gamma"], p["out_beta"], dtype, n)).astype(dtype))
    return act((u * h + (dtype(1) - u) * y).astype(dtype))


def plane_depths(D, start, end, inverse, dtype):
    if D == 1:                                         # the loop's formula divides by D - 1; one plane sits at depth_start
        return np.asarray([start], dtype)
    return O.wta_depths(D, start, end, inverse, dtype)


def _homographies(cams, D, start, end, inverse, dtype):
    if D == 1:
        return np.stack([O.get_homographies(cams[0], cams[v], 1, start, 0.0, dtype) for v in range(1, len(cams))])
    Hs = []
    for v in range(1, len(cams)):
        if inverse:
            Hs.append(O.get_homographies_inv_depth(cams[0], cams[v], D, start, end, dtype))
        else:
            Hs.append(O.get_homographies(cams[0], cams[v], D, start, (dtype(end) - dtype(start)) / (dtype(D) - dtype(1)), dtype))
    return np.stack(Hs)


def sweep(feats, cams, D, start, end, gp, inverse=False, dtype=np.float32, act=None, ln_count=None, conv1=None):
    """O.inference_winner_take_all_from_features(return_scores=True) restated over the hooks of _cell (bit-identical without
    them, D = 1 included: one plane at depth_start).  conv1 replaces cell 1's convolution.  -> depth, prob, reg (D,H,W)."""
    feats = np.asarray(feats, dtype)
    N = feats.shape[0]
    Hs = _homographies(cams, D, start, end, inverse, dtype)
    depths = plane_depths(D, start, end, inverse, dtype)
    if act is None and ln_count is None and conv1 is None:
        return O.winner_take_all(feats[0], feats[1:], Hs, depths, gp, N, dtype, return_scores=True)
    ident = lambda x: x
    conv = lambda x, w, b: O.conv2d_same(x, w, 1, b, dtype)
    Hh, W, _ = feats[0].shape
    s = [np.zeros((Hh, W, gp["gru%d" % k]["out_b"].shape[0]), dtype) for k in (1, 2, 3)]
    exp_sum = np.zeros((Hh, W), dtype); depth_image = np.zeros((Hh, W), dtype); max_prob = np.zeros((Hh, W), dtype)
    scores = []
    for d in range(D):
        warped = [O.tf_transform_homography(feats[v + 1], Hs[v, d], dtype) for v in range(N - 1)]
        x = -O.variance_cost_eager(feats[0], warped, N, dtype)
        for k in range(3):
            s[k] = _cell(x, s[k], gp["gru%d" % (k + 1)], dtype, act or ident, ln_count, (conv1 if k == 0 and conv1 else conv))
            x = s[k]
        reg = O.conv2d_same(x, gp["prob_w"], 1, gp["prob_b"], dtype)[..., 0]
        prob = np.exp(reg).astype(dtype)
        upd = max_prob < prob
        max_prob = np.where(upd, prob, max_prob)
        depth_image = np.where(upd, dtype(depths[d]), depth_image)
        exp_sum = exp_sum + prob
        scores.append(reg)
    return depth_image.astype(dtype), (max_prob / (exp_sum + dtype(1e-7))).astype(dtype), np.stack(scores).astype(dtype)


# ---- the reference and the rule ----------------------------------------------------------------------------------------------
class Scores:
    """reg64 / reg32 (D,H,W), depths (D,) float32 plane depth values, E, and the float32 oracle's own depth / prob."""

    def __init__(self, reg64, reg32, depths, depth32=None, prob32=None):
        self.reg64 = np.asarray(reg64, np.float64)
        self.reg32 = np.asarray(reg32, np.float32)
        self.depths = np.asarray(depths, np.float32)
        self.E = float(np.abs(self.reg32.astype(np.float64) - self.reg64).max())
        self.depth32, self.prob32 = depth32, prob32
        e = np.exp(self.reg64)
        self.p64 = e.max(0) / (e.sum(0) + 1e-7)


_CACHE = {}


def plane_scores(features, cams, D, start, end, gp, inverse=False):
    """-> Scores of one input, cached by the arguments' contents (many routes share one input; nobody writes to the arrays)."""
    import hashlib
    h = hashlib.sha1()
    for a in (features, cams):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    for k in ("gru1", "gru2", "gru3"):
        for name in sorted(gp[k]):
            h.update(np.ascontiguousarray(gp[k][name], np.float32).tobytes())
    h.update(gp["prob_w"].tobytes()); h.update(gp["prob_b"].tobytes())
    key = (h.hexdigest(), np.asarray(features).shape, int(D), float(start), float(end), bool(inverse))
    if key not in _CACHE:
        _d64, _p64, reg64 = sweep(features, cams, D, start, end, gp, inverse, np.float64)
        d32, p32, reg32 = sweep(features, cams, D, start, end, gp, inverse, np.float32)
        for a in (reg64, reg32, d32, p32):
            a.setflags(write=False)
        _CACHE[key] = Scores(reg64, reg32, plane_depths(D, start, end, inverse, np.float32), d32, p32)
    return _CACHE[key]


def case_scores(width, H, W, D, view=0, cams=None):
    c = case(width, H, W, D, view, cams)
    return c, plane_scores(c["features"], c["cams"], c["D"], c["start"], c["end"], c["gp"], False)


def measure(depth, prob, ref):
    """-> (plane (H,W) int, -1 where the depth is no plane's; regret (H,W); prob distance (H,W)), the last two in units of E."""
    depth = np.asarray(depth, np.float64); prob = np.asarray(prob, np.float64)
    assert depth.shape == ref.reg64.shape[1:] == prob.shape, (depth.shape, prob.shape, ref.reg64.shape)
    dv = ref.depths.astype(np.float64)
    near = np.abs(depth[None] - dv[:, None, None]) <= 1e-6 * np.abs(dv[:, None, None])
    plane = np.where(near.any(0), near.argmax(0), -1)
    chosen = np.take_along_axis(ref.reg64, np.maximum(plane, 0)[None], 0)[0]
    regret = (ref.reg64.max(0) - chosen) / ref.E
    pdist = np.abs(prob - ref.p64) / ref.p64 / ref.E
    return plane, regret, pdist


def check_every_pixel(depth, prob, ref, tag):
    """Every pixel, none excluded: the depth is a plane's depth value (1e-6 relative), that plane's float64 score is within
    4 E of the best plane's, it is the FIRST of the planes that share its float64 score bit for bit (strict '<', model.py:721),
    and prob is within 4 E, relative, of max exp / (sum exp + 1e-7) of the float64 scores.  Prints both as multiples of E."""
    plane, regret, pdist = measure(depth, prob, ref)
    ok = plane >= 0
    print("%s: E = %.3g  regret %.3f E  prob %.3f E  (%d x %d x %d)" % (
        tag, ref.E, float(regret[ok].max()) if ok.any() else float("nan"), float(pdist.max()), *ref.reg64.shape))
    assert ok.all(), "%s: %d pixel(s) hold a depth that is no plane's depth value, first at %s: %r" % (
        tag, int((~ok).sum()), tuple(np.argwhere(~ok)[0]), float(np.asarray(depth)[tuple(np.argwhere(~ok)[0])]))
    assert np.isfinite(np.asarray(prob)).all(), "%s: prob is not finite" % tag
    worst = np.unravel_index(regret.argmax(), regret.shape)
    assert regret.max() <= BOUND, "%s: winner regret %.3f E > %g E at pixel %s (plane %d, %d pixel(s) over)" % (
        tag, regret.max(), BOUND, worst, plane[worst], int((regret > BOUND).sum()))
    chosen = np.take_along_axis(ref.reg64, plane[None], 0)
    first = (ref.reg64 == chosen).argmax(0)
    late = first < plane
    assert not late.any(), "%s: %d pixel(s) took a later one of bit-equal planes (strict '<' keeps the first), first at %s" % (
        tag, int(late.sum()), tuple(np.argwhere(late)[0]))
    worst = np.unravel_index(pdist.argmax(), pdist.shape)
    assert pdist.max() <= BOUND, "%s: prob %.3f E > %g E from max/sum of the float64 scores at pixel %s (%d pixel(s) over)" % (
        tag, pdist.max(), BOUND, worst, int((pdist > BOUND).sum()))
    return float(regret.max()), float(pdist.max())


def old_rule(depth, prob, ed, ep, share=0.97, rtol=5e-4):
    """What the small-shape sweep tests asserted before: -> True when it passes."""
    same = np.abs(depth - ed) <= 1e-6 * np.abs(ed)
    return bool(same.mean() > share and np.allclose(prob[same], ep[same], rtol=rtol, atol=0.0))
