"""Ill-conditioned inputs for the hot-path kernels and the float32 floor they are held to (host only: numpy and the oracle).

The parity tests draw every tensor from N(0, 1) with unit-gain weights and affines near (1, 0); their tolerances sit 30-100 times
above what float32 costs there.  This module names the value ranges a trained network produces instead (FAMILIES, AFFINES,
ratio_weights) and gives each input its own yardstick, as tests/sweep_reference.py does for the recurrent sweep:

    e64 = the float64 oracle on that very input            E = max |e32 - e64|,  e32 a float32 restatement of the same operation

and a kernel is held to max |got - e64| <= BOUND * E with BOUND = 4.  tests/test_value_cases_host.py shows on the CPU that the
float32 restatements themselves stay inside that bound; tests/test_gpu_value_conditioning.py holds the kernels to it.

Convolutions have three restatements and E is the largest distance: the oracle at float32 (oracle/mvsnet_oracle.py), conv_taps32 (one
float32 matmul per tap, the 27 added one after the other into a float32 accumulator) and conv_running32 (ONE float32 accumulator per
output that takes the 27 x Cin products one after the other).  The third is there because the first two were measured to be no
floor: numpy's matmul sums the input channels blockwise in SIMD lanes, so its error grows with the logarithm of Cin, while every
kernel -- the library's scalar one, a plain triple loop around one fmaf, as much as the MFMA ones, whose accumulator registers take
four products per instruction -- carries a running sum whose error grows with the square root of 27 x Cin.  On the N(0, 1) control
the scalar kernel stood at 5-7.6 of the matmul restatements' E and the MFMA kernels at the same figures; against the running
accumulator both stand where a float32 implementation should.  conv_winograd32 restates F(2,3) along w; it is REPORTED only (it
shows what the formula costs) -- the Winograd kernel is held to E like the direct one.

The BatchNorm output induced by a kernel's sums has the same three restatements: the sums of a float32 convolution output differ
from the float64 ones by that output's own rounding, whatever carries the sums, so E is the distance of the BatchNorm built from
exact (float64) sums of each float32 restatement, scale and shift rounded to float32."""
from __future__ import annotations

import numpy as np

from oracle import mvsnet_oracle as O

BOUND = 4.0
BN_EPS = 1e-5
FAMILIES = ("normal", "offset", "variance-like", "range", "dead", "sparse")
AFFINES = ("near-identity", "emptying", "steep")
OFFSET = 64.0


# ---- input families ----------------------------------------------------------------------------------------------------------
def family(name, shape, seed, offset=OFFSET):
    """-> float32 array of `shape` (..., C); the last axis is the channel axis.
      normal         N(0, 1): the control, what every parity test draws
      offset         N(0, 1) + 64: a common offset 64 deviations large
      variance-like  x^2 * exp(2 g_c), g_c ~ N(0, 1) per channel: non-negative, heavy-tailed, channel scales over about three
                     decades -- a variance cost of unnormalised features
      range          N(0, 1) * 2^k_c, k_c uniform in -12 .. 12 per channel
      dead           N(0, 1), every fourth channel exactly 0
      sparse         5 % of the entries are 50 * N(0, 1), the rest exactly 0"""
    rs = np.random.RandomState(seed)
    C = shape[-1]
    x = rs.standard_normal(shape)
    if name == "normal":
        pass
    elif name == "offset":
        x = x + offset
    elif name == "variance-like":
        x = x * x * np.exp(2.0 * rs.standard_normal(C))
    elif name == "range":
        x = x * np.exp2(rs.randint(-12, 13, size=C).astype(np.float64))
    elif name == "dead":
        x[..., 0::4] = 0.0
    elif name == "sparse":
        x = np.where(rs.uniform(size=shape) < 0.05, 50.0 * x, 0.0)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, np.float32)


def affines(name, C, seed, mean=0.0):
    """-> (scale, shift) float32 of a producer BatchNorm that the consumer folds on load: relu(x * scale + shift).
      near-identity  (1 + 0.3 N, 0.2 N): what the parity tests use
      emptying       every fourth channel (scale 0.05, shift -20): negative on every input of the families above (|x| < 400), so
                     ReLU leaves an all-zero channel; the others near-identity
      steep          scale = gamma / sqrt(eps) ~ 316 as for a producer channel of variance 0, shift = beta - mean * scale with `mean`
                     the input's common offset: 316 * (x - mean) + beta, the product cancels against the shift"""
    rs = np.random.RandomState(seed)
    sc = 1 + 0.3 * rs.standard_normal(C)
    sh = 0.2 * rs.standard_normal(C)
    if name == "near-identity":
        pass
    elif name == "emptying":
        sc[0::4] = 0.05
        sh[0::4] = -20.0
    elif name == "steep":
        sc = sc / np.sqrt(BN_EPS)
        sh = sh - mean * sc
    else:
        raise KeyError(name)
    return sc.astype(np.float32), sh.astype(np.float32)


def fold(x, affine, dtype):
    """relu(x * scale + shift) in `dtype`, or x when affine is None."""
    x = np.asarray(x, dtype)
    if affine is None:
        return x
    sc, sh = (np.asarray(a, dtype) for a in affine)
    return np.maximum(x * sc + sh, dtype(0))


def conv_input(x, affine=None, skip=None, skip_affine=None, dtype=np.float64):
    """What a fused conv launch convolves: relu(bn(x)) + relu(bn(skip)), evaluated in `dtype`."""
    xin = fold(x, affine, dtype)
    if skip is not None:
        xin = xin + fold(skip, skip_affine, dtype)
    return xin


# ---- high-ratio weights ------------------------------------------------------------------------------------------------------
def ratio_weights(Cin, Cout, seed):
    """A centre-tap-dominant 3x3x3 kernel: w[1, 1, 1] a fixed positive mixing matrix (every entry (1 + 0.5 u) / Cin, u uniform in
    [-1, 1]) plus random taps of 5 % of its size everywhere.  The centre tap sees no padding, so an input's common offset reaches the
    output as a common offset at the zero-padded borders too."""
    rs = np.random.RandomState(seed)
    w = 0.05 / Cin * rs.standard_normal((3, 3, 3, Cin, Cout))
    w[1, 1, 1] += (1 + 0.5 * rs.uniform(-1, 1, size=(Cin, Cout))) / Cin
    return w.astype(np.float32)


def channel_ratio(y):
    """-> (C,) |mean| / deviation of each channel of a pre-BatchNorm output."""
    y = np.asarray(y, np.float64).reshape(-1, np.shape(y)[-1])
    return np.abs(y.mean(0)) / y.std(0)


def ratio_case(shape, Cout, seed, stride=1, target=16.0):
    """-> x (float32, N(0, 1) + offset), w, achieved ratio: the offset is chosen so that the MEDIAN channel of conv(x, w) in float64
    has |mean| / deviation = target.  conv is linear: y = conv(n) + offset * conv(1), so the ratio is solved by bisection without
    another convolution per step.  16 is twice the largest ratio entering any BatchNorm of the regulariser on the families above
    (8.4; EXPERIMENTS.md)."""
    Cin = shape[-1]
    w = ratio_weights(Cin, Cout, seed)
    noise = family("normal", shape, seed + 1)
    a = O.conv3d_same(noise, w, stride, np.float64)
    b = O.conv3d_same(np.ones(shape), w, stride, np.float64)
    ratio = lambda off: float(np.median(channel_ratio(a + off * b)))
    lo, hi = 0.0, 1.0
    while ratio(hi) < target:
        hi *= 2.0
        assert hi < 1e6, "the border variation of conv(1) caps the ratio below the target"
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ratio(mid) < target else (lo, mid)
    off = np.float32(0.5 * (lo + hi))
    x = (noise + off).astype(np.float32)
    return x, w, float(np.median(channel_ratio(O.conv3d_same(x, w, stride, np.float64))))


# ---- float32 restatements ----------------------------------------------------------------------------------------------------
def conv_taps32(x, w, stride=1, transpose=False):
    """SAME convolution (or its stride-2 transpose), one float32 matmul over the input channels per tap, the taps added one after
    the other into a float32 accumulator.  Layouts as O.convnd_same / O.convnd_transpose_same."""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    nd = x.ndim - 1
    ks = w.shape[:nd]
    if transpose:
        cout = w.shape[nd]
        outs = [x.shape[a] * stride for a in range(nd)]
        pbs = [O.same_pad(outs[a], ks[a], stride)[1] for a in range(nd)]
        acc = np.zeros(tuple((x.shape[a] - 1) * stride + ks[a] for a in range(nd)) + (cout,), np.float32)
        flat = x.reshape(-1, x.shape[-1])
        for k in np.ndindex(*ks):
            sl = tuple(slice(k[a], k[a] + (x.shape[a] - 1) * stride + 1, stride) for a in range(nd))
            acc[sl] = acc[sl] + np.matmul(flat, np.ascontiguousarray(w[k].T)).reshape(x.shape[:-1] + (cout,))
        return np.ascontiguousarray(acc[tuple(slice(pbs[a], pbs[a] + outs[a]) for a in range(nd))])
    cout = w.shape[nd + 1]
    geo = [O.same_pad(x.shape[a], ks[a], stride) for a in range(nd)]
    outs = tuple(g[0] for g in geo)
    xp = np.pad(x, [(g[1], g[2]) for g in geo] + [(0, 0)])
    acc = np.zeros(outs + (cout,), np.float32)
    for k in np.ndindex(*ks):
        sl = tuple(slice(k[a], k[a] + (outs[a] - 1) * stride + 1, stride) for a in range(nd))
        acc = acc + np.matmul(np.ascontiguousarray(xp[sl]).reshape(-1, x.shape[-1]), w[k]).reshape(acc.shape)
    return acc


def conv_running32(x, w, stride=1, transpose=False):
    """The same convolution with one running float32 accumulator per output: the taps in order, within a tap the input channels in
    order, each product rounded and added on its own (no fused multiply-add, no blocking)."""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    nd = x.ndim - 1
    ks = w.shape[:nd]
    cin = x.shape[-1]
    if transpose:
        cout = w.shape[nd]
        outs = [x.shape[a] * stride for a in range(nd)]
        pbs = [O.same_pad(outs[a], ks[a], stride)[1] for a in range(nd)]
        acc = np.zeros(tuple((x.shape[a] - 1) * stride + ks[a] for a in range(nd)) + (cout,), np.float32)
        for k in np.ndindex(*ks):
            sl = tuple(slice(k[a], k[a] + (x.shape[a] - 1) * stride + 1, stride) for a in range(nd))
            part = acc[sl]
            for ci in range(cin):
                part = part + x[..., ci:ci + 1] * w[k][:, ci]
            acc[sl] = part
        return np.ascontiguousarray(acc[tuple(slice(pbs[a], pbs[a] + outs[a]) for a in range(nd))])
    cout = w.shape[nd + 1]
    geo = [O.same_pad(x.shape[a], ks[a], stride) for a in range(nd)]
    outs = tuple(g[0] for g in geo)
    xp = np.pad(x, [(g[1], g[2]) for g in geo] + [(0, 0)])
    acc = np.zeros(outs + (cout,), np.float32)
    for k in np.ndindex(*ks):
        sl = tuple(slice(k[a], k[a] + (outs[a] - 1) * stride + 1, stride) for a in range(nd))
        xs = np.ascontiguousarray(xp[sl])
        for ci in range(cin):
            acc = acc + xs[..., ci:ci + 1] * w[k][ci]
    return acc


def conv_restatements32(x32, w, stride=1, transpose=False):
    """-> the three float32 restatements of one convolution (module docstring)."""
    if transpose:
        first = O.convnd_transpose_same(x32, w, stride, np.float32)
    else:
        first = O.convnd_same(x32, w, stride, np.float32)
    return [first, conv_taps32(x32, w, stride, transpose), conv_running32(x32, w, stride, transpose)]


def conv_winograd32(x, w):
    """3x3x3 SAME stride-1 convolution with F(2,3) along w in float32 (even W): per (kd, kh) the weights become
    g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2 and the four input columns d0..d3 of an output pair become d0 - d2, d1 + d2,
    d2 - d1, d1 - d3; the four products are accumulated over the nine (kd, kh) in float32, then y0 = m0 + m1 + m2,
    y1 = m1 - m2 - m3."""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    D, H, W, Cin = x.shape
    assert W % 2 == 0 and w.shape[:3] == (3, 3, 3)
    Cout = w.shape[4]
    xp = np.pad(x, [(1, 1), (1, 1), (1, 1), (0, 0)])
    d = [xp[:, :, j:j + W:2] for j in range(4)]                       # (D + 2, H + 2, W / 2, Cin) each
    t = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    half = np.float32(0.5)
    m = [np.zeros((D, H, W // 2, Cout), np.float32) for _ in range(4)]
    for kd in range(3):
        for kh in range(3):
            g0, g1, g2 = w[kd, kh, 0], w[kd, kh, 1], w[kd, kh, 2]
            u = [g0, (g0 + g1 + g2) * half, (g0 - g1 + g2) * half, g2]
            for i in range(4):
                a = np.ascontiguousarray(t[i][kd:kd + D, kh:kh + H]).reshape(-1, Cin)
                m[i] = m[i] + np.matmul(a, u[i]).reshape(m[i].shape)
    y = np.empty((D, H, W, Cout), np.float32)
    y[:, :, 0::2] = m[0] + m[1] + m[2]
    y[:, :, 1::2] = m[1] - m[2] - m[3]
    return y


def bn_from_sums(y64, s1, s2, gamma, beta, eps=BN_EPS, f32_affine=False):
    """relu(y64 * scale + shift) in float64, (scale, shift) from the channel sums s1 = sum y, s2 = sum y^2 as bn_affine_finish
    (csrc/conv_common.h) forms them: var = max(s2 / n - mean^2, 0)."""
    y64 = np.asarray(y64, np.float64)
    count = y64.size // y64.shape[-1]
    mean = np.asarray(s1, np.float64) / count
    var = np.maximum(np.asarray(s2, np.float64) / count - mean * mean, 0.0)
    inv = np.asarray(gamma, np.float64) / np.sqrt(var + eps)
    shift = np.asarray(beta, np.float64) - mean * inv
    if f32_affine:                                   # the kernels hand (scale, shift) on as float32
        inv, shift = inv.astype(np.float32).astype(np.float64), shift.astype(np.float32).astype(np.float64)
    return np.maximum(y64 * inv + shift, 0.0)


# Per-lane run lengths of the BatchNorm sums, read from the kernels and their launchers (csrc/):
#   every MFMA conv kernel keeps st_s[4] / st_q[4] per lane: the sums of FOUR output channels, over every voxel the lane retires
#   during its workgroup's depth range.  A workgroup of 256 lanes (the Winograd kernel: its four 3dconv0_1 waves) retires a
#   TH x TW tile of COUT channels per plane, so a lane adds  TH * TW * COUT / (256 * 4)  values per channel and plane:
#     conv3d_c8.hip        TH x TW = 8 x 16, COUT = 8   -> 1        (launch_c8: `tiles`, retire())
#     conv3d_c8_wino.hip   8 x 32 (TW = 32, TH = 8), 8  -> 2
#     conv3d_mfma.hip 16 -> 16: launch_s1<16, 16, 8>, TWG = CONV_TW = 16 -> 8 x 16 x 16 / 1024 = 2
#   times the planes of the range, a.planes_per_wg (conv_pick_planes / the even-chunk loops of launch_c8<true> and
#   mvs_conv3d_c8_wino_s2_launch, ported below; forced with MVS_HOOK_S1_PLANES / MVS_HOOK_PAIR_PLANES).  stats_commit then folds
#   16 or 32 lanes with float32 shuffles before the four wave totals are added in double.
PER_PLANE = {"c8": 1, "wino": 2, "s1_16_16": 2}
FOLD_LANES = 32


def pick_planes(D, wgs_per_chunk, slots=256, even=False):
    """conv_pick_planes (conv_common.h; halo 2) and, with even=True, the fused launches' loop over even chunk lengths."""
    best, best_cost = (2 if even else D), 1 << 60
    for dr in range(2 if even else 1, D + 1, 2 if even else 1):
        wgs = wgs_per_chunk * (-(-D // dr))
        cost = -(-wgs // slots) * (dr + 3)
        if cost < best_cost:
            best, best_cost = dr, cost
    return best


def full_size_planes():
    """Planes per workgroup the launchers choose at the full-size workload (192 x 128 x 160, the half-resolution level 96 x 64 x 80):
    the largest run a lane's float32 partials see.  The pair's SPAN schedule takes ranges of 60; whole chunks, the hook's form, 64."""
    return {"c8": pick_planes(192, (128 // 8) * (160 // 16)),
            "pair_direct": pick_planes(192, (128 // 8) * (160 // 16), even=True),
            "wino": pick_planes(192, (128 // 8) * (160 // 32), even=True),
            "s1_16_16": max(pick_planes(96, (64 // 8) * (80 // 16)), pick_planes(96, (64 // 8) * (80 // 16), even=True))}


def partial_sum_model(y64, planes, per_plane, gamma, beta, eps=BN_EPS):
    """The BatchNorm output induced by float32 per-lane partial sums of y64 (D, H, W, C): the volume is cut into depth ranges of
    `planes`; a lane owns `per_plane` consecutive voxels of a plane and adds their values, and their squares, over the range's
    planes one after the other in float32 (run = planes * per_plane values); FOLD_LANES lanes are then folded pairwise in float32
    and everything above is added in float64.  -> relu(bn) in float64."""
    y64 = np.asarray(y64, np.float64)
    D, C = y64.shape[0], y64.shape[-1]
    y32 = y64.astype(np.float32).reshape(D, -1, C)
    hw = y32.shape[1]
    pad = (-hw) % (per_plane * FOLD_LANES)
    s1 = np.zeros(C); s2 = np.zeros(C)
    for d0 in range(0, D, planes):
        blk = np.pad(y32[d0:d0 + planes], [(0, 0), (0, pad), (0, 0)])                 # zeros add nothing
        p = blk.shape[0]
        runs = blk.reshape(p, -1, per_plane, C).transpose(1, 0, 2, 3).reshape(-1, p * per_plane, C)      # (lanes, run, C)
        s = np.cumsum(runs, axis=1, dtype=np.float32)[:, -1]
        q = np.cumsum(runs * runs, axis=1, dtype=np.float32)[:, -1]
        for _ in range(int(np.log2(FOLD_LANES))):
            s = s[0::2] + s[1::2]
            q = q[0::2] + q[1::2]
        s1 += s.astype(np.float64).sum(0); s2 += q.astype(np.float64).sum(0)
    return bn_from_sums(y64, s1, s2, gamma, beta, eps)


# ---- the floor ---------------------------------------------------------------------------------------------------------------
def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def floor(op, *args, **kw):
    """-> (e64, E) of one operation on one input; E = max |e32 - e64| (module docstring).
      floor("conv", x, w, stride=1, transpose=False, affine=None, skip=None, skip_affine=None[, gamma=, beta=])
      floor("bn", y64, gamma, beta)                           relu(batch norm) of a raw output, float64 sums of y64 itself
      floor("regnet", cost, params)
      floor("softargmin", reg, start, interval, inverse)      -> ((depth64, prob64, well_posed), (E_depth, E_prob))
      floor("variance", ref, warped_list, view_num, variant)  one plane; the views are warped already"""
    return _FLOORS[op](*args, **kw)


def _floor_conv(x, w, stride=1, transpose=False, affine=None, skip=None, skip_affine=None, gamma=None, beta=None):
    """-> (e64, E); with gamma and beta -> (e64, E, bn64, E_bn), the BatchNorm output of e64 and the floor of the one a float32
    convolution's sums induce."""
    stride = 2 if transpose else stride
    conv64 = O.convnd_transpose_same if transpose else O.convnd_same
    e64 = conv64(conv_input(x, affine, skip, skip_affine, np.float64), w, stride, np.float64)
    y32 = conv_restatements32(conv_input(x, affine, skip, skip_affine, np.float32), w, stride, transpose)
    E = max(dist(y, e64) for y in y32)
    if gamma is None:
        return e64, E
    bn64, E_bn = _floor_bn(e64, gamma, beta)
    for y in y32:
        flat = y.astype(np.float64).reshape(-1, y.shape[-1])
        E_bn = max(E_bn, dist(bn_from_sums(e64, flat.sum(0), (flat * flat).sum(0), gamma, beta, f32_affine=True), bn64))
    return e64, E, bn64, E_bn


def _floor_bn(y64, gamma, beta):
    e64 = O.batch_norm_train(y64, gamma, beta, BN_EPS, True, np.float64)
    return e64, dist(O.batch_norm_train(np.asarray(y64, np.float32), gamma, beta, BN_EPS, True, np.float32), e64)


def _floor_regnet(cost, params):
    e64 = O.regnet_us0(cost, params, np.float64)
    return e64, dist(O.regnet_us0(cost, params, np.float32), e64)


def softargmin_well_posed(d64, D, start, interval, inverse, margin=1e-3):
    """(H, W) bool: the pixels whose four probability buckets do not hang on a rounding.  The buckets are floor and ceil of the
    depth's plane index (model.py:83-140); where the float64 index stands within `margin` of a whole number -- a one-hot column
    puts it ON one -- any float32 evaluation, the oracle's included, may take the neighbouring pair and move the probability by
    a whole plane's weight.  Those pixels are held through their depth, and the hand-made ones through their exact values."""
    d64 = np.asarray(d64, np.float64)
    if inverse:
        end = start + (D - 1.0) * interval
        idx = (1.0 / d64 - 1.0 / end) / ((1.0 / start - 1.0 / end) / (D - 1.0))
    else:
        idx = (d64 - start) / interval
    return np.abs(idx - np.round(idx)) > margin


def _floor_softargmin(reg, start, interval, inverse):
    """-> ((depth64, prob64, well_posed), (E_depth, E_prob)); E_prob over the well-posed pixels."""
    D = reg.shape[0]
    d64, p64 = O.softargmin_and_prob(reg, D, start, interval, inverse, np.float64)
    d32, p32 = O.softargmin_and_prob(reg, D, start, interval, inverse, np.float32)
    ok = softargmin_well_posed(d64, D, start, interval, inverse)
    # a correctly rounded float32 result stands up to half an ulp from the float64 one; on hand-made columns the float32 oracle can
    # land exactly, so its distance alone is no floor
    half_ulp = lambda a: 0.5 * float(np.spacing(np.float32(np.abs(a).max())))
    return (d64, p64, ok), (max(dist(d32, d64), half_ulp(d64)), max(dist(p32[ok], p64[ok]), half_ulp(p64[ok])))


def _floor_variance(ref, warped, view_num, variant):
    fn = O.variance_cost_mem if variant == "mem" else O.variance_cost_eager
    e64 = fn(ref, warped, view_num, np.float64)
    return e64, dist(fn(ref, warped, view_num, np.float32), e64)


_FLOORS = {"conv": _floor_conv, "bn": _floor_bn, "regnet": _floor_regnet, "softargmin": _floor_softargmin,
           "variance": _floor_variance}


def in_units(got, e64, E):
    """max |got - e64| / E."""
    return dist(got, e64) / E


def hold(tag, got, e64, E, bound=BOUND):
    """Prints got / E, then asserts it is at most `bound`; E = 0 (an exact reference) demands an exact result."""
    err = dist(got, e64)
    assert np.isfinite(np.asarray(got)).all(), "%s: not finite" % tag
    r = err / E if E > 0 else (0.0 if err == 0 else float("inf"))
    print("%s: got/E = %.3f  (E = %.3g, max |e64| = %.3g)" % (tag, r, E, float(np.abs(e64).max())))
    assert r <= bound, "%s: max |got - e64| = %.3g = %.3f E > %g E (E = %.3g)" % (tag, err, r, bound, E)
    return r


# ---- soft-argmin columns -----------------------------------------------------------------------------------------------------
def softargmin_columns(D, seed=0):
    """reg (D, 3, 5): fifteen columns of logits (softmax over -reg).
      row 0: one plane lower than the rest by 100 (first, middle, last plane, on N(0, 1) noise; the middle one on zeros too),
             and all equal
      row 1: two exactly equal minima 50 below zeros -- adjacent at the front, in the middle, at the back, and at both ends;
             and all equal at 1e4
      row 2: N(0, 1) + 1e4 (twice), N(0, 1) * 30 (twice), N(0, 1) * 30 + 1e4"""
    rs = np.random.RandomState(seed + D)
    reg = np.zeros((D, 3, 5))
    for j, k in enumerate((0, D // 2, D - 1)):
        reg[:, 0, j] = rs.standard_normal(D); reg[k, 0, j] -= 100.0
    reg[D // 2, 0, 3] = -100.0
    reg[:, 0, 4] = 0.75
    for j, (a, b) in enumerate(((0, 1), (D // 2 - 1, D // 2), (D - 2, D - 1), (0, D - 1))):
        reg[a, 1, j] = reg[b, 1, j] = -50.0
    reg[:, 1, 4] = 1e4
    reg[:, 2, 0] = rs.standard_normal(D) + 1e4
    reg[:, 2, 1] = rs.standard_normal(D) + 1e4
    reg[:, 2, 2] = rs.standard_normal(D) * 30
    reg[:, 2, 3] = rs.standard_normal(D) * 30
    reg[:, 2, 4] = rs.standard_normal(D) * 30 + 1e4
    return reg.astype(np.float32)


# ---- the cases both test files run -------------------------------------------------------------------------------------------
# one per kernel file, the smallest of tests/test_gpu_parity.py's CONV_CASES / DECONV_CASES that reaches it
CONV_CASES = [(8, 8, 16, 32, 8, 1), (8, 8, 16, 32, 16, 2), (4, 4, 8, 16, 32, 2), (6, 16, 32, 16, 16, 1), (6, 16, 24, 32, 32, 1),
              (4, 4, 4, 64, 64, 1), (6, 10, 14, 64, 32, 2), (8, 16, 16, 8, 1, 1), (6, 10, 12, 12, 6, 2)]      # D,H,W,Cin,Cout,stride
DECONV_CASES = [(2, 2, 4, 64, 32), (4, 4, 8, 32, 16), (4, 8, 8, 16, 8), (3, 5, 6, 8, 4)]                       # D,H,W,Cin,Cout
FUSED_FAMILIES = ("normal", "offset")
PAIR_SHAPES = [(8, 8, 16), (6, 10, 34)]
_CASES = {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, tuple):
            for a in v:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return d


def conv_case(case, fam, affine=None, transpose=False):
    """One convolution input with its floor, cached (nobody writes to the arrays).  affine = None: plain; a name of AFFINES: the
    producer BatchNorm folded on load and a second, additive input with an affine of the same kind.  Also the BatchNorm output of
    the float64 result (gamma, beta near (1, 0)) with its own floor."""
    key = (tuple(case), fam, affine, transpose)
    if key in _CASES:
        return _CASES[key]
    if transpose:
        D, H, W, Cin, Cout = case
        stride, wshape = 2, (3, 3, 3, Cout, Cin)
    else:
        D, H, W, Cin, Cout, stride = case
        wshape = (3, 3, 3, Cin, Cout)
    seed = sum(case) + 100 * FAMILIES.index(fam) + (1000 * (1 + AFFINES.index(affine)) if affine else 0) + (7 if transpose else 0)
    rs = np.random.RandomState(seed)
    c = dict(x=family(fam, (D, H, W, Cin), seed), w=(rs.standard_normal(wshape) / np.sqrt(27 * Cin)).astype(np.float32),
             stride=stride, transpose=transpose, aff=None, x2=None, aff2=None)
    if affine:
        mean = OFFSET if fam == "offset" else 0.0
        c.update(x2=family(fam, (D, H, W, Cin), seed + 1), aff=affines(affine, Cin, seed + 2, mean), aff2=affines(affine, Cin, seed + 3, mean))
    c["gamma"] = (1 + 0.2 * rs.standard_normal(Cout)).astype(np.float32)
    c["beta"] = (0.1 * rs.standard_normal(Cout)).astype(np.float32)
    c["e64"], c["E"], c["bn64"], c["E_bn"] = floor("conv", c["x"], c["w"], stride, transpose, c["aff"], c["x2"], c["aff2"],
                                                   gamma=c["gamma"], beta=c["beta"])
    _CASES[key] = _frozen(c)
    return c


def pair_case(shape, fam):
    """The fused 3dconv0_1 + 1_0 launch's input: one 32-channel volume, a 32 -> 8 stride-1 and a 32 -> 16 stride-2 kernel."""
    key = ("pair", tuple(shape), fam)
    if key in _CASES:
        return _CASES[key]
    seed = sum(shape) + 100 * FAMILIES.index(fam) + 5
    rs = np.random.RandomState(seed)
    c = dict(x=family(fam, tuple(shape) + (32,), seed))
    c["w1"] = (rs.standard_normal((3, 3, 3, 32, 8)) / np.sqrt(27 * 32)).astype(np.float32)
    c["w2"] = (rs.standard_normal((3, 3, 3, 32, 16)) / np.sqrt(27 * 32)).astype(np.float32)
    for k, n in (("1", 8), ("2", 16)):
        c["gamma" + k] = (1 + 0.2 * rs.standard_normal(n)).astype(np.float32)
        c["beta" + k] = (0.1 * rs.standard_normal(n)).astype(np.float32)
        c["e" + k], c["E" + k], c["bn" + k], c["E_bn" + k] = floor("conv", c["x"], c["w" + k], int(k), gamma=c["gamma" + k], beta=c["beta" + k])
    c["wino_over_E"] = dist(conv_winograd32(c["x"], c["w1"]), c["e1"]) / c["E1"]
    _CASES[key] = _frozen(c)
    return c
