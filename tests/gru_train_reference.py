"""The recurrent cells' training kernels (mvs_gru_train_cell_fwd_f32 / _bwd_f32) restated with the kernels' own interface.

A plain helper module (no fixtures, no GPU).  Written from ConvGRUCell.__call__ (mvsnet/convgru.py:82-122) and from the ABI comment
above mvs_gru_train_slots in include/mvsnet_hip.h -- not from csrc/gru_train.hip: what the header promises is what is held.

    g[d]   = px[d][.., :2F] + conv3x3(h[d], wgh)                        the raw gate convolution, channels [reset | update]
    r, u   = sigmoid(LN(g_r)), sigmoid(LN(g_u))                         LayerNorm over all H*W*F elements of the plane, eps 1e-12
    rh[d]  = r * h[d]
    c[d]   = px[d][.., 2F:] + conv3x3(rh[d], woh)
    h[d+1] = u * h[d] + (1 - u) * tanh(LN(c[d]))
    stats[d] = (sum g_r, sum g_r^2, sum g_u, sum g_u^2, sum c, sum c^2)   what the kernels keep per slot, folded over the slots

Every gradient is torch autograd of these expressions for the scalar  sum_d <h[d+1], gh[d]>  (+ <h[D], dh_in>): gpx is the gradient
of px, dh_out that of h[0], and `part` that of a per-plane copy of ln -- ln enters as a (D,6,F) leaf, so that the per-plane sums of
dz (beta) and dz * xhat (gamma) come out of autograd: part[d, k, 0] = d beta_k, part[d, k, 1] = d gamma_k (k = reset, update,
candidate), the layout of the kernels' `part` once it is summed over its slots.  Nothing backward is derived by hand.

run(.., dtype=torch.float32) evaluates the same expressions on the CPU in float32: its distance from the float64 run is the float32
floor of the operation, from which tests/test_gru_train_reference_host.py derives BOUNDS (the procedure is floor_fit below).

`defect=` seeds ONE defect of the kind a tiled kernel can have into the reference (the host test shows that each is at least 100
bounds large where it lands, so that a failing GPU test means what it says):

    halo      plane 0's gate convolution of tile (0, 1) sees the h column left of the tile, w = 15, as zero
    ln_rows   plane 0's reset LayerNorm takes its moments without the last, partial tile row (rows >= 2 TH)
    group     not a change of the computation: the last output-channel group of tile (1, 1) compared against zero (unwritten)
    parity    the state gradient entering plane D - 2 from above is the one that entered plane D - 1 (the other ping-pong buffer)
    no_dh_in  dh_in is left out of the scalar
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

LN_EPSILON = 1e-12          # tf.contrib.layers.layer_norm (convgru.py:30-31)
TW = 16                     # tile columns; rows per tile and output-channel groups: tile_of
FILTERS = (16, 8, 4, 2, 1)
MARGIN = 4.0                # over the float32 floor: what tests/test_gpu_value_conditioning.py grants (max |got - e64| <= 4 E)
OUTPUTS = ("g", "c", "rh", "h", "stats", "gpx", "part", "dh_out")
DEFECTS = ("halo", "ln_rows", "group", "parity", "no_dh_in")

Case = collections.namedtuple("Case", "F D H W seed")


def tile_of(Fn):
    """-> (rows, columns, output-channel groups) of a workgroup's tile: TH = 16 / NS rows of 16 pixels, NS = 4, 2, 1 groups."""
    ns = 4 if Fn >= 16 else (2 if Fn >= 8 else 1)
    return 16 // ns, TW, ns


def seam_shape(Fn):
    """The smallest (H, W) at which both tiled axes have two full tiles and a one-pixel remainder."""
    th, tw, _ = tile_of(Fn)
    return 2 * th + 1, 2 * tw + 1


# Seeds moved off 0, {case id: seed}: a property of the float64 reference alone, asserted in the host test (conditioned()).
SEEDS = {}


def case_id(c):
    return "F%d-D%d-%dx%d" % (c.F, c.D, c.H, c.W)


def _case(Fn, D, H, W):
    c = Case(Fn, D, H, W, 0)
    return c._replace(seed=SEEDS.get(case_id(c), 0))


SEAM_CASES = tuple(_case(Fn, D, *seam_shape(Fn)) for Fn in FILTERS for D in (3, 4))
# H*W*F is no multiple of 256 at any of these: the elementwise launches end in a partial block; D = 1 and 2 run nowhere else
NARROW_CASES = tuple(_case(Fn, D, H, W) for Fn in FILTERS for D, H, W in ((2, 1, 17), (2, 17, 1), (1, 5, 7)))
CASES = SEAM_CASES + NARROW_CASES


def shape_class(c):
    return "seam" if (c.H, c.W) == seam_shape(c.F) else "narrow"


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """float32 operands of a case by name, read-only: px, wgh, woh, ln, h0, gh, dh_in."""
    Fn, D, H, W = c.F, c.D, c.H, c.W
    rs = np.random.RandomState(1000 * Fn + 100 * D + 7 * H + W + 100003 * c.seed)
    f32 = np.float32
    a = dict(px=rs.standard_normal((D, H, W, 3 * Fn)).astype(f32),
             wgh=(rs.standard_normal((3, 3, Fn, 2 * Fn)) * (1.5 / np.sqrt(9 * Fn))).astype(f32),
             woh=(rs.standard_normal((3, 3, Fn, Fn)) * (1.5 / np.sqrt(9 * Fn))).astype(f32))
    ln = np.empty((6, Fn), f32)
    ln[0::2] = 1 + 0.3 * rs.standard_normal((3, Fn))          # gammas around 1
    ln[1::2] = 0.2 * rs.standard_normal((3, Fn))              # betas
    h0 = np.tanh(rs.standard_normal((H, W, Fn))).astype(f32)  # a state: inside (-1, 1), non-zero everywhere
    h0[h0 == 0] = 0.5
    a.update(ln=ln, h0=h0, gh=rs.standard_normal((D, H, W, Fn)).astype(f32), dh_in=rs.standard_normal((H, W, Fn)).astype(f32))
    for v in a.values():
        v.setflags(write=False)
    return a


# ---- the expressions ---------------------------------------------------------------------------------------------------------------
def _conv(x, w):
    """x (H,W,Cin), w (3,3,Cin,Cout) in the TensorFlow layout -> (H,W,Cout), 3x3 SAME."""
    return F.conv2d(x.permute(2, 0, 1)[None], w.permute(3, 2, 0, 1), padding=1)[0].permute(1, 2, 0)


def _layer_norm(x, gamma, beta, rows=None):
    """Moments over all elements of x (H,W,F) -- over x[:rows] for the seeded defect -- gamma, beta per channel."""
    m = x if rows is None else x[:rows]
    mean = m.mean()
    var = ((m - mean) ** 2).mean()
    return (x - mean) / torch.sqrt(var + LN_EPSILON) * gamma + beta


def run(px, wgh, woh, ln, h0, gh, dh_in=None, dtype=torch.float64, defect=None):
    """-> {g, c, rh (D,..), h (D+1,..), stats (D,6), var (D,3), gpx (D,H,W,3F), part (D,3,2,F), dh_out (H,W,F)} as float64
    numpy arrays, computed in `dtype` on the CPU."""
    assert defect in (None, "halo", "ln_rows", "parity", "no_dh_in")
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    D, H, W, Fn = np.asarray(gh).shape
    th, tw, _ = tile_of(Fn)
    px_t, h0_t = t(px).requires_grad_(True), t(h0).requires_grad_(True)
    ln_t = t(ln)[None].repeat(D, 1, 1).requires_grad_(True)               # a copy per plane: per-plane gamma / beta gradients
    wgh_t, woh_t, gh_t = t(wgh), t(woh), t(gh)
    dh_in_t = None if dh_in is None or defect == "no_dh_in" else t(dh_in)
    h, hs, gs, cs, rhs, stats, var = h0_t, [h0_t], [], [], [], [], []
    for d in range(D):
        g = px_t[d][..., :2 * Fn] + _conv(h, wgh_t)                                            # convgru.py:89-94
        if defect == "halo" and d == 0:
            only = torch.zeros_like(h)
            only[:th, tw - 1] = h[:th, tw - 1]
            miss = torch.zeros_like(g)
            miss[:th, tw] = _conv(only, wgh_t)[:th, tw]
            g = g - miss
        gr, gu = g[..., :Fn], g[..., Fn:]
        rows = 2 * th if defect == "ln_rows" and d == 0 else None
        r = torch.sigmoid(_layer_norm(gr, ln_t[d, 0], ln_t[d, 1], rows))                       # :97,101
        u = torch.sigmoid(_layer_norm(gu, ln_t[d, 2], ln_t[d, 3]))                             # :98,102
        rh = r * h
        c = px_t[d][..., 2 * Fn:] + _conv(rh, woh_t)                                           # :107-111
        y = torch.tanh(_layer_norm(c, ln_t[d, 4], ln_t[d, 5]))                                 # :114-117
        h = u * h + (1.0 - u) * y                                                              # :120
        gs.append(g); cs.append(c); rhs.append(rh); hs.append(h)
        parts = (gr[:rows] if rows else gr, gu, c)
        stats.append(torch.stack([s for x in parts for s in (x.sum(), (x * x).sum())]))
        var.append(torch.stack([((x - x.mean()) ** 2).mean() for x in (gr, gu, c)]))
    total = sum((hs[d + 1] * gh_t[d]).sum() for d in range(D))
    if dh_in_t is not None:
        total = total + (hs[D] * dh_in_t).sum()
    if defect == "parity" and D >= 2:
        # what reaches h[D-1] from above is replaced by what reached h[D] from above (dh_in or nothing): autograd plumbing only
        stale = dh_in_t if dh_in_t is not None else torch.zeros_like(h0_t)
        hs[D - 1].register_hook(lambda grad: gh_t[D - 2] + stale)
    total.backward()
    out = dict(g=torch.stack(gs), c=torch.stack(cs), rh=torch.stack(rhs), h=torch.stack(hs), stats=torch.stack(stats),
               var=torch.stack(var), gpx=px_t.grad, dh_out=h0_t.grad,
               part=torch.stack([ln_t.grad[:, 1::2], ln_t.grad[:, 0::2]], 2))                 # (D, 3, [d beta, d gamma], F)
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def expect(c, with_dh_in, dtype=torch.float64):
    a = case_inputs(c)
    out = run(a["px"], a["wgh"], a["woh"], a["ln"], a["h0"], a["gh"], a["dh_in"] if with_dh_in else None, dtype)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def floor_fit(e32, e64):
    """(atol, rtol) of the float32 floor of one output: the smallest pair of this form that the float32 run itself meets,
        atol = max |e32 - e64| over the elements with |e64| <= median |e64|,
        rtol = max (|e32 - e64| - atol) / |e64| over the others (0 when atol already covers them)."""
    err, mag = np.abs(e32 - e64).ravel(), np.abs(e64).ravel()
    small = mag <= np.median(mag)
    atol = float(err[small].max())
    rest = ~small & (err > atol)
    rtol = float(((err[rest] - atol) / mag[rest]).max()) if rest.any() else 0.0
    return atol, rtol


def case_floor(c):
    """{output: (atol, rtol)} of one case; the backward outputs over both runs (without and with dh_in)."""
    fit = {}
    for with_dh_in in (False, True):
        e64, e32 = expect(c, with_dh_in), expect(c, with_dh_in, torch.float32)
        for k in OUTPUTS:
            a, r = floor_fit(e32[k], e64[k])
            fit[k] = (max(a, fit.get(k, (0, 0))[0]), max(r, fit.get(k, (0, 0))[1]))
    return fit


# {(F, shape class): {output: (atol, rtol)}} = MARGIN * the worst floor over the cases of that F and class, as
# tests/test_gru_train_reference_host.py measures and prints it (and holds these constants to what it measures).  The
# element-by-element outputs carry the same pair in both classes of an F (one element's rounding error does not depend on the
# image's extent; the narrow cases only sample it with fewer elements); the sums (stats, part) grow with the number of terms.
BOUNDS = {
    (16, 'seam'): {'g': (4.8e-06, 1.8e-06), 'c': (2.8e-06, 1.5e-06), 'rh': (1e-06, 9.2e-07), 'h': (1.7e-06, 7.9e-08), 'stats': (0.00046, 4.8e-07), 'gpx': (1.6e-06, 4.6e-06), 'part': (1.1e-05, 3.1e-06), 'dh_out': (2.6e-06, 7.6e-07)},
    (16, 'narrow'): {'g': (4.8e-06, 1.8e-06), 'c': (2.8e-06, 1.5e-06), 'rh': (1e-06, 9.2e-07), 'h': (1.7e-06, 7.9e-08), 'stats': (2.4e-05, 4.6e-07), 'gpx': (1.6e-06, 4.6e-06), 'part': (2.9e-06, 1e-06), 'dh_out': (2.6e-06, 7.6e-07)},
    (8, 'seam'): {'g': (3.6e-06, 6.9e-07), 'c': (1.6e-06, 1.6e-07), 'rh': (8.5e-07, 5.1e-07), 'h': (1.3e-06, 2.3e-08), 'stats': (0.00089, 3.6e-07), 'gpx': (9.4e-07, 5.9e-06), 'part': (1.5e-05, 1.9e-06), 'dh_out': (2e-06, 1.2e-06)},
    (8, 'narrow'): {'g': (3.6e-06, 6.9e-07), 'c': (1.6e-06, 1.6e-07), 'rh': (8.5e-07, 5.1e-07), 'h': (1.3e-06, 2.3e-08), 'stats': (2.9e-05, 3.7e-07), 'gpx': (9.4e-07, 5.9e-06), 'part': (2.8e-06, 1.5e-06), 'dh_out': (2e-06, 1.2e-06)},
    (4, 'seam'): {'g': (2.8e-06, 5.7e-07), 'c': (1.7e-06, 1e-07), 'rh': (6.5e-07, 3.1e-07), 'h': (1.2e-06, 2.7e-07), 'stats': (0.002, 9.2e-08), 'gpx': (9.3e-07, 8.5e-06), 'part': (1.7e-05, 6.2e-07), 'dh_out': (3e-06, 7.1e-07)},
    (4, 'narrow'): {'g': (2.8e-06, 5.7e-07), 'c': (1.7e-06, 1e-07), 'rh': (6.5e-07, 3.1e-07), 'h': (1.2e-06, 2.7e-07), 'stats': (3.8e-06, 3e-07), 'gpx': (9.3e-07, 8.5e-06), 'part': (5.4e-06, 2.7e-06), 'dh_out': (3e-06, 7.1e-07)},
    (2, 'seam'): {'g': (2.1e-06, 2.1e-07), 'c': (1.3e-06, 3e-07), 'rh': (5.2e-07, 3.3e-07), 'h': (7.7e-07, 7.5e-07), 'stats': (0.001, 9.4e-08), 'gpx': (8.6e-07, 3.2e-06), 'part': (7.6e-06, 2.2e-06), 'dh_out': (1.9e-06, 1e-06)},
    (2, 'narrow'): {'g': (2.1e-06, 2.1e-07), 'c': (1.3e-06, 3e-07), 'rh': (5.2e-07, 3.3e-07), 'h': (7.7e-07, 7.5e-07), 'stats': (5.9e-06, 2.4e-07), 'gpx': (8.6e-07, 3.2e-06), 'part': (1.8e-06, 2.3e-06), 'dh_out': (1.9e-06, 1e-06)},
    (1, 'seam'): {'g': (1.1e-06, 3.7e-07), 'c': (1.1e-06, 2.7e-07), 'rh': (4e-07, 1.1e-06), 'h': (8.8e-07, 2.2e-07), 'stats': (6.6e-05, 4.7e-07), 'gpx': (1.1e-06, 1.4e-05), 'part': (1.3e-05, 1.6e-06), 'dh_out': (1.9e-06, 8.1e-07)},
    (1, 'narrow'): {'g': (1.1e-06, 3.7e-07), 'c': (1.1e-06, 2.7e-07), 'rh': (4e-07, 1.1e-06), 'h': (8.8e-07, 2.2e-07), 'stats': (2.9e-06, 3.9e-07), 'gpx': (1.1e-06, 1.4e-05), 'part': (8.7e-07, 5.8e-06), 'dh_out': (1.9e-06, 8.1e-07)},
}


def bound(c, name, e64):
    atol, rtol = BOUNDS[(c.F, shape_class(c))][name]
    return atol + rtol * np.abs(e64)


def conditioned(c):
    """The float64 reference is well conditioned at this case: every LayerNorm plane has a variance far above epsilon."""
    return float(expect(c, True)["var"].min())


# ---- failures by plane, tile and position ------------------------------------------------------------------------------------------
def describe_failures(c, name, got, e64, limit=8):
    """None when `got` is within bound(c, name) of e64 everywhere, else a message that names the worst elements: for the
    (planes, H, W, channels) buffers by plane, tile index, position in the tile and channel (with its output-channel group)."""
    got = np.asarray(got, np.float64).reshape(e64.shape)
    lim = bound(c, name, e64)
    err = np.abs(got - e64)
    bad = ~(err <= lim)                                       # (NaN counts as bad)
    if not bad.any():
        return None
    atol, rtol = BOUNDS[(c.F, shape_class(c))][name]
    th, tw, ns = tile_of(c.F)
    score = np.where(bad, np.where(np.isfinite(err), err / lim, np.inf), -1.0)
    lines = ["%s %s: %d of %d elements outside atol %.3g + rtol %.3g |expected|; tile %d x %d, %d channel group(s); worst:"
             % (case_id(c), name, bad.sum(), bad.size, atol, rtol, th, tw, ns)]
    for flat in np.argsort(-score, axis=None)[:limit]:
        i = np.unravel_index(flat, e64.shape)
        if not bad[i]:
            break
        if e64.ndim == 4 or name == "dh_out":
            d, (y, x, ch) = (i[0] if e64.ndim == 4 else 0), i[-3:]
            where = "plane %d, tile (%d, %d), row %d col %d of the tile, channel %d" % (d, y // th, x // tw, y % th, x % tw, ch)
            if name in ("g", "c", "dh_out"):                  # what a convolution's epilogue writes, one channel group per wave set
                where += " (group %d)" % (ch // max(e64.shape[-1] // ns, 1))
        else:
            where = "index %s" % (tuple(int(v) for v in i),)
        lines.append("  %s: got %r expected %r (%.1f bounds)" % (where, float(got[i]), float(e64[i]), float(score[i])))
    return "\n".join(lines)
