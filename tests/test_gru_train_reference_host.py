"""Preconditions of tests/test_gpu_gru_train_seams.py, asserted on the CPU from tests/gru_train_reference.py alone (no GPU):

  * the reference is the oracle's cell: h[1..D] equals a chain of oracle.torch_grad.conv_gru_cell calls to 1e-12, with px formed
    by the host's batched convolution as mvsnet_amd/gru_train.py forms it;
  * the bounds: per F and shape class the float32 floor of every output -- the reference's float32 mode against its float64 mode,
    fitted as atol + rtol |expected| (gru_train_reference.floor_fit), worst over the cases -- times MARGIN is what BOUNDS holds
    (the element-by-element outputs share one floor per F, the worst of both classes; the sums have one per class: measured_floor).
    The floor is printed (pytest -s); BOUNDS was filled from that output and is held to it within a factor of 1.5 either way (a
    float32 convolution may add in another order on another host);
  * the cases: three tiles on both axes at the seam shapes, a partial last block of the elementwise launches at the narrow ones,
    and every LayerNorm plane of the float64 reference with a variance far above epsilon (nothing is masked in the GPU test, so
    nothing may be ill-conditioned);
  * every seeded defect (gru_train_reference's docstring) is at least 100 bounds large where it lands, at every seam case.

A margin is the largest |seeded - true| / bound over the elements the defect touches (one of them outside is a failing test), the
smallest such figure over the buffers it lands in: halo -- g of plane 0 in column 0 of tile (0, 1); ln_rows -- the two sums, rh,
c and the next state of plane 0; group -- the last channel group of tile (1, 1) in every plane of g, c, rh, h, gpx and dh_out,
against zero; parity -- gpx of planes D - 2 and 0, dh_out; no_dh_in -- gpx of planes D - 1 and 0, dh_out.  Each must be >= 100 at
every seam case; the smallest per F is printed (pytest -s) and recorded here as measured on the reference:

    F     halo   ln_rows    group   parity  no_dh_in
    16  171168      1075   188941   487030    386871
    8   319678      1784   157077   625438    422551
    4   384200       683   112569   432993    426984
    2   509278       406   258935   521996    471076
    1   513792       520    68359   333257    364102

No shape and no seed had to be moved (gru_train_reference.SEEDS is empty): the smallest LayerNorm variance of any case is 0.36.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_grad as TG

from tests import gru_train_reference as R

MARGIN = 100.0
BAND = 1.5


def test_the_reference_is_the_oracles_cell_chain():
    D, H, W, Cin, Fn = 3, 9, 19, 3, 4
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    c = Cin + Fn
    p = {"gates_w": rnd(3, 3, c, 2 * Fn) * (1.5 / np.sqrt(9 * c)), "out_w": rnd(3, 3, c, Fn) * (1.5 / np.sqrt(9 * c)),
         "gates_b": 0.1 * rnd(2 * Fn), "out_b": 0.1 * rnd(Fn)}
    for nm in ("reset", "update", "out"):
        p[nm + "_gamma"], p[nm + "_beta"] = 1 + 0.3 * rnd(Fn), 0.2 * rnd(Fn)
    x, h0 = rnd(D, H, W, Cin), torch.tanh(rnd(H, W, Fn))
    # the x parts of both convolutions, as gru_train._cell_forward forms them: one batched convolution, [reset | update | candidate]
    wx = torch.cat([p["gates_w"][:, :, :Cin, :], p["out_w"][:, :, :Cin, :]], 3).permute(3, 2, 0, 1).contiguous()
    px = F.conv2d(x.permute(0, 3, 1, 2), wx, torch.cat([p["gates_b"], p["out_b"]]), padding=1).permute(0, 2, 3, 1)
    ln = torch.stack([p[k] for k in ("reset_gamma", "reset_beta", "update_gamma", "update_beta", "out_gamma", "out_beta")])
    out = R.run(px.numpy(), p["gates_w"][:, :, Cin:, :].numpy(), p["out_w"][:, :, Cin:, :].numpy(), ln.numpy(), h0.numpy(),
                np.ones((D, H, W, Fn)))
    h = h0.permute(2, 0, 1)[None]
    for d in range(D):
        h = TG.conv_gru_cell(x[d].permute(2, 0, 1)[None], h, p)
        np.testing.assert_allclose(out["h"][d + 1], h[0].permute(1, 2, 0).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(out["h"][0], h0.numpy())
    np.testing.assert_allclose(out["rh"][0] / h0.numpy(), 1 / (1 + np.exp(-_ln_np(out["g"][0][..., :Fn], ln[0].numpy(), ln[1].numpy()))),
                               rtol=1e-12)
    np.testing.assert_allclose(out["stats"][1], [s for v in (out["g"][1][..., :Fn], out["g"][1][..., Fn:], out["c"][1])
                                                 for s in (v.sum(), (v ** 2).sum())], rtol=1e-12)


def _ln_np(x, gamma, beta):
    return (x - x.mean()) / np.sqrt(x.var() + R.LN_EPSILON) * gamma + beta


def test_the_gradients_are_those_of_the_shared_parameters():
    """Summed over the planes, `part` is the gradient of the six shared LayerNorm vectors, and dh_in enters as <h[D], dh_in>."""
    c = R.SEAM_CASES[-1]
    a = R.case_inputs(c)
    t = lambda k: torch.tensor(a[k], dtype=torch.float64)
    ln, h0 = t("ln").requires_grad_(True), t("h0").requires_grad_(True)
    h, total = h0, 0.0
    for d in range(c.D):
        g = t("px")[d][..., :2 * c.F] + R._conv(h, t("wgh"))
        r = torch.sigmoid(R._layer_norm(g[..., :c.F], ln[0], ln[1]))
        u = torch.sigmoid(R._layer_norm(g[..., c.F:], ln[2], ln[3]))
        y = torch.tanh(R._layer_norm(t("px")[d][..., 2 * c.F:] + R._conv(r * h, t("woh")), ln[4], ln[5]))
        h = u * h + (1.0 - u) * y
        total = total + (h * t("gh")[d]).sum()
    (total + (h * t("dh_in")).sum()).backward()
    e = R.expect(c, True)
    shared = e["part"].sum(0)                                           # (3, [d beta, d gamma], F)
    np.testing.assert_allclose(shared[:, 1], ln.grad[0::2].numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(shared[:, 0], ln.grad[1::2].numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(e["dh_out"], h0.grad.numpy(), rtol=1e-10, atol=1e-13)
    assert np.abs(e["dh_out"] - R.expect(c, False)["dh_out"]).max() > 1e-3


def test_the_cases_are_the_shapes_the_kernels_branch_on():
    assert len(set(map(R.case_id, R.CASES))) == len(R.CASES)
    assert {R.seam_shape(Fn) for Fn in R.FILTERS} == {(9, 33), (17, 33), (33, 33)}
    for c in R.SEAM_CASES:
        th, tw, ns = R.tile_of(c.F)
        assert (c.H, c.W) == (2 * th + 1, 2 * tw + 1) and th * ns == 16 and c.D in (3, 4)
    for Fn in R.FILTERS:
        assert {c.D for c in R.CASES if c.F == Fn} == {1, 2, 3, 4}
    for c in R.NARROW_CASES:
        assert (c.H * c.W * c.F) % 256 != 0


def test_every_case_is_well_conditioned():
    """Nothing is masked in the GPU test: the float64 reference itself must not sit on a LayerNorm with a vanishing variance."""
    low = {R.case_id(c): R.conditioned(c) for c in R.CASES}
    print("smallest LayerNorm variance per case:", {k: round(v, 3) for k, v in low.items()})
    assert all(v > 0.05 for v in low.values()), {k: v for k, v in low.items() if not v > 0.05}


def measured_floor():
    """{(F, class): {output: (atol, rtol)}}: the worst float32 floor over the cases of that F and shape class."""
    worst = {}
    for c in R.CASES:
        w = worst.setdefault((c.F, R.shape_class(c)), {})
        for k, (a, r) in R.case_floor(c).items():
            w[k] = (max(a, w.get(k, (0, 0))[0]), max(r, w.get(k, (0, 0))[1]))
    # The rounding error of ONE element does not depend on the extent of the image, and a narrow case samples it with a few
    # dozen elements where a seam case has thousands: the element-by-element outputs take the worst of both classes.  The
    # sums (stats, part) keep a floor per class: theirs grows with the number of terms.
    for Fn in R.FILTERS:
        seam, narrow = worst[(Fn, "seam")], worst[(Fn, "narrow")]
        for k in R.OUTPUTS:
            if k not in ("stats", "part"):
                seam[k] = narrow[k] = (max(seam[k][0], narrow[k][0]), max(seam[k][1], narrow[k][1]))
    return worst


def test_the_float32_floor_fixes_the_bounds():
    floor = measured_floor()
    print("float32 floor (atol, rtol) per F, shape class and output; BOUNDS = %g x these:" % R.MARGIN)
    for key in sorted(floor, reverse=True):
        print("    %r: {%s}," % (key, ", ".join("'%s': (%.2g, %.2g)" % (k, R.MARGIN * floor[key][k][0], R.MARGIN * floor[key][k][1])
                                               for k in R.OUTPUTS)))
    assert set(R.BOUNDS) == set(floor)
    for key, outs in floor.items():
        for k, (a, r) in outs.items():
            ba, br = R.BOUNDS[key][k]
            assert R.MARGIN * a / BAND <= ba <= R.MARGIN * a * BAND, (key, k, "atol", ba, R.MARGIN * a)
            # (a relative part below one float32 ulp decides nothing next to the absolute one: held from above only)
            assert br <= R.MARGIN * r * BAND and (br >= R.MARGIN * r / BAND or R.MARGIN * r < 6e-8), (key, k, "rtol", br, R.MARGIN * r)


# ---- the seeded defects ------------------------------------------------------------------------------------------------------------
def _seeded(c, defect):
    a = R.case_inputs(c)
    return R.run(a["px"], a["wgh"], a["woh"], a["ln"], a["h0"], a["gh"], a["dh_in"], defect=defect)


def defect_margins(c):
    """{defect: smallest, over the buffers the defect lands in, of the largest |defect - true| / bound over the elements it touches}."""
    e = R.expect(c, True)
    th, tw, ns = R.tile_of(c.F)
    ratio = lambda name, got, at: float((np.abs(got[name][at] - e[name][at]) / R.bound(c, name, e[name])[at]).max())
    out = {}
    d = _seeded(c, "halo")
    out["halo"] = ratio("g", d, (0, slice(0, th), tw))                   # plane 0, tile (0, 1), its column 0
    d = _seeded(c, "ln_rows")
    out["ln_rows"] = min(ratio("stats", d, (0, slice(0, 2))), ratio("rh", d, 0), ratio("c", d, 0), ratio("h", d, 1))
    zero = {k: np.zeros_like(v) for k, v in e.items()}
    per = []
    for name in ("g", "c", "rh", "h", "gpx", "dh_out"):
        ch = e[name].shape[-1]
        grp = slice(ch - max(ch // ns, 1), ch)                           # the last output-channel group
        tile = (slice(th, 2 * th), slice(tw, 2 * tw), grp)
        planes = [()] if name == "dh_out" else [(p,) for p in range(1 if name == "h" else 0, e[name].shape[0])]
        per += [ratio(name, zero, p + tile) for p in planes]
    out["group"] = min(per)
    d = _seeded(c, "parity")
    out["parity"] = min(ratio("gpx", d, c.D - 2), ratio("gpx", d, 0), ratio("dh_out", d, ()))
    d = _seeded(c, "no_dh_in")
    out["no_dh_in"] = min(ratio("gpx", d, c.D - 1), ratio("gpx", d, 0), ratio("dh_out", d, ()))
    return out


@pytest.mark.parametrize("Fn", R.FILTERS)
def test_a_seeded_defect_is_a_hundred_times_the_bound(Fn):
    low = {}
    for c in (c for c in R.SEAM_CASES if c.F == Fn):
        for k, v in defect_margins(c).items():
            low[k] = min(v, low.get(k, np.inf))
            assert v >= MARGIN, (R.case_id(c), k, v)
    print("margins F = %2d: %s" % (Fn, "  ".join("%s %.0f" % (k, low[k]) for k in R.DEFECTS)))
    assert set(low) == set(R.DEFECTS)


def test_a_failure_names_plane_tile_position_and_channel():
    c = R.SEAM_CASES[0]                                                  # F = 16: tiles of 4 x 16, 4 groups
    e = R.expect(c, False)["c"]
    got = e.astype(np.float32).astype(np.float64)
    assert R.describe_failures(c, "c", got, e) is None
    got[2, 8, 32, 13] = np.nan                                           # the one-pixel corner tile
    got[1, 3, 16, 5] += 1e-3
    msg = R.describe_failures(c, "c", got, e)
    assert "2 of %d elements" % e.size in msg
    assert "plane 2, tile (2, 2), row 0 col 0 of the tile, channel 13 (group 3)" in msg
    assert "plane 1, tile (0, 1), row 3 col 0 of the tile, channel 5 (group 1)" in msg
    s = R.expect(c, False)["stats"]
    assert "index (1, 4)" in R.describe_failures(c, "stats", s + 1e3 * (np.arange(6) == 4) * (np.arange(c.D) == 1)[:, None], s)
