"""Every pixel of the recurrent winner-take-all sweep against float64 plane scores, on every kernel route of mvs_gru_wta_f32 /
mvs_gru_wta_batch_f32 (csrc/gru.hip, gru_fused.hip, gru_mfma.hip).  The rule and where its bound comes from: tests/sweep_reference.py;
that the reference itself stays inside it and planted faults do not: tests/test_sweep_reference_host.py.  No pixel is excluded.

Shapes of the 'normal' width (32 feature channels, filters 16 / 4 / 2), and what each reaches:
  (27,41) (9,47) (31,17) x 16   partial 8 x 16 and 16 x 16 tiles; a single tile row; a narrow tile column
  (5,11) x 17                   smaller than one tile both ways; a second cost batch of ONE plane (XB = 16)
  (21,37) x 19                  the batch test's shape
  (19,35) x 2, 3, 4             shorter than the fused pipeline (t runs to D + 2, the STEADY template first runs at D = 4)
  (19,35) x 70                  the fused sweep's 64-row LayerNorm-sum ring wraps; the 16-plane state ring wraps four times
  (19,35) x 83                  the wavefront's (d / XB) % (SB + 1) LayerNorm ring wraps
  (17,33) x 130                 the fused ring wraps twice
Every case prints its worst winner regret and prob distance as multiples of E (pytest -s)."""
import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L

from tests import sweep_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    from mvsnet_amd.model import DepthPlan
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    keep = DepthPlan(3, 2, 8, 16, 32, weights_of("normal"), "GRU", DEV)      # holds the stream set: one calibration for the file
    yield
    keep.close()


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


_WEIGHTS = {}


def weights_of(width):
    from mvsnet_amd.model import MVSNetWeights
    if width not in _WEIGHTS:
        _WEIGHTS[width] = MVSNetWeights.from_numpy("normal", gru=R.width_params(width)[1], device=DEV)
    return _WEIGHTS[width]


def run_device(width, H, W, D, views=(0,), form=0, impl="auto", **hooks):
    """One sweep of `views` (view indices of sweep_reference.case) on the route (formulation, convolution implementation, test
    hooks) -> depth, prob as (len(views), H, W) torch tensors.  One view goes through mvs_gru_wta_f32, several through the batch."""
    from mvsnet_amd.model import DepthPlan, wta_depth_values
    cases = [R.case(width, H, W, D, v) for v in views]
    plan = DepthPlan(3, D, H, W, cases[0]["C"], weights_of(width), "GRU", DEV, views=len(views))
    dvs = []
    for i, c in enumerate(cases):
        if D == 1:                                   # the Python wrappers divide by D - 1: one plane at depth_start
            interval, dv = 0.0, np.asarray([c["start"]], np.float32)
        else:
            interval = float((np.float32(c["end"]) - np.float32(c["start"])) / (np.float32(D) - np.float32(1)))
            dv = wta_depth_values(D, c["start"], c["end"], False)
        plan.set_cameras(t(c["cams"]), c["start"], interval, c["start"] if D == 1 else c["end"], False, view=i)
        dvs.append(dv)
    feats = [t(c["features"]) for c in cases]
    lib = L.load()
    try:
        L.set_conv_impl(impl)
        L.check(lib.mvs_gru_set_formulation(form), "mvs_gru_set_formulation")
        with L.test_hooks(**hooks):
            if len(views) == 1:
                d, p = plan.run_gru(feats[0], dvs[0])
                d, p = d[None], p[None]
            else:
                d, p = plan.run_gru_batch(feats, dvs)
            torch.cuda.synchronize()
            d, p = d.clone(), p.clone()
    finally:
        L.check(lib.mvs_gru_set_formulation(0), "mvs_gru_set_formulation")
        L.set_conv_impl("auto")
    return d, p


def hold(width, H, W, D, views=(0,), tag="", **route):
    dt, pt = run_device(width, H, W, D, views, **route)
    d, p = dt.cpu().numpy(), pt.cpu().numpy()
    for i, v in enumerate(views):
        _c, ref = R.case_scores(width, H, W, D, v)
        R.check_every_pixel(d[i], p[i], ref, "%s %s %dx%d D=%d view %d of %d" % (tag, width, H, W, D, v, len(views)))
    return dt, pt


SHAPES = R.NORMAL_SHAPES
sid = lambda s: "%dx%d-D%d" % s
LONG = [s for s in SHAPES if s[2] > 8]               # the wavefront needs more than 2 * PG = 8 planes


# ---- the fused two-launch sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_fused_sweep_on_a_prepared_stream(shape):
    """Formulation 0: from 17 planes on the cost slices come from the producer stream, one batch ahead."""
    hold("normal", *shape, tag="fused")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_fused_sweep_on_one_stream(shape):
    hold("normal", *shape, tag="fused, one stream", gru_one_stream=1)


def test_fused_sweep_producer_workgroup_sizes_give_the_same_bits():
    """include/mvsnet_hip.h: the fused sweep gives the same bits every time -- the producer's workgroup size is a tuning hook."""
    d0, p0 = run_device("normal", 19, 35, 70)
    for threads in (64, 256):
        d, p = hold("normal", 19, 35, 70, tag="fused, producer of %d threads" % threads, gru_producer_threads=threads)
        assert torch.equal(d, d0) and torch.equal(p, p0), threads


# ---- the wavefront formulations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("shape", LONG + [(19, 35, 4)], ids=sid)
def test_wavefront_on_a_prepared_stream(shape, form):
    """Formulation 1: cell 1's x-part hoisted; 2: full 48-channel kernels.  Four streams from 9 planes on; 4 planes stay on one."""
    hold("normal", *shape, tag="wavefront %d" % form, form=form)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("shape", [(27, 41, 16), (19, 35, 83)], ids=sid)
def test_wavefront_on_one_stream(shape, form):
    """The unfolded blend and a separate prob_wta launch per plane."""
    hold("normal", *shape, tag="wavefront %d, one stream" % form, form=form, gru_one_stream=1)


def test_scalar_implementation():
    """mvs_set_conv_impl(SCALAR): generic cell 1 plus the small-cell kernels, one stream."""
    hold("normal", 27, 41, 16, tag="scalar", impl="scalar")


# ---- several views per sweep ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [dict(form=0), dict(form=1), dict(form=2), dict(form=0, impl="scalar")],
                         ids=["fused", "wavefront1", "wavefront2", "scalar"])
def test_three_views_each_against_its_own_scores(route):
    """Different features and depth ranges per view.  The wavefront routes take the vector form of conv2d_small_kernel here."""
    hold("normal", 27, 41, 16, views=(0, 1, 2), tag="3 views %s" % (route,), **route)


# ---- other widths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [(0,), (0, 1)], ids=["1view", "2views"])
@pytest.mark.parametrize("shape", R.WIDTH_SHAPES, ids=sid)
@pytest.mark.parametrize("width", ["lite", "fat"])
def test_other_widths(width, shape, views):
    """'lite' (16 channels) and 'fat' (64 channels), filters 8 / 2 / 1: generic cell 1, small cells 2 and 3, prob_wta_kernel<1>."""
    hold(width, *shape, views=views, tag="width")


@pytest.mark.parametrize("views", [(0,), (0, 1)], ids=["1view", "2views"])
def test_fat_variant_filters_32_8_4(views):
    """64 channels, filters 32 / 8 / 4 (include/mvsnet_hip.h's 'fat' variant): every cell generic, a 64-channel gate convolution,
    prob_wta_kernel<4>."""
    hold("wide", 27, 41, 16, views=views, tag="32/8/4")


def test_hand_made_filters_12_6_3():
    """16 channels, filters 12 / 6 / 3: no cell has a specialised kernel, and the tail is prob_conv through the generic convolution
    followed by mvs_wta_update_f32 (the default: branch of prob_wta)."""
    hold("odd", 27, 41, 16, tag="12/6/3")


# ---- one plane --------------------------------------------------------------------------------------------------------------------
def test_one_plane():
    """D = 1 through mvs_gru_wta_f32 with one depth value: every pixel holds it, prob = e / (e + 1e-7) of the single score."""
    for route in (dict(), dict(form=1), dict(impl="scalar")):
        d, p = run_device("normal", 19, 35, 1, **route)
        d, p = d.cpu().numpy()[0], p.cpu().numpy()[0]
        _c, ref = R.case_scores("normal", 19, 35, 1)
        assert np.all(d == np.float32(R.DEPTH_START)), route
        e = np.exp(ref.reg64[0])
        assert np.array_equal(ref.p64, e / (e + 1e-7))
        R.check_every_pixel(d, p, ref, "one plane %s" % (route,))


# ---- the two public entry points of the tail --------------------------------------------------------------------------------------
def test_wta_update_and_finish_known_answers():
    """mvs_wta_update_f32 plane by plane over a 1 x 70 map, then mvs_wta_finish_f32: the first maximum is kept (exact ties between
    planes, a later strictly larger plane), exp_sum is the float32 running sum in plane order bit for bit, scores of -1000 add
    nothing, prob = max / (sum + 1e-7f)."""
    lib = L.load()
    P, W = 6, 70
    rs = np.random.RandomState(4)
    reg = rs.uniform(-2.0, 0.5, size=(P, W)).astype(np.float32)
    reg[3, :20] = reg[1, :20] = 1.0 + 0.01 * np.arange(20, dtype=np.float32)      # exact tie of the two largest: plane 1 stays
    reg[4, 10:30] = 2.5                                                          # a later, strictly larger plane takes over
    reg[5, 25:40] = 2.5                                                          # ... and its own tie leaves plane 4 where it won
    reg[:, 40:50] = -1000.0                                                      # exp underflows to zero on every plane
    reg[:, 50:60] = -1000.0; reg[2, 50:60] = -0.25                               # one live plane among dead ones
    depths = (425.0 + 30.0 * np.arange(P)).astype(np.float32)
    sp = L.stream_ptr()
    z = lambda: torch.zeros(W, device=DEV)
    dreg = t(reg)
    # the device's own exp of every score (one update from zero: exp_sum = 0 + p), within 2 ulp of the float64 value
    pexp = np.empty_like(reg)
    for d in range(P):
        mp, di, es = z(), z(), z()
        L.check(lib.mvs_wta_update_f32(L.ptr(dreg[d]), float(depths[d]), 1, W, L.ptr(mp), L.ptr(di), L.ptr(es), sp))
        pexp[d] = es.cpu().numpy()
        assert torch.equal(mp, es)
    exact = np.exp(reg.astype(np.float64))
    assert np.all(np.abs(pexp - exact) <= 2 * np.spacing(exact.astype(np.float32)))
    assert np.all(pexp[:, 40:50] == 0)
    # the sweep
    mp, di, es = z(), z(), z()
    for d in range(P):
        L.check(lib.mvs_wta_update_f32(L.ptr(dreg[d]), float(depths[d]), 1, W, L.ptr(mp), L.ptr(di), L.ptr(es), sp))
    prob = torch.empty(W, device=DEV)
    L.check(lib.mvs_wta_finish_f32(L.ptr(mp), L.ptr(es), 1, W, L.ptr(prob), sp))
    torch.cuda.synchronize()
    e_mp = np.zeros(W, np.float32); e_di = np.zeros(W, np.float32); e_es = np.zeros(W, np.float32)
    for d in range(P):
        upd = e_mp < pexp[d]
        e_mp = np.where(upd, pexp[d], e_mp); e_di = np.where(upd, depths[d], e_di); e_es = e_es + pexp[d]
    assert np.array_equal(di.cpu().numpy(), e_di)
    assert np.all(e_di[:10] == depths[1]) and np.all(e_di[10:30] == depths[4]) and np.all(e_di[30:40] == depths[5])
    assert np.all(e_di[40:50] == 0) and np.all(e_di[50:60] == depths[2])
    assert np.array_equal(mp.cpu().numpy(), e_mp)
    assert np.array_equal(es.cpu().numpy(), e_es)
    assert np.array_equal(prob.cpu().numpy(), e_mp / (e_es + np.float32(1e-7)))
    assert np.all(prob.cpu().numpy()[40:50] == 0)
