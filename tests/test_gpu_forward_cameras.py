"""The forward geometry path -- mvs_homography_transforms_f32, mvs_warp_f32 (zero fill), mvs_cost_volume_f32 on both of its
routes, and what consumes them (features to depth, the recurrent sweep) -- under the camera families of tests/camera_families.py,
hand-made transforms (a horizon, samples beyond int32, proj near and exactly 0) and far worlds, every element against the float64
reference.  The rule, its unit and the case table: tests/forward_warp_reference.py; that the float32 CPU oracle stays within a
third of the bound and planted faults do not: tests/test_forward_warp_reference_host.py.  No voxel is excluded.

Every test prints its worst ratio (pytest -s)."""
import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S
from mvsnet_amd import _lib as L

from tests import forward_warp_reference as F
from tests import sweep_reference as SR
from tests.device_arena import PATTERNS, Arena

pytestmark = pytest.mark.gpu

DEV = "cuda"
ids = lambda c: c.tag


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def t(a):
    return torch.as_tensor(np.array(a, dtype=np.float32, order="C")).to(DEV)          # (a copy: the cached inputs are read-only)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- homographies --------------------------------------------------------------------------------------------------------------
WORLDS = [(nm, None) for nm in F.FAMILIES] + [("random0", w) for w in F.FAR_WORLDS] + [("roll60", F.FAR_WORLDS[1])]


@pytest.mark.parametrize("inverse", [False, True], ids=["linear", "inverse"])
@pytest.mark.parametrize("name,world", WORLDS, ids=["%s%s" % (nm, "" if w is None else "-far%g" % w[0]) for nm, w in WORLDS])
def test_homographies_match_float64_entry_by_entry(name, world, inverse):
    """Both outputs at both depth intervals.  Per entry: 3 x the float32 oracle's largest distance from float64 among the entries
    of its kind for that view over the planes (linear terms, translations, projective terms; each row of H), floor 4 eps32 |entry|."""
    from mvsnet_amd.homography_warping import homography_transforms
    worst = 0.0
    for interval in F.INTERVALS:
        cams = F.family_cams(name, interval=interval)
        if world is not None:
            cams = F.far_world(cams, *world)
        start = float(cams[0, 1, 3, 0])
        end = start + (F.D - 1) * interval
        T64, H64, bT, bH, _e = F.homography_reference(cams, F.D, start, interval, end, inverse)
        T, Hm = homography_transforms(t(cams), F.D, start, interval, end, inverse, True)
        T, Hm = n(T).astype(np.float64), n(Hm).astype(np.float64)
        assert T.shape == T64.shape and Hm.shape == H64.shape
        assert np.isfinite(T).all() and np.isfinite(Hm).all()
        rT, rH = np.abs(T - T64) / bT, np.abs(Hm - H64) / bH
        worst = max(worst, float(rT.max()), float(rH.max()))
        print("homographies %s %s interval %g %s: worst share of the bound T %.3f H %.3f" % (
            name, world, interval, "inverse" if inverse else "linear", rT.max(), rH.max()))
        assert rT.max() <= 1.0, (interval, np.unravel_index(rT.argmax(), rT.shape), float(rT.max()))
        assert rH.max() <= 1.0, (interval, np.unravel_index(rH.argmax(), rH.shape), float(rH.max()))


# ---- warp ----------------------------------------------------------------------------------------------------------------------
WARP_CASES = [F._camera_case(nm, iv) for nm in F.FAMILIES for iv in F.INTERVALS] + F.hand_cases(16)


@pytest.mark.parametrize("case", WARP_CASES, ids=ids)
def test_warp_holds_every_pixel(case):
    """mvs_warp_f32 with zero fill: one plane per source view of a camera case, every plane of the hand-made transforms."""
    from mvsnet_amd.homography_warping import transform_image
    p = F.problem(case)
    for v in range(p.T.shape[0]):
        planes = range(p.T.shape[1]) if case.kind == "hand" else [(3 * v + 1) % p.T.shape[1]]
        img = t(p.features[v + 1])
        for d in planes:
            ref, unit = F.warp_reference(p.features[v + 1], p.T[v, d])
            F.check_every_voxel(n(transform_image(img, t(p.T[v, d]))), ref, unit, "warp %s view %d plane %d" % (case.tag, v + 1, d))


# ---- cost volume ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", F.all_cases(), ids=ids)
def test_cost_volume_holds_every_voxel(case):
    """The voted launch of both variants and the negated eager one against the float64 reference; each forced wave-tile shape
    gives the voted launch's bits; planes d_begin .. d_begin + 1 launched alone give the whole launch's bits."""
    from mvsnet_amd.model import cost_volume
    p = F.problem(case)
    ref, unit = F.reference(case)
    ft, Tt = t(p.features), t(p.T)
    b = 3 if case.planes >= 5 else 1
    L.set_test_hook("cv_tile_rows_log2", -1)
    route = "sweep, vote %d" % F.vote(p.T, case.height, case.width, case.channels) if F.takes_sweep(case) else "per plane"
    for variant in ("mem", "eager"):
        got = n(cost_volume(ft[0], ft[1:], Tt, variant=variant))
        F.check_every_voxel(got, ref, unit, "cost volume %s %s (%s)" % (case.tag, variant, route))
        if F.takes_sweep(case):
            for rows_log2 in range(4):
                with L.test_hooks(cv_tile_rows_log2=rows_log2):
                    forced = n(cost_volume(ft[0], ft[1:], Tt, variant=variant))
                assert same_bits(forced, got), (variant, rows_log2)
        sub = n(cost_volume(ft[0], ft[1:], Tt, d_begin=b, d_count=2, variant=variant))
        assert same_bits(sub, got[b:b + 2]), variant
    neg = n(cost_volume(ft[0], ft[1:], Tt, variant="eager", negate=True))
    F.check_every_voxel(neg, -ref, unit, "cost volume %s -eager (%s)" % (case.tag, route))


SHARED = [c for c in F.all_cases() if c.channels == 16]                 # the voters at 16 channels and the hand-made transforms


@pytest.mark.parametrize("case", SHARED, ids=ids)
def test_sweep_and_per_plane_kernels_agree(case):
    """Channels do not mix in the cost volume: the first 12 channels of a 16-channel case go through the per-plane kernel (3 lanes
    per pixel), all 16 through the sweep, and the 12 they share agree to 2 BOUND units, non-finite at the same voxels."""
    from mvsnet_amd.model import cost_volume
    p = F.problem(case)
    ref, unit = F.reference(case)
    ft, Tt = t(p.features), t(p.T)
    f12 = ft[..., :12].contiguous()
    for variant in ("mem", "eager"):
        sweep = n(cost_volume(ft[0], ft[1:], Tt, variant=variant))[..., :12]
        plane = n(cost_volume(f12[0], f12[1:], Tt, variant=variant))
        F.check_every_voxel(sweep, ref[..., :12], unit[..., :12], "sweep %s %s" % (case.tag, variant))
        F.check_every_voxel(plane, ref[..., :12], unit[..., :12], "per plane %s %s" % (case.tag, variant))
        assert np.array_equal(np.isfinite(sweep), np.isfinite(plane))
        fin = np.isfinite(sweep)
        with np.errstate(invalid="ignore", divide="ignore"):
            between = np.where(sweep[fin] == plane[fin], 0.0, np.abs(sweep[fin].astype(np.float64) - plane[fin]) / unit[..., :12][fin])
        print("between the routes %s %s: %.3f units" % (case.tag, variant, between.max()))
        assert between.max() <= 2 * F.BOUND


# ---- hand-made transforms in the arena -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
@pytest.mark.parametrize("case", F.hand_cases(16) + F.hand_cases(12), ids=ids)
def test_hand_made_transforms_in_the_arena(case, pattern):
    """Both routes (16 channels: the sweep; 12: the per-plane kernel) with every operand inside the poisoned, guarded arena: a
    sample point tens of widths out, beyond int32 or not finite reads no tap and stores nowhere but its own voxel.  At proj == 0
    both routes agree: a +-inf sample point contributes 0, a 0 / 0 one gives NaN (include/mvsnet_hip.h)."""
    p = F.problem(case)
    ref, unit = F.reference(case)
    a = Arena(2 << 20, pattern, DEV)
    dt = torch.float32
    rt = a.take(p.features[0].shape, dt, data=p.features[0], readonly=True, name="ref")
    st = a.take(p.features[1:].shape, dt, data=p.features[1:], readonly=True, name="src")
    Tt = a.take(p.T.shape, dt, data=p.T, readonly=True, name="transforms")
    for variant in (0, 1):
        y = a.take(ref.shape, dt, name="cost%d" % variant)
        L.check(L.load().mvs_cost_volume_f32(L.ptr(rt), L.ptr(st), L.ptr(Tt), case.views, case.planes, 0, case.planes, case.height,
                                             case.width, case.channels, variant, 0, 0, L.ptr(y), L.stream_ptr()), "mvs_cost_volume_f32")
        got = n(y)
        a.check()
        F.check_every_voxel(got, ref, unit, "arena %s variant %d pattern %#x" % (case.tag, variant, pattern))
    if case.name == "exact_zero":                                  # +-inf on planes 0, 1: the view contributes 0; 0 / 0 on planes 2, 3: NaN
        assert np.isfinite(got[:2]).all() and np.isnan(got[2:, :, 8]).all() and np.isfinite(np.delete(got, 8, axis=2)).all()


# ---- features to depth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["roll90", "tilt20", "random3"])
def test_features_to_depth_under_camera_families(name):
    """tests/test_gpu_view_counts.test_features_to_depth_at_other_view_counts at 3 views under other cameras, its bars unchanged."""
    from mvsnet_amd.model import DepthPlan, MVSNetWeights, inference_mem
    Nv, Dd, Hh, Ww, Cc, interval = 3, 8, 16, 16, 32, 60.0
    cams = F.family_cams(name, Nv, Hh, Ww, Dd, interval=interval)
    feats = S.make_features(Nv, Hh, Ww, Cc)
    start = float(cams[0, 1, 3, 0])
    rp = S.make_regnet_params("normal", seed=1, random_affine=True)
    weights = MVSNetWeights.from_numpy("normal", regnet=rp, device=DEV)
    ed, ep = O.inference_mem_from_features(feats, cams, Dd, start, interval, rp, False, np.float64)

    def hold(depth, prob, tag):
        abs_rel = float(np.mean(np.abs(depth - ed) / ed))
        share = float((~(np.abs(prob - ep) <= 1e-3)).mean())
        print("features to depth %s %s: abs-rel %.3g, prob share off by more than 1e-3: %.3g" % (name, tag, abs_rel, share))
        assert abs_rel < 1e-4, (tag, abs_rel)
        assert share < 0.02, (tag, share)

    depth, prob = inference_mem(None, t(cams)[None], Dd, start, interval, weights=weights, features=t(feats))
    assert depth.shape == (1, Hh, Ww, 1)
    hold(n(depth)[0, :, :, 0], n(prob)[0, :, :, 0], "one call")
    plan = DepthPlan(Nv, Dd, Hh, Ww, Cc, weights, "3DCNN", DEV)
    plan.set_cameras(t(cams), start, interval, start + (Dd - 1) * interval, False)
    d2, p2 = plan.run_3dcnn(t(feats), start, interval)
    hold(n(d2), n(p2), "set_cameras + run_3dcnn")


# ---- recurrent sweep -----------------------------------------------------------------------------------------------------------
_WEIGHTS = []


def gru_weights():
    from mvsnet_amd.model import MVSNetWeights
    if not _WEIGHTS:
        _WEIGHTS.append(MVSNetWeights.from_numpy("normal", gru=SR.width_params("normal")[1], device=DEV))
    return _WEIGHTS[0]


@pytest.fixture(scope="module")
def stream_set():
    """Holds the recurrent sweep's stream set for the sweep tests of this file: one calibration."""
    from mvsnet_amd.model import DepthPlan
    keep = DepthPlan(3, 2, 8, 16, 32, gru_weights(), "GRU", DEV)
    yield
    keep.close()


@pytest.mark.parametrize("impl", ["auto", "scalar"], ids=["fused", "scalar"])
@pytest.mark.parametrize("name", SR.CAMERA_FAMILIES)
def test_recurrent_sweep_under_camera_families(stream_set, name, impl):
    """27 x 41 pixels, 16 planes through sweep_reference.check_every_pixel as it is, on the fused route and on the scalar
    implementation (tests/test_sweep_reference_host.py holds the float32 reference of both cases to the same rule)."""
    from mvsnet_amd.model import DepthPlan, wta_depth_values
    Hh, Ww, Dd = SR.CAMERA_SHAPE
    c, ref = SR.case_scores("normal", Hh, Ww, Dd, cams=SR.family_cams(name))
    plan = DepthPlan(3, Dd, Hh, Ww, c["C"], gru_weights(), "GRU", DEV)
    interval = float((np.float32(c["end"]) - np.float32(c["start"])) / (np.float32(Dd) - np.float32(1)))
    plan.set_cameras(t(c["cams"]), c["start"], interval, c["end"], False)
    try:
        L.set_conv_impl(impl)
        d, p = plan.run_gru(t(c["features"]), wta_depth_values(Dd, c["start"], c["end"], False))
        torch.cuda.synchronize()
        d, p = d.cpu().numpy(), p.cpu().numpy()
    finally:
        L.set_conv_impl("auto")
    SR.check_every_pixel(d, p, ref, "recurrent sweep %s %s" % (name, impl))
