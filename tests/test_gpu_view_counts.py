"""Every view count the cost-volume launchers branch on, forward and backward, against the float64 oracle.

cost_volume.hip instantiates the depth sweep for 1..7 source views; from 5 on its per-plane LDS table holds a second quad of block
offsets (NOF = 2, read as ofq[v >> 2], table stride ENT = NSRC + NOF); 9 views and more, and channel counts whose C/4 is no power of
two, take the per-plane kernel.  backward.hip unrolls its kernels over 1..8 source views and answers MVS_E_SHAPE beyond.  The inputs
come from tests/view_count_cases.py, whose preconditions tests/test_view_count_cases_host.py asserts on the CPU: on band_case a view
that is blended with another view's block, weights or offsets cannot give the right plane.

    view_num   2 .. 8   cost_volume_sweep_kernel<NSRC = view_num - 1>; 6, 7, 8: two offset quads
               9, 10    cost_volume_kernel (per plane)
    backward   2 .. 9   cost_volume_bwd_kernel / cvb_pass1_kernel <NSRC>; 10: MVS_E_SHAPE
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from oracle import torch_grad as TG
from mvsnet_amd import synthetic as S
from mvsnet_amd import _lib as L

from tests import sweep_reference as SR
from tests import view_count_cases as V
from tests.device_arena import PATTERNS, Arena

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_SHAPE = -2      # MVS_E_SHAPE
BH, BW, BD = 6, 10, 24                       # band_case on the GPU: 6 x 10 pixels, 24 planes (one period of the shifts)


@functools.lru_cache(maxsize=None)
def gru_weights():
    from mvsnet_amd.model import MVSNetWeights
    gp = S.make_gru_params("normal", seed=2, in_channels=32, random_affine=True)
    return gp, MVSNetWeights.from_numpy("normal", gru=gp, device=DEV)


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


@pytest.fixture(scope="module")
def stream_set():
    """Holds the recurrent sweep's stream set for the sweep tests of this file: one calibration."""
    from mvsnet_amd.model import DepthPlan
    keep = DepthPlan(3, 2, 8, 16, 32, gru_weights()[1], "GRU", DEV)
    yield
    keep.close()


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


def d64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64)).requires_grad_(grad)


# ---- exact bands -----------------------------------------------------------------------------------------------------------------
def hold_bands(n_src, Cc, variant, negate):
    """band_case against the float64 oracle at rtol = 0, atol = 2e-5 (sums of exact products of small integers and 1/16ths are exact
    in float32; the 1/N scalings round once each: test_gpu_parity.test_cost_volume_border_bands_are_exact): the whole volume, every
    plane launched alone, and a sub-range that starts and ends inside the table."""
    from mvsnet_amd.model import cost_volume
    ref, src, T = V.band_case(n_src, BH, BW, Cc, BD)
    exp = V.band_expected(n_src, BH, BW, Cc, BD, variant) * (-1.0 if negate else 1.0)
    rt, st, Tt = t(ref), t(src), t(T)
    got = n(cost_volume(rt, st, Tt, variant=variant, negate=negate))
    assert got.shape == (BD, BH, BW, Cc)
    for d in range(BD):
        np.testing.assert_allclose(got[d], exp[d], rtol=0, atol=2e-5, err_msg="plane %d" % d)
    alone = n(torch.cat([cost_volume(rt, st, Tt, d_begin=d, d_count=1, variant=variant, negate=negate) for d in range(BD)]))
    for d in range(BD):
        np.testing.assert_allclose(alone[d], exp[d], rtol=0, atol=2e-5, err_msg="plane %d alone" % d)
        np.testing.assert_allclose(alone[d], got[d], rtol=0, atol=2e-5, err_msg="plane %d alone against the whole launch" % d)
    b, c = 5, 13                                 # planes 5 .. 17: neither end is an end of the table, 13 is no multiple of the lanes per pixel
    sub = n(cost_volume(rt, st, Tt, d_begin=b, d_count=c, variant=variant, negate=negate))
    assert sub.shape == (c, BH, BW, Cc)
    for k in range(c):
        np.testing.assert_allclose(sub[k], exp[b + k], rtol=0, atol=2e-5, err_msg="plane %d of the sub-range" % (b + k))


@pytest.mark.parametrize("variant", ["mem", "eager"])
@pytest.mark.parametrize("Cc", [8, 32, 64])
@pytest.mark.parametrize("view_num", range(2, 11))
def test_cost_volume_exact_bands_at_every_view_count(view_num, Cc, variant):
    """2, 8 and 16 lanes per pixel; the eager variant negated (the recurrent sweep's input), the mem variant as it is."""
    hold_bands(view_num - 1, Cc, variant, negate=(variant == "eager"))


@pytest.mark.parametrize("variant", ["mem", "eager"])
def test_cost_volume_exact_bands_with_twelve_channels(variant):
    """C / 4 = 3 lanes per pixel is no power of two: the other way into the per-plane kernel, at 3 views."""
    hold_bands(2, 12, variant, negate=(variant == "eager"))


# ---- projective ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", V.CAMERA_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
@pytest.mark.parametrize("N", V.CAMERA_VIEW_COUNTS)
def test_cost_volume_projective_at_every_view_count(N, shape):
    """camera_case at the bounds of test_cost_volume_wave_tile_shapes_give_the_same_bits (the float32 oracle itself: rel-L1 <= 4.9e-7,
    no voxel off by 1e-4 -- host file); at 7 views every forced wave-tile shape and the voted one give the same bits."""
    from mvsnet_amd.model import cost_volume
    Hh, Ww, Cc, D = shape
    c = V.camera_case(N, Hh, Ww, Cc, D)
    ft, Tt = t(c["features"]), t(c["t8"])
    L.set_test_hook("cv_tile_rows_log2", -1)
    for variant in ("mem", "eager"):
        got = n(cost_volume(ft[0], ft[1:], Tt, variant=variant))
        exp = V.camera_expected(N, Hh, Ww, Cc, D, variant)
        rel, share = rel_l1(got, exp), float((~(np.abs(got - exp) <= 1e-4)).mean())
        print("projective N=%d %s %s: rel-L1 %.3g, share of voxels off by more than 1e-4: %.3g" % (N, shape, variant, rel, share))
        assert np.isfinite(got).all() and got.any()
        assert rel < 1e-5
        assert share < 2e-3
        if N == 7:
            for rows_log2 in range(4):
                with L.test_hooks(cv_tile_rows_log2=rows_log2):
                    forced = n(cost_volume(ft[0], ft[1:], Tt, variant=variant))
                assert np.array_equal(forced, got), rows_log2


# ---- homographies ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("N", [2, 7, 10])
def test_homographies_at_other_view_counts(N, inverse):
    """D = 130: (N - 1) * D = 130, 780, 1170 is no multiple of the launch's 128-thread block.  Bounds of test_homographies_match_oracle."""
    from mvsnet_amd.homography_warping import homography_transforms
    D, start, interval = 130, 425.0, 2.65
    cams = S.make_cams(N, 128, 160, D, interval=interval)
    end = start + (D - 1) * interval
    T, Hm = homography_transforms(t(cams), D, start, interval, end, inverse, True)
    T, Hm = n(T), n(Hm)
    assert T.shape == (N - 1, D, 8) and Hm.shape == (N - 1, D, 3, 3)
    for v in range(1, N):
        if inverse:
            Ho = O.get_homographies_inv_depth(cams[0], cams[v], D, start, end, np.float64)
        else:
            Ho = O.get_homographies(cams[0], cams[v], D, start, interval, np.float64)
        np.testing.assert_allclose(Hm[v - 1], Ho, rtol=2e-5, atol=2e-4)
        np.testing.assert_allclose(T[v - 1], O.homography_to_transform8(Ho, np.float64), rtol=2e-5, atol=2e-4)


# ---- features to depth -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 4, 7, 9])
def test_features_to_depth_at_other_view_counts(N):
    """inference_mem(features=...) (mvs_depth_from_features_f32) and DepthPlan.set_cameras + run_3dcnn, at the toy size, against
    O.inference_mem_from_features in float64 at the bounds of test_inference_mem_from_features_matches_oracle."""
    from mvsnet_amd.model import DepthPlan, MVSNetWeights, inference_mem
    D, Hh, Ww, Cc, interval = 8, 16, 16, 32, 60.0
    cams = S.make_cams(N, Hh, Ww, D, interval=interval)
    feats = S.make_features(N, Hh, Ww, Cc)
    start = float(cams[0, 1, 3, 0])
    rp = S.make_regnet_params("normal", seed=1, random_affine=True)
    weights = MVSNetWeights.from_numpy("normal", regnet=rp, device=DEV)
    ed, ep = O.inference_mem_from_features(feats, cams, D, start, interval, rp, False, np.float64)

    def hold(depth, prob, tag):
        abs_rel = float(np.mean(np.abs(depth - ed) / ed))
        share = float((~(np.abs(prob - ep) <= 1e-3)).mean())
        print("features to depth N=%d %s: abs-rel %.3g, prob share off by more than 1e-3: %.3g" % (N, tag, abs_rel, share))
        assert abs_rel < 1e-4, (tag, abs_rel)
        assert share < 0.02, (tag, share)

    depth, prob = inference_mem(None, t(cams)[None], D, start, interval, weights=weights, features=t(feats))
    assert depth.shape == (1, Hh, Ww, 1)
    hold(n(depth)[0, :, :, 0], n(prob)[0, :, :, 0], "one call")
    plan = DepthPlan(N, D, Hh, Ww, Cc, weights, "3DCNN", DEV)
    plan.set_cameras(t(cams), start, interval, start + (D - 1) * interval, False)
    d2, p2 = plan.run_3dcnn(t(feats), start, interval)
    hold(n(d2), n(p2), "set_cameras + run_3dcnn")


# ---- recurrent sweep -------------------------------------------------------------------------------------------------------------
def sweep_problem(N, D):
    """The toy workload's 16 x 16 x 32 maps at N views; D = 8 is toy's own, D = 19 keeps its depth range (interval 25)."""
    interval = 60.0 if D == 8 else 25.0
    cams = S.make_cams(N, 16, 16, D, interval=interval)
    feats = S.make_features(N, 16, 16, 32)
    start = float(cams[0, 1, 3, 0])
    return feats, cams, start, start + (D - 1) * interval


def run_sweep(N, D, form=0, **hooks):
    from mvsnet_amd.model import inference_winner_take_all
    feats, cams, start, end = sweep_problem(N, D)
    lib = L.load()
    L.check(lib.mvs_gru_set_formulation(form), "mvs_gru_set_formulation")
    try:
        with L.test_hooks(**hooks):
            d, p = inference_winner_take_all(None, t(cams)[None], D, start, end, weights=gru_weights()[1], features=t(feats))
            torch.cuda.synchronize()
    finally:
        L.check(lib.mvs_gru_set_formulation(0), "mvs_gru_set_formulation")
    return d[0, :, :, 0].clone(), p[0, :, :, 0].clone()


@pytest.mark.parametrize("D", [8, 19])
@pytest.mark.parametrize("N", [2, 7, 9])
def test_recurrent_sweep_at_other_view_counts(stream_set, N, D):
    """inference_winner_take_all through sweep_reference.check_every_pixel on the default route, the wavefront route and on one
    stream.  At toy's 8 planes every route stays on the caller's stream (the producer stream is taken from 17 planes on, the
    wavefront from 9 on: gru_sweep.hip) and its producer is the 256-thread sweep; 19 planes reach the 128-thread producer on its
    own stream, a second cost batch of 3 planes and the wavefront proper.  9 views: the per-plane kernel as the producer."""
    feats, cams, start, end = sweep_problem(N, D)
    ref = SR.plane_scores(feats, cams, D, start, end, gru_weights()[0], False)
    for tag, route in (("default", dict()), ("wavefront", dict(form=1)), ("one stream", dict(gru_one_stream=1))):
        d, p = run_sweep(N, D, **route)
        SR.check_every_pixel(d.cpu().numpy(), p.cpu().numpy(), ref, "N=%d D=%d %s" % (N, D, tag))


def test_recurrent_sweep_producer_workgroup_sizes_at_seven_views(stream_set):
    """The producer launches the sweep with 64 .. 192 threads: its LDS table is threads / 64 * 64 * (NSRC + NOF) * 16 bytes, 9 KB
    per wave at 7 views.  On a prepared stream with 19 planes (the producer stream is not taken below 17), the depth map of every
    size is bit-equal to the 128-thread run, which is held to the oracle."""
    N, D = 7, 19
    feats, cams, start, end = sweep_problem(N, D)
    d0, p0 = run_sweep(N, D)
    SR.check_every_pixel(d0.cpu().numpy(), p0.cpu().numpy(), SR.plane_scores(feats, cams, D, start, end, gru_weights()[0], False),
                         "N=7 D=19 producer of 128 threads")
    for threads in (64, 192):
        d, p = run_sweep(N, D, gru_producer_threads=threads)
        assert torch.equal(d, d0) and torch.equal(p, p0), threads


# ---- backward --------------------------------------------------------------------------------------------------------------------
def camera_problem(N, D, Hh, Ww, Cc):
    """As test_gpu_backward._toy_problem builds it."""
    cams = S.make_cams(N, Hh, Ww, D)
    feats = S.make_features(N, Hh, Ww, Cc, seed=5)
    start, interval = float(cams[0, 1, 3, 0]), float(cams[0, 1, 3, 1])
    Hs = np.stack([O.get_homographies(cams[0], cams[v], D, start, interval, np.float32) for v in range(1, N)])
    return feats, O.homography_to_transform8(Hs, np.float32), start, interval


@functools.lru_cache(maxsize=None)
def cost_backward_case(n_src, Cc):
    """8 x 12 pixels, 50 planes: pass 1's chunks of 48 planes and pass 2's of 24 both end in a chunk of 2.  -> inputs and the float64
    autograd gradient (N,H,W,C), shared by the two methods."""
    feats, t8, _, _ = camera_problem(n_src + 1, 50, 8, 12, Cc)
    rs = np.random.RandomState(3)
    g1 = rs.randn(t8.shape[1], *feats.shape[1:]).astype(np.float32)
    g2 = rs.randn(*g1.shape).astype(np.float32)
    f = d64(feats, True)
    cost = TG.cost_volume(f, d64(t8)).permute(1, 2, 3, 0)               # (D,H,W,C)
    (cost * (d64(g1) + d64(g2))).sum().backward()
    return feats, t8, g1, g2, f.grad.numpy()


@pytest.mark.parametrize("method", ["gather", "scatter"])
@pytest.mark.parametrize("n_src,Cc", [(3, 32), (5, 32), (6, 32), (7, 32), (8, 32), (7, 16)])
def test_cost_volume_backward_at_other_view_counts(n_src, Cc, method):
    from mvsnet_amd import backward as B
    feats, t8, g1, g2, exp = cost_backward_case(n_src, Cc)
    ft = t(feats)
    g_ref, g_src = B.cost_volume_bwd(ft[0], ft[1:], t(t8), t(g1), t(g2), method=method)
    got = np.concatenate([n(g_ref)[None], n(g_src)], 0).astype(np.float64)
    if method == "gather":                       # bit-reproducible
        r2, s2 = B.cost_volume_bwd(ft[0], ft[1:], t(t8), t(g1), t(g2), method=method)
        assert torch.equal(r2, g_ref) and torch.equal(s2, g_src)
    err = rel_l1(got, exp)
    per_view = [rel_l1(got[v], exp[v]) for v in range(n_src + 1)]
    print("cost volume backward %d source views C=%d %s: rel-L1 %.3g, worst view %.3g" % (n_src, Cc, method, err, max(per_view)))
    assert err < 1e-4
    assert max(per_view) < 1e-4, per_view        # (a view that received another view's gradient hides in the sum over all of them)


def test_backward_refuses_ten_views():
    """9 source views are one more than the backward kernels unroll over: both C entries answer MVS_E_SHAPE and launch nothing
    (outputs pre-filled with 7.0 stay as they are), and the Python entry points raise instead of returning what was never written."""
    from mvsnet_amd import backward as B
    lib = L.load()
    N, D, Hh, Ww, Cc = 10, 4, 8, 12, 32
    feats, t8, start, interval = camera_problem(N, D, Hh, Ww, Cc)
    ft, Tt = t(feats), t(t8)
    g1 = torch.ones((D, Hh, Ww, Cc), device=DEV)
    need = lib.mvs_cost_volume_bwd_workspace_bytes(N, D, Hh, Ww, Cc)
    ws = torch.empty(max(need, 16), device=DEV, dtype=torch.uint8)
    for entry in ("scatter", "gather"):
        g_ref = torch.full((Hh, Ww, Cc), 7.0, device=DEV)
        g_src = torch.full((N - 1, Hh, Ww, Cc), 7.0, device=DEV)
        if entry == "scatter":
            rc = lib.mvs_cost_volume_bwd_f32(L.ptr(ft[0]), L.ptr(ft[1:]), L.ptr(Tt), N, D, Hh, Ww, Cc, L.ptr(g1), None, L.ptr(g_ref),
                                             L.ptr(g_src), L.stream_ptr())
        else:
            rc = lib.mvs_cost_volume_bwd_gather_f32(L.ptr(ft[0]), L.ptr(ft[1:]), L.ptr(Tt), N, D, Hh, Ww, Cc, L.ptr(g1), None,
                                                    C.c_void_p(ws.data_ptr()), ws.numel(), L.ptr(g_ref), L.ptr(g_src), L.stream_ptr())
        assert rc == E_SHAPE, entry
        assert float(n(g_ref).min()) == 7.0 == float(n(g_ref).max()) and float(n(g_src).min()) == 7.0 == float(n(g_src).max()), entry
        with pytest.raises(L.MvsnetHipError):
            B.cost_volume_bwd(ft[0], ft[1:], Tt, g1, None, method=entry)
    params = S.make_regnet_params("normal", seed=1, random_affine=True)
    pt = {k: {kk: t(vv).requires_grad_(True) for kk, vv in v.items()} for k, v in params.items()}
    feats, t8, start, interval = camera_problem(N, 8, 16, 16, Cc)
    fg = t(feats).requires_grad_(True)
    with pytest.raises(L.MvsnetHipError):
        depth, _prob = B.plane_sweep_depth(fg, t(t8), start, interval, pt)      # the forward has no such limit (per-plane kernel)
        depth.sum().backward()
    torch.cuda.synchronize()
    assert fg.grad is None


@pytest.mark.parametrize("N", [2, 6])
def test_plane_sweep_depth_gradients_at_other_view_counts(N):
    """test_gpu_backward.test_plane_sweep_depth_gradients_match_autograd (3 views) at 2 and 6, same size and the same 2e-3 bound."""
    from mvsnet_amd import backward as B
    feats, t8, start, interval = camera_problem(N, 16, 16, 32, 32)
    params = S.make_regnet_params("normal", seed=1, random_affine=True)
    g = np.random.RandomState(11).randn(feats.shape[1], feats.shape[2]).astype(np.float32)
    f64 = d64(feats, True)
    p64 = {k: {kk: d64(vv, True) for kk, vv in v.items()} for k, v in params.items()}
    depth64 = TG.depth_from_features(f64, d64(t8), start, interval, p64)
    (depth64 * d64(g)).sum().backward()
    ft = t(feats).requires_grad_(True)
    pt = {k: {kk: t(vv).requires_grad_(True) for kk, vv in v.items()} for k, v in params.items()}
    depth, _prob = B.plane_sweep_depth(ft, t(t8), start, interval, pt)
    assert rel_l1(n(depth), depth64.detach().numpy()) < 1e-5
    (depth * t(g)).sum().backward()
    got = n(ft.grad).astype(np.float64)
    print("plane_sweep_depth N=%d: feature gradient rel-L1 %.3g, per view %s" % (
        N, rel_l1(got, f64.grad.numpy()), ["%.3g" % rel_l1(got[v], f64.grad.numpy()[v]) for v in range(N)]))
    assert rel_l1(got, f64.grad.numpy()) < 2e-3
    for name in p64:
        for key in p64[name]:
            e = rel_l1(n(pt[name][key].grad), p64[name][key].grad.numpy())
            assert e < 2e-3, (name, key, e)


# ---- arena -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
@pytest.mark.parametrize("view_num", [8, 9])
def test_cost_volume_in_the_arena_at_eight_and_nine_views(view_num, pattern):
    """The sweep with the most views it is built for and the per-plane kernel just above, operands inside the poisoned, guarded
    arena.  The sweep reads the source maps through a buffer resource of NSRC * H * W * C * 4 bytes: band_case's planes put blocks
    in the last row and column of the LAST view and far outside every view, so a bound that is a view short returns zeros where the
    oracle has features, and a load past the last view picks up poison."""
    n_src, Cc = view_num - 1, 32
    ref, src, T = V.band_case(n_src, BH, BW, Cc, BD)
    a = Arena(2 << 20, pattern, DEV)
    f32 = torch.float32
    rt = a.take(ref.shape, f32, data=ref, readonly=True, name="ref")
    st = a.take(src.shape, f32, data=src, readonly=True, name="src")
    Tt = a.take(T.shape, f32, data=T, readonly=True, name="transforms")
    y = a.take((BD, BH, BW, Cc), f32, name="cost")
    L.check(L.load().mvs_cost_volume_f32(L.ptr(rt), L.ptr(st), L.ptr(Tt), view_num, BD, 0, BD, BH, BW, Cc, 0, 0, 0, L.ptr(y),
                                         L.stream_ptr()), "mvs_cost_volume_f32")
    got = n(y)
    a.check()
    exp = V.band_expected(n_src, BH, BW, Cc, BD, "mem")
    for d in range(BD):
        np.testing.assert_allclose(got[d], exp[d], rtol=0, atol=2e-5, err_msg="plane %d" % d)
