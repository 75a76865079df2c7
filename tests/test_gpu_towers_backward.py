"""The UNetDS2GN training towers' backward pass (mvsnet_amd/feature_net_train.py, `HipTowers`) against float64 torch-CPU
autograd of the same network (oracle/torch_grad.py `unet_ds2gn`; TensorFlow's autodiff supplies these gradients in the
reference, mvsnet/train.py:428-429): the whole towers, every input-gradient convolution the backward launches through the
C ABI, and the GroupNorm backward with its totals over the views.

The whole-tower bound is measured, not chosen: the same oracle run in float32 on the CPU gives the float32 noise floor of
this computation, the device gets three times the largest per-tensor distance of that run (another float32 summation
order, not another arithmetic -- the margin tests/test_gpu_full_size.py uses).  tests/test_towers_oracle_host.py shows on
the CPU that this bound rejects a wrong kernel tap, a view missing from the gamma / beta totals and a dropped border column.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_grad as TG
from mvsnet_amd import synthetic as S
from _helpers import tensor_distance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 3.0                      # device bound = MARGIN x the float32 CPU oracle's largest distance from float64

# ---- the cases: every ("bwd", name) job of _WeightPlan for `normal` mode, as (cin_tot, cout) of the FORWARD layer ----
# (tests/test_towers_oracle_host.py holds these lists to an enumeration of the tower's layer table)
STRIDE1 = [(8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (16, 8), (32, 16), (64, 32), (128, 64)]
STRIDE2 = [(16, 32), (32, 64), (64, 128)]
TRANSPOSED = [(128, 64), (64, 32), (32, 16), (16, 8)]           # (Cin, Cout) of a deconv kernel (3,3,Cout,Cin)
STRIDE2_EXTRA = [(8, 16)]         # not a layer of the towers: the smallest pair the transposed-conv kernel takes in this role
LAYER_SIZES = [(2, 10, 20), (1, 6, 34)]                          # V, h, w of the SMALL side: ragged 16-column tiles on both axes
HOOKS = {"default": {}, "tile": {"unet_persistent": 0}, "grid3": {"unet_grid": 3}}
GN_CASES = [(8, 24 * 40), (16, 12 * 20), (64, 6 * 10), (128, 4 * 6)]       # C, hw; V = 3
GN_NEAR_ZERO = 1e-5               # |pre-activation| below which the ReLU's sign may legitimately differ in float32


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy().astype(np.float64)


# ---- 3.1 whole towers ------------------------------------------------------------------------------------------------

def tower_problem(V, H, W):
    """images, parameters with non-trivial GroupNorm affines, and the cotangent of the features: numpy float32."""
    params = S.make_unet_params("normal", seed=3)
    rs = np.random.RandomState(1)
    for name in params:
        if "gamma" in params[name]:
            params[name]["gamma"] = (1.0 + 0.2 * rs.randn(*params[name]["gamma"].shape)).astype(np.float32)
            params[name]["beta"] = (0.1 * rs.randn(*params[name]["beta"].shape)).astype(np.float32)
    return S.make_images(V, H, W, seed=4), params, rs.randn(V, H // 4, W // 4, 32).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tower_reference(V, H, W):
    """(float64 features, float64 gradients, float32-CPU distance of the features, of every gradient) -- computed once per size
    and shared; nobody writes to it."""
    images, params, g = tower_problem(V, H, W)
    f64, g64 = TG.unet_ds2gn_gradients(images, params, g, torch.float64)
    f32, g32 = TG.unet_ds2gn_gradients(images, params, g, torch.float32)
    return f64, g64, tensor_distance(f32, f64), {k: tensor_distance(g32[k], g64[k]) for k in g64}


def _device_towers(V, H, W, into, fill):
    from mvsnet_amd.feature_net_train import flatten_unet_params, hip_towers
    images, params, g = tower_problem(V, H, W)
    p = {name: {key: t(v).requires_grad_(True) for key, v in d.items()} for name, d in params.items()}
    if into:                                                   # the trainer's mode: .grad slices of one flat buffer, ADDED to
        leaves = flatten_unet_params(p)
        flat = torch.full((sum(x.numel() for x in leaves),), fill, dtype=torch.float32, device=DEV)
        off = 0
        for x in leaves:
            x.grad = flat[off:off + x.numel()].view(x.shape)
            off += x.numel()
    f = hip_towers(t(images), p, accumulate_into_grads=into)
    (f * t(g)).sum().backward()
    grads = {(name, key): n(x.grad) - (fill if into else 0.0) for name, d in p.items() for key, x in d.items()}
    return n(f), grads


@pytest.mark.parametrize("size,hooks,into", [((2, 32, 48), "default", False), ((2, 32, 48), "default", True),
                                             ((3, 48, 80), "default", False), ((3, 48, 80), "tile", False),
                                             ((3, 48, 80), "grid3", False)])
def test_hip_towers_match_float64_autograd(size, hooks, into, lib_built):
    """HipTowers forward + backward against the float64 oracle: the features and all 94 parameter gradients, each within
    3 x the largest distance the float32 CPU oracle has from float64 on any gradient tensor.  2 x 32 x 48: the coarsest level is
    2 x 3; 3 x 48 x 80: odd tile counts on both axes at every level, three views for the per-view GroupNorm and the totals over
    the views, under the default schedule, the one-tile-per-workgroup kernels (MVS_HOOK_UNET_PERSISTENT = 0) and multi-tile
    persistent ranges (MVS_HOOK_UNET_GRID = 3).  `into`: the gradients ADDED into slices of a flat buffer pre-filled with a
    constant -- a power of two no larger than the smallest max |gradient| of the reference, so that adding and removing it costs
    no more than a float32 rounding of the gradient itself.

    Measured on an MI355X (worst tensor of each run; bound = 3 x the float32 CPU floor):
      size, schedule, path            float32 CPU floor   bound       worst device tensor             share of the bound
      2 x 32 x 48, default, returned  2.66e-06            7.99e-06    2dconv1_0 beta   3.51e-06       44 %
      2 x 32 x 48, default, flat      2.66e-06            7.99e-06    2dconv1_0 beta   3.51e-06       44 %
      3 x 48 x 80, default            3.30e-06            9.89e-06    2dconv3_1 gamma  2.49e-06       25 %
      3 x 48 x 80, tile kernels       3.30e-06            9.89e-06    conv10_0 gamma   2.55e-06       26 %
      3 x 48 x 80, 3 workgroups       3.30e-06            9.89e-06    conv10_0 gamma   2.52e-06       26 %
    (features: 0.93e-06 .. 1.31e-06 on the device, 1.08e-06 for the float32 CPU oracle.  The floor depends on the host's float32
    summation order: 3.24e-06 at 2 x 32 x 48 on another CPU.)
    """
    from mvsnet_amd import _lib as L
    f64, g64, f32_dist, g32_dist = tower_reference(*size)
    assert len(g64) == 94
    floor = max(g32_dist.values())
    bound = MARGIN * floor
    fill = 2.0 ** np.floor(np.log2(min(np.abs(v).max() for v in g64.values())))
    with L.test_hooks(**HOOKS[hooks]):
        f, grads = _device_towers(*size, into, fill)
    rows = [("features", "", tensor_distance(f, f64), f32_dist)]
    rows += [(name, key, tensor_distance(grads[name, key], g64[name, key]), g32_dist[name, key]) for name, key in g64]
    print("\n%s hooks=%s into=%s: float32 CPU floor %.3e, bound %.3e" % (size, hooks, into, floor, bound))
    print("%-12s %-6s %12s %12s %8s" % ("layer", "tensor", "device", "cpu float32", "of bound"))
    for name, key, d, c in rows:
        print("%-12s %-6s %12.3e %12.3e %7.1f%%" % (name, key, d, c, 100.0 * d / bound))
    worst = max(rows, key=lambda r: r[2])
    print("worst: %s %s %.3e = %.1f%% of the bound" % (worst[0], worst[1], worst[2], 100.0 * worst[2] / bound))
    bad = [(name, key, d) for name, key, d, _c in rows if not d <= bound]
    assert not bad, (bound, bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
@pytest.mark.parametrize("size", [(2, 32, 48), (3, 48, 80)])
def test_training_forward_is_the_inference_forward(size, dtype, lib_built):
    """`hip_towers` and `HipUNetDS2GN` launch their layers through one function (feature_net_hip.launch_layer): the same
    launches, another order of the float64 GroupNorm atomics -- the 1e-6 tests/test_gpu_unet.py holds two such passes to."""
    from mvsnet_amd.feature_net_hip import HipUNetDS2GN
    from mvsnet_amd.feature_net_train import hip_towers
    images, params, _g = tower_problem(*size)
    img = t(images)
    if dtype == torch.uint8:
        img = torch.randint(0, 256, img.shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(size[2])).to(DEV)
    got = n(hip_towers(img, {name: {key: t(v) for key, v in d.items()} for name, d in params.items()}))
    want = n(HipUNetDS2GN(params, DEV, side_streams=0)(img))
    dist = np.abs(got - want).max() / np.abs(want).max()
    print("\n%s %s: max |training - inference| / max |inference| = %.3e" % (size, dtype, dist))
    assert got.shape == want.shape == (size[0], size[1] // 4, size[2] // 4, 32) and dist < 1e-6, dist


def test_weight_plan_jobs_are_the_cases_of_this_file(lib_built):
    """What `_WeightPlan` really prepares for the backward on this device = the case lists above."""
    from mvsnet_amd.feature_net import UNET_LAYERS
    from mvsnet_amd.feature_net_train import _WeightPlan
    params = S.make_unet_params("normal", seed=3)
    plan = _WeightPlan({name: t(params[name]["w"]) for name in params}, torch.device(DEV))
    got = {"stride1": set(), "stride2": set(), "transposed": set()}
    for name, kind, _srcs, _k, _mult, stride in UNET_LAYERS:
        if ("bwd", name) in plan.prepared:
            w = params[name]["w"]
            route = "transposed" if kind == "dg" else ("stride1" if stride == 1 else "stride2")
            got[route].add((w.shape[3], w.shape[2]) if kind == "dg" else (w.shape[2], w.shape[3]))
    assert got == {"stride1": set(STRIDE1), "stride2": set(STRIDE2), "transposed": set(TRANSPOSED)}


# ---- 3.2 the input-gradient convolutions, layer by layer -----------------------------------------------------------------

def _prepare(lib, L, kind, w, c1, cout, floats, many):
    """kind as in mvs_unet_prepare_many_f32: 0 forward layout, 1 input-gradient layout, 2 transposed-conv layout."""
    prep = torch.full((floats,), float("nan"), dtype=torch.float32, device=DEV)
    st = L.stream_ptr()
    if many:
        one = lambda v: (C.c_int * 1)(v)
        L.check(lib.mvs_unet_prepare_many_f32(1, one(kind), (C.c_void_p * 1)(w.data_ptr()), one(3), one(c1), one(0), one(c1), one(cout),
                                              (C.c_void_p * 1)(prep.data_ptr()), st), "mvs_unet_prepare_many_f32")
    elif kind == 1:
        L.check(lib.mvs_conv2d_prepare_dgrad_f32(L.ptr(w), 3, c1, cout, L.ptr(prep), st), "mvs_conv2d_prepare_dgrad_f32")
    elif kind == 2:
        L.check(lib.mvs_deconv2d_prepare_f32(L.ptr(w), c1, cout, L.ptr(prep), st), "mvs_deconv2d_prepare_f32")
    else:
        L.check(lib.mvs_conv2d_prepare_f32(L.ptr(w), 3, c1, 0, cout, L.ptr(prep), st), "mvs_conv2d_prepare_f32")
    return prep


def _input_gradient_case(route, pair, size, many):
    """One layer's input gradient the way HipTowers.backward launches it, against float64 autograd of the forward layer."""
    from mvsnet_amd import _lib as L
    lib = L.load()
    V, h, w_ = size
    rs = np.random.RandomState(1000 * pair[0] + pair[1] + h)
    st = L.stream_ptr()
    d64 = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64)).requires_grad_(grad)
    if route == "transposed":                                  # forward: x (V,h,w,Cin) -> y (V,2h,2w,Cout), kernel (3,3,Cout,Cin)
        cin, cout = pair
        wk = (rs.randn(3, 3, cout, cin) / np.sqrt(9 * cin)).astype(np.float32)
        gy = rs.randn(V, 2 * h, 2 * w_, cout).astype(np.float32)
        x64 = d64(np.zeros((V, h, w_, cin)), True)
        y64 = TG.deconv2d_same(x64, d64(wk))
    else:                                                      # forward: x (V,sh,sw,cin) -> y (V,h,w,cout), kernel (3,3,cin,cout)
        cin, cout = pair
        s = 1 if route == "stride1" else 2
        wk = (rs.randn(3, 3, cin, cout) / np.sqrt(9 * cin)).astype(np.float32)
        gy = rs.randn(V, h, w_, cout).astype(np.float32)
        x64 = d64(np.zeros((V, s * h, s * w_, cin)), True)
        y64 = TG.conv2d_same(x64, d64(wk), s)
    assert tuple(y64.shape) == gy.shape
    (y64 * d64(gy)).sum().backward()
    exp = x64.grad.numpy()
    tw, tgy = t(wk), t(gy)
    gx = torch.full(exp.shape, float("nan"), dtype=torch.float32, device=DEV)
    gh, gw = gy.shape[1:3]
    if route == "stride1":                                     # convolution over g_y with the mirrored, transposed kernel
        prep = _prepare(lib, L, 1, tw, cin, cout, lib.mvs_conv2d_prepared_floats(3, cout, 0, cin), many)
        L.check(lib.mvs_conv2d_gn_f32(L.ptr(tgy), None, None, None, cout, 0, None, None, None, None, 0, 0, L.ptr(prep), V, gh, gw, cin, 3, 1,
                                      L.ptr(gx), None, st), "mvs_conv2d_gn_f32")
    elif route == "stride2":                                   # transposed convolution of g_y with the same array
        floats = lib.mvs_deconv2d_prepared_floats(cout, cin)
        assert floats > 0
        prep = _prepare(lib, L, 2, tw, cout, cin, floats, many)
        L.check(lib.mvs_deconv2d_gn_f32(L.ptr(tgy), None, None, None, cout, 0, L.ptr(tw), L.ptr(prep), V, gh, gw, cin, L.ptr(gx), None, st),
                "mvs_deconv2d_gn_f32")
    else:                                                      # stride-2 convolution over g_y with the same array
        prep = _prepare(lib, L, 0, tw, cout, cin, lib.mvs_conv2d_prepared_floats(3, cout, 0, cin), many)
        L.check(lib.mvs_conv2d_gn_f32(L.ptr(tgy), None, None, None, cout, 0, None, None, None, None, 0, 0, L.ptr(prep), V, gh, gw, cin, 3, 2,
                                      L.ptr(gx), None, st), "mvs_conv2d_gn_f32")
    got = n(gx)
    assert torch.isfinite(prep).all()                          # every float of the layout was written
    np.testing.assert_allclose(got, exp, rtol=2e-4, atol=2e-4, err_msg=str((route, pair, size, many)))


ROUTE_CASES = ([("stride1", p_) for p_ in STRIDE1] + [("stride2", p_) for p_ in STRIDE2 + STRIDE2_EXTRA] +
               [("transposed", p_) for p_ in TRANSPOSED])


@pytest.mark.parametrize("route,pair", ROUTE_CASES)
def test_input_gradient_convolutions_match_float64_autograd(route, pair, lib_built):
    """Every (route, channel pair) of the towers' backward: the single preparation + the forward kernel in its input-gradient
    role (no GroupNorm on the load, no statistics out), element by element against float64 autograd of TG.conv2d_same /
    TG.deconv2d_same -- the layers are linear; rtol = atol = 2e-4 as test_conv2d_gn_matches_oracle holds the same kernels to."""
    for size in LAYER_SIZES:
        _input_gradient_case(route, pair, size, many=False)


@pytest.mark.parametrize("route,pair", [("stride1", (32, 16)), ("stride2", (32, 64)), ("transposed", (64, 32))])
def test_input_gradient_layouts_through_prepare_many(route, pair, lib_built):
    """The same layouts laid out by mvs_unet_prepare_many_f32 (what the towers call), kinds 1, 2 and 0 in their swapped roles."""
    for size in LAYER_SIZES:
        _input_gradient_case(route, pair, size, many=True)


@pytest.mark.parametrize("hooks", ["tile", "grid3"])
@pytest.mark.parametrize("pair", [(32, 32), (128, 64)])
def test_stride1_input_gradients_under_the_schedule_hooks(pair, hooks, lib_built):
    from mvsnet_amd import _lib as L
    with L.test_hooks(**HOOKS[hooks]):
        for size in LAYER_SIZES:
            _input_gradient_case("stride1", pair, size, many=False)


# ---- 3.3 GroupNorm backward with the totals over the views -----------------------------------------------------------------

def gn_problem(Cn, hw, relu, V=3):
    """Inputs (numpy float32) and the float64 reference of one GroupNorm(+ReLU) backward: x, gamma, beta, g, and
    (pre-activation, dx, d beta, d gamma)."""
    rs = np.random.RandomState(Cn + relu)
    x = (rs.randn(V, hw, Cn) * 1.3 + 0.2).astype(np.float32)
    gamma = (1.0 + 0.3 * rs.randn(Cn)).astype(np.float32); beta = (0.2 * rs.randn(Cn)).astype(np.float32)
    g = rs.randn(V, hw, Cn).astype(np.float32)
    d64 = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64)).requires_grad_(grad)
    xx, gg, bb = d64(x, True), d64(gamma, True), d64(beta, True)
    pre = F.group_norm(xx.permute(0, 2, 1), Cn // 8, gg, bb, eps=1e-5).permute(0, 2, 1)
    ((F.relu(pre) if relu else pre) * d64(g)).sum().backward()
    return (x, gamma, beta, g), (pre.detach().numpy(), xx.grad.numpy(), bb.grad.numpy(), gg.grad.numpy())


def gn_excluded(pre, relu):
    """Elements whose ReLU gate is not decided at float32: left out of the dx comparison."""
    return (np.abs(pre) < GN_NEAR_ZERO) if relu else np.zeros(pre.shape, bool)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("Cn,hw", GN_CASES)
def test_gn_backward_with_totals_matches_float64_autograd(Cn, hw, relu, lib_built):
    """mvs_gn_bwd_reduce_f32 + mvs_gn_bwd_apply_tot_f32 as the towers call them: dx element by element, and d beta / d gamma
    ADDED to pre-filled totals by the launch's first workgroup only ((8, 24 x 40) runs several workgroups per view)."""
    from mvsnet_amd import _lib as L
    lib = L.load()
    V, const = 3, 0.75
    (x, gamma, beta, g), (pre, dx64, db64, dg64) = gn_problem(Cn, hw, relu, V)
    if Cn == 8:
        assert (hw * (Cn // 4) + 255) // 256 > 1               # more than one workgroup per view
    skip = gn_excluded(pre, relu)
    assert skip.mean() <= 1e-3
    x64 = x.astype(np.float64)
    stats = t(np.stack([x64.sum(1), (x64 * x64).sum(1)], 1), torch.float64)            # (V, 2, C): exact channel sums
    sums = torch.zeros(lib.mvs_gn_bwd_sums_doubles(V, Cn), dtype=torch.float64, device=DEV)
    totals = torch.full((2, Cn), const, dtype=torch.float64, device=DEV)
    tx, tga, tbe, tg = t(x), t(gamma), t(beta), t(g)
    dx = torch.full((V, hw, Cn), float("nan"), dtype=torch.float32, device=DEV)
    args = (L.ptr(tx), L.ptr(stats), L.ptr(tga), L.ptr(tbe), 1e-5, relu, L.ptr(tg))
    st = L.stream_ptr()
    L.check(lib.mvs_gn_bwd_reduce_f32(*args, V, hw, Cn, L.ptr(sums), st), "mvs_gn_bwd_reduce_f32")
    L.check(lib.mvs_gn_bwd_apply_tot_f32(*args, L.ptr(sums), L.ptr(totals), V, hw, Cn, L.ptr(dx), st), "mvs_gn_bwd_apply_tot_f32")
    tot = n(totals) - const
    got = n(dx)
    err = np.abs(tot - np.stack([db64, dg64])) / np.abs(np.stack([db64, dg64]))
    print("\nC=%d hw=%d relu=%d: totals worst relative error %.2e, dx worst |error| %.2e, excluded %d" %
          (Cn, hw, relu, err.max(), np.abs(got - dx64)[~skip].max(), int(skip.sum())))
    np.testing.assert_allclose(tot[0], db64, rtol=1e-5, atol=0)
    np.testing.assert_allclose(tot[1], dg64, rtol=1e-5, atol=0)
    np.testing.assert_allclose(got[~skip], dx64[~skip], rtol=1e-4, atol=1e-5)
