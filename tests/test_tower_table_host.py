"""The towers' layer table (mvsnet_amd/feature_net.py `tower_layers`) and the host pieces of the HIP towers that need neither
a GPU nor the library: channel counts, sizes and input-gradient routes against literals; `unet_macs` / `unet_layer_work`
against the values they returned before the table existed; the fork / join layers of the side branches; and the ATen step
of the training towers' backward (`feature_net_train.aten_step`) on CPU tensors against float64 autograd."""
import numpy as np
import pytest
import torch

from oracle import torch_grad as TG
from mvsnet_amd import synthetic as S
from mvsnet_amd import feature_net as FN
import test_gpu_towers_backward as G

# name, cin_tot (the image counted as the padded 4), cout, output size at 32 x 48, at 48 x 80
TABLE = [
    ("2dconv1_0", 4, 16, (16, 24), (24, 40)), ("2dconv2_0", 16, 32, (8, 12), (12, 20)), ("2dconv3_0", 32, 64, (4, 6), (6, 10)),
    ("2dconv4_0", 64, 128, (2, 3), (3, 5)), ("2dconv0_1", 4, 8, (32, 48), (48, 80)), ("2dconv0_2", 8, 8, (32, 48), (48, 80)),
    ("2dconv1_1", 16, 16, (16, 24), (24, 40)), ("2dconv1_2", 16, 16, (16, 24), (24, 40)), ("2dconv2_1", 32, 32, (8, 12), (12, 20)),
    ("2dconv2_2", 32, 32, (8, 12), (12, 20)), ("2dconv3_1", 64, 64, (4, 6), (6, 10)), ("2dconv3_2", 64, 64, (4, 6), (6, 10)),
    ("2dconv4_1", 128, 128, (2, 3), (3, 5)), ("2dconv4_2", 128, 128, (2, 3), (3, 5)), ("2dconv5_0", 128, 64, (4, 6), (6, 10)),
    ("2dconv5_1", 128, 64, (4, 6), (6, 10)), ("2dconv5_2", 64, 64, (4, 6), (6, 10)), ("2dconv6_0", 64, 32, (8, 12), (12, 20)),
    ("2dconv6_1", 64, 32, (8, 12), (12, 20)), ("2dconv6_2", 32, 32, (8, 12), (12, 20)), ("2dconv7_0", 32, 16, (16, 24), (24, 40)),
    ("2dconv7_1", 32, 16, (16, 24), (24, 40)), ("2dconv7_2", 16, 16, (16, 24), (24, 40)), ("2dconv8_0", 16, 8, (32, 48), (48, 80)),
    ("2dconv8_1", 16, 8, (32, 48), (48, 80)), ("2dconv8_2", 8, 8, (32, 48), (48, 80)), ("conv9_0", 8, 16, (16, 24), (24, 40)),
    ("conv9_1", 16, 16, (16, 24), (24, 40)), ("conv9_2", 16, 16, (16, 24), (24, 40)), ("conv10_0", 16, 32, (8, 12), (12, 20)),
    ("conv10_1", 32, 32, (8, 12), (12, 20)), ("conv10_2", 32, 32, (8, 12), (12, 20)),
]
FORK_JOIN = {"data", "2dconv0_2", "2dconv1_0", "2dconv1_2", "2dconv2_0", "2dconv2_2", "2dconv3_0", "2dconv3_2"}
# (H, W) -> unet_macs, and (multiply-adds, bytes) per layer of unet_layer_work in the order of UNET_LAYERS: what the functions
# returned when each of them walked UNET_LAYERS itself (base filter 8, three image channels)
WORK = {
    (512, 640): (6009651200.0, [
        (35389440, 9175040.0), (94371840, 7864320.0), (94371840, 3932160.0), (94371840, 1966080.0), (70778880, 14417920.0),
        (188743680, 20971520.0), (188743680, 10485760.0), (188743680, 10485760.0), (188743680, 5242880.0),
        (188743680, 5242880.0), (188743680, 2621440.0), (188743680, 2621440.0), (188743680, 1310720.0), (188743680, 1310720.0),
        (94371840.0, 1966080.0), (377487360, 3932160.0), (188743680, 2621440.0), (94371840.0, 3932160.0),
        (377487360, 7864320.0), (188743680, 5242880.0), (94371840.0, 7864320.0), (377487360, 15728640.0),
        (188743680, 10485760.0), (94371840.0, 15728640.0), (377487360, 31457280.0), (188743680, 20971520.0),
        (262144000, 15728640.0), (188743680, 10485760.0), (188743680, 10485760.0), (262144000, 7864320.0),
        (188743680, 5242880.0), (188743680, 5242880.0)]),
    (864, 1152): (18254315520.0, [
        (107495424, 27869184.0), (286654464, 23887872.0), (286654464, 11943936.0), (286654464, 5971968.0),
        (214990848, 43794432.0), (573308928, 63700992.0), (573308928, 31850496.0), (573308928, 31850496.0),
        (573308928, 15925248.0), (573308928, 15925248.0), (573308928, 7962624.0), (573308928, 7962624.0),
        (573308928, 3981312.0), (573308928, 3981312.0), (286654464.0, 5971968.0), (1146617856, 11943936.0),
        (573308928, 7962624.0), (286654464.0, 11943936.0), (1146617856, 23887872.0), (573308928, 15925248.0),
        (286654464.0, 23887872.0), (1146617856, 47775744.0), (573308928, 31850496.0), (286654464.0, 47775744.0),
        (1146617856, 95551488.0), (573308928, 63700992.0), (796262400, 47775744.0), (573308928, 31850496.0),
        (573308928, 31850496.0), (796262400, 23887872.0), (573308928, 15925248.0), (573308928, 15925248.0)]),
    (1200, 1600): (35212800000.0, [
        (207360000, 53760000.0), (552960000, 46080000.0), (552960000, 23040000.0), (552960000, 11520000.0),
        (414720000, 84480000.0), (1105920000, 122880000.0), (1105920000, 61440000.0), (1105920000, 61440000.0),
        (1105920000, 30720000.0), (1105920000, 30720000.0), (1105920000, 15360000.0), (1105920000, 15360000.0),
        (1105920000, 7680000.0), (1105920000, 7680000.0), (552960000.0, 11520000.0), (2211840000, 23040000.0),
        (1105920000, 15360000.0), (552960000.0, 23040000.0), (2211840000, 46080000.0), (1105920000, 30720000.0),
        (552960000.0, 46080000.0), (2211840000, 92160000.0), (1105920000, 61440000.0), (552960000.0, 92160000.0),
        (2211840000, 184320000.0), (1105920000, 122880000.0), (1536000000, 92160000.0), (1105920000, 61440000.0),
        (1105920000, 61440000.0), (1536000000, 46080000.0), (1105920000, 30720000.0), (1105920000, 30720000.0)]),
    (48, 80): (70425600.0, [
        (414720, 107520.0), (1105920, 92160.0), (1105920, 46080.0), (1105920, 23040.0), (829440, 168960.0),
        (2211840, 245760.0), (2211840, 122880.0), (2211840, 122880.0), (2211840, 61440.0), (2211840, 61440.0),
        (2211840, 30720.0), (2211840, 30720.0), (2211840, 15360.0), (2211840, 15360.0), (1105920.0, 23040.0),
        (4423680, 46080.0), (2211840, 30720.0), (1105920.0, 46080.0), (4423680, 92160.0), (2211840, 61440.0),
        (1105920.0, 92160.0), (4423680, 184320.0), (2211840, 122880.0), (1105920.0, 184320.0), (4423680, 368640.0),
        (2211840, 245760.0), (3072000, 184320.0), (2211840, 122880.0), (2211840, 122880.0), (3072000, 92160.0),
        (2211840, 61440.0), (2211840, 61440.0)]),
}


def normal_table():
    params = S.make_unet_params("normal", seed=3)
    return FN.tower_layers_of({name: np.asarray(p["w"]) for name, p in params.items()})


def test_the_table_of_the_normal_towers():
    layers = normal_table()
    assert [l[:5] for l in layers] == [(name, kind, srcs, k, stride) for name, kind, srcs, k, _mult, stride in FN.UNET_LAYERS]
    assert [(l.name, l.cin_tot, l.cout) for l in layers] == [row[:3] for row in TABLE]
    for col, (H, W) in ((3, (32, 48)), (4, (48, 80))):
        sizes = FN.layer_sizes(layers, H, W)
        assert [s_[2:] for s_ in sizes] == [row[col] for row in TABLE]
        by_name = dict(zip((l.name for l in layers), sizes), data=(0, 0, H, W))
        assert all(s_[:2] == by_name[l.srcs[0]][2:] and l.out_size(*s_[:2]) == s_[2:] for l, s_ in zip(layers, sizes))
    for l in layers:
        assert sum(l.cins) == l.cin_tot and len(l.cins) == len(l.srcs)
        assert l.relu == (1 if l.kind == "cg" else 0)
    assert layers[0].cins == (4,) and layers[15].cins == (64, 64)          # the padded image; 2dconv5_1 = 5_0 + 3_2


def test_the_routes_are_the_cases_of_the_gpu_file():
    layers = normal_table()
    pairs = lambda route: {(l.cin_tot, l.cout) for l in layers if l.gx_route == route}
    assert pairs(FN.GX_CONV_S1) == set(G.STRIDE1)
    assert pairs(FN.GX_DECONV) == set(G.STRIDE2)                      # a stride-2 convolution's: the transposed convolution
    assert pairs(FN.GX_CONV_S2) == set(G.TRANSPOSED)                  # a transposed convolution's: the stride-2 convolution
    assert {l.name for l in layers if l.gx_route == FN.GX_NONE} == {"2dconv1_0", "2dconv0_1"}
    assert {l.name for l in layers if l.gx_route == FN.GX_ATEN} == {"conv9_0", "conv10_0"}
    for l in layers:                                                   # the launch of a HIP route: Cout -> cin_tot channels, 3 x 3
        hip = l.gx_route in (FN.GX_CONV_S1, FN.GX_CONV_S2, FN.GX_DECONV)
        assert (l.gx is not None) == hip
        if hip:
            kind, stride = {FN.GX_CONV_S1: ("c", 1), FN.GX_CONV_S2: ("c", 2), FN.GX_DECONV: ("dg", 2)}[l.gx_route]
            assert (l.gx.kind, l.gx.k, l.gx.stride, l.gx.cins, l.gx.cout, l.gx.relu, l.gx.gx) == (kind, 3, stride, (l.cout,), l.cin_tot, 0, None)
            assert (l.kind == "dg") == (l.gx_route == FN.GX_CONV_S2) and (l.stride == 1) == (l.gx_route == FN.GX_CONV_S1)


@pytest.mark.parametrize("size", sorted(WORK))
def test_macs_and_layer_work_are_what_they_were(size):
    macs, rows = WORK[size]
    assert FN.unet_macs(*size) == macs
    assert FN.unet_layer_work(*size) == [(name, m, b) for (name, *_r), (m, b) in zip(FN.UNET_LAYERS, rows)]


def test_fork_join_layers_of_the_side_branches():
    from mvsnet_amd.feature_net_hip import fork_join_layers
    assert fork_join_layers(normal_table()) == FORK_JOIN


class _SizesOnly:
    """Stands in for the library where only its size queries are asked; `no_deconv_layout`: (c1, cout) pairs for which
    mvs_deconv2d_prepared_floats answers 0 -- a run-time fact of the library, not of the table."""

    def __init__(self, no_deconv_layout=()):
        self.no_deconv_layout = set(no_deconv_layout)

    def mvs_conv2d_prepared_floats(self, k, c1, c2, cout):
        return k * k * (c1 + c2) * cout

    def mvs_deconv2d_prepared_floats(self, c1, cout):
        return 0 if (c1, cout) in self.no_deconv_layout else 9 * c1 * cout


def test_prepare_jobs_follow_the_table_and_the_library_answer():
    """The rows of mvs_unet_prepare_many_f32's table, (kind, ks, c1, c2, cin_src, cout), for one layer of each route against
    literals; where the library has no prepared transposed-conv layout (0 floats) there is no job, forward or backward, and the
    launch gets the raw kernel alone."""
    from mvsnet_amd.feature_net_train import _prepare_job
    by_name = {l.name: l for l in normal_table()}
    w_of = lambda l: np.empty((3, 3, l.cout, l.cin_tot) if l.kind == "dg" else (l.k, l.k, 3 if l.srcs == ("data",) else l.cin_tot, l.cout))
    lib = _SizesOnly()

    def jobs(name, lib=lib):
        l = by_name[name]
        fwd = _prepare_job(lib, ("fwd", name), l, w_of(l))
        bwd = _prepare_job(lib, ("bwd", name), l.gx, w_of(l), l.gx_route == FN.GX_CONV_S1) if l.gx is not None else None
        return [j and j[1:2] + j[3:] for j in (fwd, bwd)]
    assert jobs("2dconv1_0") == [(0, 3, 4, 0, 3, 16, 9 * 4 * 16), None]                      # image-fed: 3 channels in the variable
    assert jobs("conv9_0") == [(0, 5, 8, 0, 8, 16, 25 * 8 * 16), None]                       # ATen route: nothing to prepare
    assert jobs("2dconv5_1") == [(0, 3, 64, 64, 128, 64, 9 * 128 * 64), (1, 3, 128, 0, 128, 64, 9 * 64 * 128)]
    assert jobs("2dconv2_0") == [(0, 3, 16, 0, 16, 32, 9 * 16 * 32), (2, 3, 32, 0, 32, 16, 9 * 32 * 16)]
    assert jobs("2dconv6_0") == [(2, 3, 64, 0, 64, 32, 9 * 64 * 32), (0, 3, 32, 0, 32, 64, 9 * 32 * 64)]
    none = _SizesOnly(no_deconv_layout={(64, 32), (32, 16)})
    assert jobs("2dconv6_0", none) == [None, (0, 3, 32, 0, 32, 64, 9 * 32 * 64)]             # forward transposed layer 64 -> 32
    assert jobs("2dconv2_0", none) == [(0, 3, 16, 0, 16, 32, 9 * 16 * 32), None]             # its gradient: transposed 32 -> 16


# kind, k, stride, Cin (of x), Cout, h, w, need_gx as the towers call the step, what the case is there for
ATEN_CASES = [
    ("cg", 5, 2, 8, 16, 12, 20, True, "asymmetric padding"),
    ("cg", 3, 2, 4, 16, 32, 48, False, "image-fed: pad, no crop"),
    ("cg", 3, 1, 4, 8, 6, 10, False, "image-fed: the 4 -> 3 channel cut of the returned gradient"),
    ("dg", 3, 2, 16, 8, 3, 5, False, "the padded gfull"),
    ("cg", 3, 1, 16, 16, 2, 3, False, "the shape-only weight tensor"),
]


@pytest.mark.parametrize("case", ATEN_CASES, ids=[c[-1] for c in ATEN_CASES])
def test_the_aten_step_on_cpu_tensors_matches_float64_autograd(case):
    """Weight gradients of every shape of the step, input gradients where the route is ATen, rtol = atol = 2e-4 (the bound the
    project holds these layers to; the formulas themselves sit at 6e-8 .. 5e-7 relative).  The image-fed rows hand the step the
    padded 4-channel input and a 3-channel kernel, as the towers do."""
    from mvsnet_amd.feature_net_train import aten_step, tf_weight_grad
    kind, k, stride, cin, cout, h, w, need_gx, _what = case
    V, image_fed = 2, cin == 4
    rs = np.random.RandomState(100 * k + 10 * stride + cin)
    x = rs.randn(V, h, w, cin).astype(np.float32)
    wk = (rs.randn(*((k, k, cout, cin) if kind == "dg" else (k, k, cin, cout))) / np.sqrt(k * k * cin)).astype(np.float32)
    d64 = lambda a_: torch.tensor(np.asarray(a_, np.float64)).requires_grad_(True)
    x64, w64 = d64(x), d64(wk)
    y64 = TG.deconv2d_same(x64, w64) if kind == "dg" else TG.conv2d_same(x64, w64, stride)
    g = rs.randn(*y64.shape).astype(np.float32)
    (y64 * torch.tensor(g, dtype=torch.float64)).sum().backward()
    w_tf = torch.as_tensor(wk[:, :, :3] if image_fed else wk)            # the variable: three input channels for the image
    g_w, g_x = aten_step(kind, k, stride, torch.as_tensor(x), torch.as_tensor(g), w_tf, need_gx)
    assert tuple(g_w.shape) == ((cin, cout, k, k) if kind == "dg" else (cout, cin, k, k))
    np.testing.assert_allclose(g_w.permute(2, 3, 1, 0).numpy(), w64.grad.numpy(), rtol=2e-4, atol=2e-4)
    returned = tf_weight_grad(g_w, image_fed)
    assert returned.is_contiguous() and tuple(returned.shape) == tuple(w_tf.shape)
    np.testing.assert_allclose(returned.numpy(), w64.grad.numpy()[:, :, :3] if image_fed else w64.grad.numpy(), rtol=2e-4, atol=2e-4)
    if need_gx:
        assert tuple(g_x.shape) == (V, cin, h, w)
        np.testing.assert_allclose(g_x.permute(0, 2, 3, 1).numpy(), x64.grad.numpy(), rtol=2e-4, atol=2e-4)
    else:
        assert g_x is None
