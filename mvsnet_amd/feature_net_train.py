"""UNetDS2GN towers for TRAINING as one autograd node (SURVEY 8f f2 + f4; mvsnet/cnn_wrapper/mvsnetworks.py:53-115,
the towers of `inference`, mvsnet/model.py:270-292, differentiated by TensorFlow in the reference).

Forward: exactly the inference extractor (`feature_net_hip.HipUNetDS2GN`): its `launch_layer` once per row of the layer table
(`feature_net.tower_layers`), the producer's GroupNorm (+ReLU) folded into the consumer's load; the raw layer outputs it keeps
anyway are what the backward needs.  (~0.7 ms for 3 x 480 x 640 against ~3.5 ms for the MIOpen convolutions + separate
GroupNorm passes.)

Backward, per layer in reverse, one function per step: GroupNorm(+ReLU) backward on the HIP library (`_gn_backward`); the
normalised input (`_normalised`); the input gradient by the route the table names -- on the forward HIP kernels through
`launch_layer` for the 3x3 layers (`_hip_input_gradient`: flipped kernel / conv <-> transposed conv with the same array) --
and ATen's `convolution_backward` (MIOpen) for the weight gradients and the two 5x5 stride-2 layers (`aten_step`, the
remaining PyTorch-ROCm glue in the towers); then the parameter gradients added into the trainer's flat buffer
(`_add_into_flat`) or returned to autograd (`_returned_grads`).
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple

import torch
import torch.nn.functional as F

from . import _lib
from .feature_net import GX_ATEN, GX_CONV_S1, UNET_VARIABLES, _same_pad, layer_sizes, tower_layers_of
from .feature_net_hip import Source, launch_layer

GN_EPS = 1e-5
_conv_bwd = torch.ops.aten.convolution_backward      # MIOpen's weight gradients (and the two 5x5 layers' input gradients)
_SHAPE_ONLY = {}          # (shape, device) -> uninitialised tensor handed to ATen where only the weight's shape matters


def _cl(t):
    """(V,H,W,C) contiguous -> the (V,C,H,W) channels_last view ATen wants (no copy)."""
    return t.permute(0, 3, 1, 2)


def flatten_unet_params(params) -> List[torch.Tensor]:
    return [params[name][key] for name, keys in UNET_VARIABLES for key in keys]


_WEIGHT_PLANS = {}        # (device, ((layer, address, shape), ...)) -> _WeightPlan
_SLABS = {}               # (views, H, W, slots, output channels per layer) -> _Slabs


class PrepareJob(NamedTuple):
    """One row of mvs_unet_prepare_many_f32's table."""
    key: tuple                # ("fwd" | "bwd", layer)
    kind: int                 # 0 forward layout, 1 input-gradient layout (mirrored, transposed), 2 transposed-conv layout
    w: torch.Tensor           # the kernel in the TensorFlow layout
    ks: int
    c1: int
    c2: int
    cin_src: int
    cout: int
    floats: int


def _prepare_job(lib, key, l, w, mirrored=False):
    """The preparation of `w` for the launch the record `l` describes (a layer, or a layer's `gx`); `mirrored`: the stride-1
    input gradient, whose preparation takes the FORWARD layer's channel counts.  None where the library has no prepared layout
    for a transposed convolution of these channels: the launch then gathers from the raw kernel."""
    # (c1, cin_src, cout) of the three input-gradient jobs, in the FORWARD layer's Cin (= cin_tot) and Cout:
    #   stride-1 conv, mirrored (kind 1): (Cin, Cin, Cout)   -- the forward layer's own counts; `floats` by the launch (Cout -> Cin)
    #   transposed layer -> stride-2 conv with the same array (3,3,Cout,Cin) (kind 0): (Cout, Cout, Cin)
    #   stride-2 conv -> transposed conv with the same array (3,3,Cin,Cout) (kind 2): (Cout, Cout, Cin)
    c1, c2 = l.cins[0], (l.cins[1] if len(l.cins) > 1 else 0)
    if l.kind == "dg":
        floats = lib.mvs_deconv2d_prepared_floats(c1, l.cout)
        return PrepareJob(key, 2, w, 3, c1, 0, c1, l.cout, floats) if floats else None
    floats = lib.mvs_conv2d_prepared_floats(l.k, c1, c2, l.cout)
    if mirrored:
        return PrepareJob(key, 1, w, 3, l.cout, 0, l.cout, c1, floats)
    return PrepareJob(key, 0, w, l.k, c1, c2, w.shape[2], l.cout, floats)


class _WeightPlan:
    """Every layer's kernel in the layouts the convolution kernels read -- for the forward pass AND for the input-gradient
    convolution of the backward pass -- laid out by ONE launch per step (`mvs_unet_prepare_many_f32`; ~60 launches before).
    Built once per set of variables (their addresses: the trainer's leaves are views of one flat buffer) and kept: the
    prepared copies live in one slab that every step overwrites in stream order, the job table is a handful of ctypes
    arrays.  (A forward pass whose backward has not run yet shares the slab with any later forward pass over the same
    variables: same values unless the variables were updated in between.)"""

    def __init__(self, weights, dev):
        lib = _lib.load()
        self.layers = tower_layers_of(weights)
        self.by_name = {l.name: l for l in self.layers}
        self.couts = tuple(l.cout for l in self.layers)
        jobs = []
        for l in self.layers:
            jobs.append(_prepare_job(lib, ("fwd", l.name), l, weights[l.name]))
            if l.gx is not None:                            # the input gradient on the forward kernels
                jobs.append(_prepare_job(lib, ("bwd", l.name), l.gx, weights[l.name], l.gx_route == GX_CONV_S1))
        jobs = [j for j in jobs if j is not None]
        self.slab = torch.empty(sum((j.floats + 63) // 64 * 64 for j in jobs), dtype=torch.float32, device=dev)
        self.prepared, off = {}, 0
        for j in jobs:
            self.prepared[j.key] = self.slab[off:off + j.floats]
            off += (j.floats + 63) // 64 * 64
        n = self.n = len(jobs)
        ints = lambda col: (C.c_int * n)(*[getattr(j, col) for j in jobs])
        self.args = (ints("kind"), (C.c_void_p * n)(*[j.w.data_ptr() for j in jobs]), ints("ks"), ints("c1"), ints("c2"),
                     ints("cin_src"), ints("cout"), (C.c_void_p * n)(*[self.prepared[j.key].data_ptr() for j in jobs]))
        self.keep = [j.w for j in jobs]                     # the addresses in the table stay valid

    def run(self, st):
        _lib.check(_lib.load().mvs_unet_prepare_many_f32(self.n, *self.args, st), "mvs_unet_prepare_many_f32")


def _weight_plan(weights, dev):
    key = (str(dev), tuple((n_, w.data_ptr(), tuple(w.shape)) for n_, w in weights.items()))
    plan = _WEIGHT_PLANS.get(key)
    if plan is None:
        if len(_WEIGHT_PLANS) > 8:                          # trainers come and go in tests: do not collect their slabs
            _WEIGHT_PLANS.clear()
        plan = _WEIGHT_PLANS[key] = _WeightPlan(weights, dev)
    return plan


class _Slabs(NamedTuple):
    """Where every GroupNorm layer's sums lie in the float64 slabs of one step, for one input shape."""
    sizes: list               # feature_net.layer_sizes
    slot_sums: dict           # layer -> slice of the slot sums the forward convolutions write; one zeroed slab
    slot_total: int
    to_channel_sums: tuple    # the job table of mvs_gn_slots_to_channel_sums_many_f64: n, slot offsets, C, channel-sum offsets
    chan_sums: dict           # layer -> (offset, C) of the per-channel (V, 2, C) sums of the raw output
    chan_total: int
    bwd_sums: dict            # layer -> offset of the backward's (slots, V, 2, C) gradient sums; one zeroed slab ...
    bwd_total: int
    totals: dict              # layer -> (offset, C) of their totals over the views, (2, C) = [d beta, d gamma], behind them
    totals_total: int


def _slabs(lib, plan, V, H, W, slots):
    key = (V, H, W, slots, plan.couts)
    s = _SLABS.get(key)
    if s is None:
        gn = [l for l in plan.layers if l.kind != "c"]
        slot_sums, chan_sums, bwd_sums, totals = {}, {}, {}, {}
        n_slot = n_chan = n_bwd = n_tot = 0
        for l in gn:
            slot_sums[l.name] = slice(n_slot, n_slot + V * (l.cout // 8) * 2 * slots)
            chan_sums[l.name], bwd_sums[l.name], totals[l.name] = (n_chan, l.cout), n_bwd, (n_tot, l.cout)
            n_slot = slot_sums[l.name].stop
            n_chan += V * 2 * l.cout
            n_bwd += lib.mvs_gn_bwd_sums_doubles(V, l.cout)
            n_tot += 2 * l.cout
        n = len(gn)
        table = (n, (C.c_longlong * n)(*[slot_sums[l.name].start for l in gn]), (C.c_int * n)(*[l.cout for l in gn]),
                 (C.c_longlong * n)(*[chan_sums[l.name][0] for l in gn]))
        s = _SLABS[key] = _Slabs(layer_sizes(plan.layers, H, W), slot_sums, n_slot, table, chan_sums, n_chan, bwd_sums, n_bwd,
                                 totals, n_tot)
    return s


class _Saved(NamedTuple):
    """What the forward pass leaves for the backward pass."""
    data: torch.Tensor        # the image padded 3 -> 4 channels
    acts: dict                # layer -> raw output
    P: dict                   # layer -> {'w', 'gamma', 'beta'} as the forward pass read them
    chan_stats: dict          # layer -> per-channel (V, 2, C) float64 sums of the raw output
    plan: _WeightPlan
    slabs: _Slabs


def _stage_images(lib, images, st):
    """(V,H,W,3) float32 (centred) or uint8 (decoded; standardised here) -> the padded (V,H,W,4) input of the first layers."""
    (V, H, W, _), dev = images.shape, images.device
    if images.dtype == torch.uint8:
        data = torch.empty((V, H, W, 4), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.mvs_center_images_workspace_bytes(V) // 8, dtype=torch.int64, device=dev)
        _lib.check(lib.mvs_center_images_u8_f32(_lib.ptr(images.contiguous()), V, H, W, _lib.ptr(data), _lib.ptr(ws), st),
                   "mvs_center_images_u8_f32")
    else:
        data = torch.zeros((V, H, W, 4), dtype=torch.float32, device=dev)
        data[..., :3] = images.detach()
    return data


def _forward_layers(lib, plan, P, data, slabs, st):
    """Every layer's raw output, and the zeroed slab their GroupNorm slot sums went to (one fill instead of 31)."""
    V, dev = data.shape[0], data.device
    so_slab = torch.zeros(slabs.slot_total, dtype=torch.float64, device=dev)
    acts, src_of = {}, {"data": Source(data)}
    for l, (h, w, ho, wo) in zip(plan.layers, slabs.sizes):
        name, p = l.name, P[l.name]
        y = acts[name] = torch.empty((V, ho, wo, l.cout), dtype=torch.float32, device=dev)
        so = so_slab[slabs.slot_sums[name]] if l.kind != "c" else None
        launch_layer(lib, l, [src_of[s_] for s_ in l.srcs], p["w"], plan.prepared.get(("fwd", name)), V, h, w, y, so, st)
        src_of[name] = Source(y, so, p.get("gamma"), p.get("beta"), l.relu)
    return acts, so_slab


def _channel_sums(lib, slabs, so_slab, V, slots, st):
    """Per-channel (V, 2, C) float64 sums of every raw output, from the slot sums the convolutions wrote (no second pass over
    the activations): all layers in one launch, for the backward's GroupNorm kernels."""
    n, slot_off_a, c_a, stat_off_a = slabs.to_channel_sums
    cs_slab = torch.empty(slabs.chan_total, dtype=torch.float64, device=so_slab.device)
    _lib.check(lib.mvs_gn_slots_to_channel_sums_many_f64(n, _lib.ptr(so_slab), slot_off_a, c_a, V, slots, _lib.ptr(cs_slab), stat_off_a, st),
               "mvs_gn_slots_to_channel_sums_many_f64")
    return {n_: cs_slab[o_:o_ + V * 2 * c_].view(V, 2, c_) for n_, (o_, c_) in slabs.chan_sums.items()}


def _gn_backward(lib, s, l, g_a, bs_slab, ps_slab, st):
    """GroupNorm(+ReLU) backward of layer `l`: the gradient `g_a` w.r.t. its normalised output -> the gradient w.r.t. its raw
    output; d beta / d gamma summed over the views land in the layer's place in `ps_slab`."""
    y, p = s.acts[l.name], s.P[l.name]
    V, ho, wo, cout = y.shape
    args = (_lib.ptr(y), _lib.ptr(s.chan_stats[l.name]), _lib.ptr(p["gamma"]), _lib.ptr(p["beta"]), GN_EPS, l.relu, _lib.ptr(g_a))
    sums = bs_slab[s.slabs.bwd_sums[l.name]:]                      # this layer's (slots, V, 2, C) start here
    o = s.slabs.totals[l.name][0]
    tot = ps_slab[o:o + 2 * cout]
    _lib.check(lib.mvs_gn_bwd_reduce_f32(*args, V, ho * wo, cout, _lib.ptr(sums), st), "mvs_gn_bwd_reduce_f32")
    g_y = torch.empty_like(y)
    _lib.check(lib.mvs_gn_bwd_apply_tot_f32(*args, _lib.ptr(sums), _lib.ptr(tot), V, ho * wo, cout, _lib.ptr(g_y), st),
               "mvs_gn_bwd_apply_tot_f32")
    return g_y


def _normalised(lib, s, name, cache, st):
    """What the consumers of `name` saw: GroupNorm(+ReLU) of the raw output (the padded image for 'data'); kept in `cache`."""
    if name == "data":
        return s.data
    if name not in cache:
        y, p = s.acts[name], s.P[name]
        V, h, w, c = y.shape
        out = cache[name] = torch.empty_like(y)
        _lib.check(lib.mvs_gn_apply_f32(_lib.ptr(y), _lib.ptr(s.chan_stats[name]), _lib.ptr(p["gamma"]), _lib.ptr(p["beta"]), GN_EPS,
                                        s.plan.by_name[name].relu, V, h * w, c, _lib.ptr(out), st), "mvs_gn_apply_f32")
    return cache[name]


def _hip_input_gradient(lib, l, g_y, x_shape, w_tf, prepared, st):
    """The input gradient of a 3 x 3 layer on the forward kernels, `l.gx` launched over the output gradient: a stride-1
    convolution's is the convolution with the flipped, transposed kernel, a stride-2 convolution's IS the transposed
    convolution with the same kernel array and vice versa (as for the 3D layers, backward.py)."""
    V, ho, wo, _ = g_y.shape
    gxt = torch.empty((V, x_shape[1], x_shape[2], l.cin_tot), dtype=torch.float32, device=g_y.device)
    launch_layer(lib, l.gx, [Source(g_y)], w_tf, prepared, V, ho, wo, gxt, None, st)
    return gxt


def aten_step(kind, k, stride, x, g_y, w_tf, need_gx):
    """ATen's convolution_backward of one layer (library-free: CPU tensors work too).  `x` (V,h,w,Cin) the normalised input,
    `g_y` (V,ho,wo,Cout) the gradient of the raw output, `w_tf` the kernel in the TensorFlow layout -- read only with
    `need_gx`, otherwise ATen needs the kernel's SHAPE, not its values.  -> (weight gradient in ATen's layout (Cout,Cin,k,k),
    transposed conv (Cin,Cout,k,k); input gradient (V,Cin,h,w) or None), with TensorFlow's SAME padding: symmetric, padded
    and cropped by hand where it is not, the full transposed output for 'dg'."""
    xin, gy = _cl(x), _cl(g_y)
    if need_gx:
        w_t = w_tf.permute(3, 2, 0, 1).contiguous()        # conv (Cout,Cin,k,k); transposed conv (Cin,Cout,k,k)
    else:
        shp = (w_tf.shape[3], x.shape[3] if kind != "dg" else w_tf.shape[2], w_tf.shape[0], w_tf.shape[1])
        w_t = _SHAPE_ONLY.get((shp, x.device))
        if w_t is None:
            w_t = _SHAPE_ONLY[(shp, x.device)] = torch.empty(shp, dtype=torch.float32, device=x.device)
    mask, s2 = [need_gx, True, False], [stride, stride]
    if kind == "dg":
        (n_h, n_w), (ho, wo) = x.shape[1:3], g_y.shape[1:3]
        pb_h, pb_w = _same_pad(n_h * stride, k, stride)[0], _same_pad(n_w * stride, k, stride)[0]
        full_h, full_w = stride * (n_h - 1) + k, stride * (n_w - 1) + k
        gfull = F.pad(gy, (pb_w, full_w - pb_w - wo, pb_h, full_h - pb_h - ho))
        g_x, g_w, _ = _conv_bwd(gfull, xin, w_t, None, s2, [0, 0], [1, 1], True, [0, 0], 1, mask)
    else:
        ph, pw = _same_pad(x.shape[1], k, stride), _same_pad(x.shape[2], k, stride)
        if ph[0] == ph[1] and pw[0] == pw[1]:
            g_x, g_w, _ = _conv_bwd(gy, xin, w_t, None, s2, [ph[0], pw[0]], [1, 1], False, [0, 0], 1, mask)
        else:
            xp = F.pad(xin, (pw[0], pw[1], ph[0], ph[1]))
            g_x, g_w, _ = _conv_bwd(gy, xp, w_t, None, s2, [0, 0], [1, 1], False, [0, 0], 1, mask)
            if need_gx:
                g_x = g_x[:, :, ph[0]:ph[0] + x.shape[1], pw[0]:pw[0] + x.shape[2]]
    return g_w, (g_x if need_gx else None)


def tf_weight_grad(g_w, image_fed):
    """ATen's weight gradient back in the TensorFlow layout; the image layers drop the padding channel (4 -> 3)."""
    g_wtf = g_w.permute(2, 3, 1, 0)
    return (g_wtf[:, :, :3] if image_fed else g_wtf).contiguous()


def _add_into_flat(lib, s, g_w, ps_slab, into, st):
    """The trainer's ending: all weight gradients (still in ATen's layout) transposed and added into their slices of the flat
    gradient buffer by one launch, all gamma / beta gradients (float64 totals) by a second."""
    into = dict(zip(((name, key) for name, keys in UNET_VARIABLES for key in keys), into))
    src, dst, dims = [], [], []
    for l in s.plan.layers:
        gw = g_w[l.name]                                      # (B, A, k, k) -> (k, k, A [:3 for the image], B)
        src.append(gw.data_ptr()); dst.append(into[l.name, "w"].data_ptr())
        dims += [gw.shape[0], gw.shape[1], l.k * l.k, 3 if l.srcs == ("data",) else gw.shape[1]]
    n = len(src)
    _lib.check(lib.mvs_transpose_add_many_f32(n, (C.c_void_p * n)(*src), (C.c_void_p * n)(*dst), (C.c_int * (4 * n))(*dims), st),
               "mvs_transpose_add_many_f32")
    src, dst, cnt = [], [], []
    base = ps_slab.data_ptr()
    for name, (o_, c_) in s.slabs.totals.items():             # [d beta (C), d gamma (C)] float64 per layer
        src += [base + 8 * (o_ + c_), base + 8 * o_]
        dst += [into[name, "gamma"].data_ptr(), into[name, "beta"].data_ptr()]
        cnt += [c_, c_]
    n = len(src)
    _lib.check(lib.mvs_add_f64_many_f32(n, (C.c_void_p * n)(*src), (C.c_void_p * n)(*dst), (C.c_int * n)(*cnt), st),
               "mvs_add_f64_many_f32")


def _returned_grads(s, g_w, ps_slab):
    """Autograd's ending: the gradients in the order of flatten_unet_params (weights already in the TensorFlow layout)."""
    ps32 = ps_slab.to(torch.float32)
    grads = {(name, "w"): g for name, g in g_w.items()}
    for name, (o_, c_) in s.slabs.totals.items():
        grads[name, "beta"], grads[name, "gamma"] = ps32[o_:o_ + c_], ps32[o_ + c_:o_ + 2 * c_]
    return tuple(grads[name, key] for name, keys in UNET_VARIABLES for key in keys)


class HipTowers(torch.autograd.Function):
    """images (V,H,W,3) float32 (centred) or uint8 (as decoded; standardised here) + the tower variables in TensorFlow layouts
    -> features (V,H/4,W/4,32)."""

    @staticmethod
    def forward(ctx, images, into, *flat):
        """`into`: None, or one tensor per entry of `flat` (the variables' slices of a flat gradient buffer): the backward then
        ACCUMULATES the parameter gradients there itself -- two launches for all 94 of them -- and hands autograd nothing
        (otherwise: a permute-copy per kernel and an accumulation launch per variable, ~190 launches)."""
        lib = _lib.load()
        V, H, W, _ = images.shape
        if H % 16 or W % 16:
            raise ValueError("UNetDS2GN needs image sizes divisible by 16")
        slots = lib.mvs_gn_stat_slots()
        st = _lib.stream_ptr()
        data = _stage_images(lib, images, st)
        it = iter(flat)
        P = {name: {key: next(it).detach().contiguous() for key in keys} for name, keys in UNET_VARIABLES}
        plan = _weight_plan({n_: P[n_]["w"] for n_ in P}, images.device)
        plan.run(st)                                                             # all forward + input-gradient layouts: one launch
        slabs = _slabs(lib, plan, V, H, W, slots)
        acts, so_slab = _forward_layers(lib, plan, P, data, slabs, st)
        ctx.into = into
        ctx.saved = _Saved(data, acts, P, _channel_sums(lib, slabs, so_slab, V, slots, st), plan, slabs)
        return acts["conv10_2"].clone()

    @staticmethod
    def backward(ctx, g_feat):
        lib = _lib.load()
        s, into = ctx.saved, ctx.into
        st = _lib.stream_ptr()
        zero_slab = torch.zeros(s.slabs.bwd_total + s.slabs.totals_total, dtype=torch.float64, device=s.data.device)
        bs_slab, ps_slab = zero_slab[:s.slabs.bwd_total], zero_slab[s.slabs.bwd_total:]
        norm_cache, g_act, g_w = {}, {}, {}              # g_act: gradient w.r.t. a layer's normalised output, summed over its consumers
        for l in reversed(s.plan.layers):
            name, w_tf = l.name, s.P[l.name]["w"]
            g_y = g_feat.contiguous() if l.kind == "c" else _gn_backward(lib, s, l, g_act.pop(name).contiguous(), bs_slab, ps_slab, st)
            # convolution backward on the materialised normalised inputs: weight gradient through ATen / MIOpen, input
            # gradient by the layer's route
            xs = [_normalised(lib, s, s_, norm_cache, st) for s_ in l.srcs]
            x = xs[0] if len(xs) == 1 else torch.cat(xs, dim=3)
            g_x = None
            if l.gx is not None:
                g_x = _cl(_hip_input_gradient(lib, l, g_y, x.shape, w_tf, s.plan.prepared.get(("bwd", name)), st))
            gw, gx_aten = aten_step(l.kind, l.k, l.stride, x, g_y, w_tf, l.gx_route == GX_ATEN)
            g_w[name] = gw.contiguous() if into is not None else tf_weight_grad(gw, l.srcs == ("data",))
            if gx_aten is not None:
                g_x = gx_aten
            if g_x is not None:
                g_x = g_x.permute(0, 2, 3, 1)                         # (V,H,W,Cin) view
                c0 = 0
                for s_, c in zip(l.srcs, l.cins):
                    g = g_x[..., c0:c0 + c]
                    g_act[s_] = g if s_ not in g_act else g_act[s_] + g
                    c0 += c
        ctx.saved = None
        if into is None:
            return (None, None) + _returned_grads(s, g_w, ps_slab)
        _add_into_flat(lib, s, g_w, ps_slab, into, st)
        return (None, None) + (None,) * len(into)


def hip_towers(images, params, accumulate_into_grads=False):
    """images (V,H,W,3) device tensor, params[name] = {'w','gamma','beta'} leaves in TF layouts -> (V,H/4,W/4,32).
    `accumulate_into_grads`: the leaves carry pre-allocated contiguous `.grad` tensors (train.FlatParameters: views of one flat
    buffer) and the backward adds the parameter gradients into them itself (see HipTowers.forward); autograd then sees no
    gradient for them -- for callers that read `.grad` afterwards, not for torch.autograd.grad."""
    flat = flatten_unet_params(params)
    into = None
    if accumulate_into_grads:
        into = [p.grad for p in flat]
        if any(g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.device != images.device or g.shape != p.shape
               for g, p in zip(into, flat)):
            raise ValueError("accumulate_into_grads needs a contiguous float32 .grad of the variable's shape on every leaf")
    return HipTowers.apply(images, into, *flat)
