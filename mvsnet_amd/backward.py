"""Training-time forward and backward of the plane-sweep hot path on the HIP library.

The reference trains through `inference` (mvsnet/model.py:257-372: towers -> eager variance cost volume
-> RegNetUS0 -> soft-argmin) and lets TensorFlow differentiate the graph (`opt.compute_gradients`,
mvsnet/train.py:428-429).  Here the hot path is one `torch.autograd.Function` whose forward and backward
are sequences of C-ABI calls: torch owns memory, the 2D towers (`feature_net.UNetDS2GN`, differentiated by
torch autograd, as north_star keeps them on PyTorch-ROCm) and the loss expressions (`loss.py`).

Layer bookkeeping of RegNetUS0 (mvsnetworks.py:122-158): `regnet_layers.REGNET_LAYERS` is the network as data -- kind,
channels, producers, BatchNorm -- and both passes are loops over it.  Forward (`regnet_forward_train`, table order; the cost
volume's two readers in one `conv3d_pair` where that kernel is built): every BatchNorm layer keeps its RAW output y, its
float64 batch sums and the folded affine; consumers apply BN+ReLU on load exactly as in inference.  Backward
(`regnet_backward`, REGNET_BACKWARD_ORDER: consumers first) per layer:  the one or two gradients its consumers filed for its
post-ReLU activation -> BN+ReLU backward (two HBM passes) -> g_y -> the input activation (BN+ReLU of the producers, recomputed
once per producer set and dropped behind its last reader) -> weight gradient (MFMA contraction over voxels) -> input gradient
(INPUT_GRAD by kind, on the forward MFMA kernels: conv stride 2 <-> conv_transpose with the same kernel array, stride 1 with
the flipped / transposed kernel), filed under the producers.  The variables' flat order is REGNET_SLOTS, for parameters and
gradients alike.  tests/test_regnet_table_host.py runs both loops on CPU float64 stand-ins of the single-op wrappers.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from . import _lib
from .model import BN_EPSILON, bn_finalize, conv3d, conv3d_pair, cost_volume
from .regnet_layers import (BN_LAYERS, REGNET_BACKWARD_ORDER, REGNET_CONSUMERS, REGNET_LAYER, REGNET_LAYERS, REGNET_ORDER, REGNET_PAIR,
                            REGNET_SLOTS, S1, S2, UP)


# ------------------------------------------------------------------------------------------------
# single-op wrappers
# ------------------------------------------------------------------------------------------------

def softargmin_bwd(reg, g_depth, depth_start, depth_interval, inverse_depth=False, g_prob=None):
    """reg (D,H,W), g_depth (H,W) [, g_prob (H,W)] -> g_reg (D,H,W)   (model.py:343-366, 45-144)"""
    lib = _lib.load()
    D, H, W = reg.shape
    g = torch.empty_like(reg)
    gd = _lib.f32(g_depth.contiguous()) if g_depth is not None else None
    gp = _lib.f32(g_prob.contiguous()) if g_prob is not None else None
    _lib.check(lib.mvs_softargmin_bwd_f32(_lib.ptr(reg), _lib.ptr(gd), _lib.ptr(gp), D, H, W,
                                          float(depth_start), float(depth_interval), int(bool(inverse_depth)),
                                          _lib.ptr(g), _lib.stream_ptr()), "mvs_softargmin_bwd_f32")
    return g


def bn_relu(y, affine=None, y2=None, affine2=None):
    """act(y*s+t) [+ act(y2*s2+t2)]: the normalised input a consumer layer sees."""
    lib = _lib.load()
    s, t = affine if affine is not None else (None, None)
    s2, t2 = affine2 if affine2 is not None else (None, None)
    out = torch.empty_like(y)
    Cn = y.shape[-1]
    _lib.check(lib.mvs_bn_relu_f32(_lib.ptr(y), _lib.ptr(s), _lib.ptr(t), _lib.ptr(y2), _lib.ptr(s2), _lib.ptr(t2),
                                   y.numel() // Cn, Cn, _lib.ptr(out), _lib.stream_ptr()), "mvs_bn_relu_f32")
    return out


class SyncBN:
    """Cross-replica BatchNorm for data-parallel training (SURVEY 8f f4 lists it as an addition; the reference's
    towers keep per-GPU statistics): the float64 per-channel sums of every BatchNorm layer -- forward [sum, sumsq],
    backward [sum gz, sum gz*xhat] -- are summed over the ranks and the voxel count is multiplied by the world size,
    exactly as if the replicas' volumes were one batch.  Per-variable gradients stay local (the flat-buffer
    all-reduce averages them afterwards).  RCCL reduces the tiny buffers in place; under gloo (CPU tests) they are
    staged through host memory."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist, self.group = dist, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.direct = dist.is_initialized() and dist.get_backend(group) == "nccl"

    def all_reduce(self, t):
        if self.world == 1:
            return t
        if self.direct:
            self.dist.all_reduce(t, group=self.group)
        else:
            h = t.cpu()
            self.dist.all_reduce(h, group=self.group)
            t.copy_(h)
        return t


def bn_relu_bwd(y, stats, affine, gamma, g1, g2=None, eps=BN_EPSILON, sync: Optional[SyncBN] = None, sums=None):
    """BatchNorm(batch statistics)+ReLU backward (network.py:492-509).  Returns (g_y, g_gamma, g_beta).
    `stats` are the sums the forward normalised with (global ones under `sync`).  `sums`: a ZEROED float64 buffer of
    mvs_bn_bwd_sum_slots() * 2 * C entries to use (regnet_backward hands out pieces of one slab: one fill for all layers)."""
    lib = _lib.load()
    Cn = y.shape[-1]
    vox = y.numel() // Cn
    world = sync.world if sync is not None else 1
    if sums is None:
        sums = torch.zeros((lib.mvs_bn_bwd_sum_slots(), 2, Cn), device=y.device, dtype=torch.float64)
    else:
        sums = sums.view(lib.mvs_bn_bwd_sum_slots(), 2, Cn)
    s, t = affine
    _lib.check(lib.mvs_bn_bwd_reduce_f32(_lib.ptr(y), _lib.ptr(stats), float(vox * world), float(eps), _lib.ptr(s), _lib.ptr(t),
                                         _lib.ptr(g1), _lib.ptr(g2), vox, Cn, _lib.ptr(sums), _lib.stream_ptr()),
               "mvs_bn_bwd_reduce_f32")
    g_y = torch.empty_like(y)
    g_gamma = torch.empty(Cn, device=y.device, dtype=torch.float32)
    g_beta = torch.empty_like(g_gamma)
    local = None
    if world > 1:                                      # the variables' gradients are this replica's own sums
        local = sums.sum(0).to(torch.float32)
        sync.all_reduce(sums)
    _lib.check(lib.mvs_bn_bwd_apply_f32(_lib.ptr(y), _lib.ptr(stats), float(vox * world), float(eps), _lib.ptr(s), _lib.ptr(t),
                                        _lib.ptr(gamma), _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(sums), vox, Cn,
                                        _lib.ptr(g_y), _lib.ptr(g_gamma), _lib.ptr(g_beta), _lib.stream_ptr()),
               "mvs_bn_bwd_apply_f32")
    if local is not None:
        g_gamma, g_beta = local[1].contiguous(), local[0].contiguous()
    return g_y, g_gamma, g_beta


_WS: Dict[torch.device, torch.Tensor] = {}


def conv3d_wgrad(big, small, stride):
    """dW(3,3,3,Cbig,Csmall) = sum_o big(stride*o + tap - pad) (x) small(o); see include/mvsnet_hip.h."""
    lib = _lib.load()
    D, H, W, Cb = big.shape
    Cs = small.shape[-1]
    need = lib.mvs_conv3d_wgrad_workspace_bytes(D, H, W, Cb, Cs, stride)
    if need == 0:
        raise _lib.MvsnetHipError("weight gradient not built for %d x %d channels, stride %d" % (Cb, Cs, stride))
    ws = _WS.get(big.device)
    if ws is None or ws.numel() < need:
        ws = _WS[big.device] = torch.empty(need, device=big.device, dtype=torch.uint8)
    dw = torch.empty((3, 3, 3, Cb, Cs), device=big.device, dtype=torch.float32)
    _lib.check(lib.mvs_conv3d_wgrad_f32(_lib.ptr(big), _lib.ptr(small), D, H, W, Cb, Cs, stride,
                                        C.c_void_p(ws.data_ptr()), ws.numel(), _lib.ptr(dw), _lib.stream_ptr()),
               "mvs_conv3d_wgrad_f32")
    return dw


_CVWS: Dict[torch.device, torch.Tensor] = {}


def cost_volume_bwd(ref, src, transforms, g1, g2=None, method="gather"):
    """Gradient of the warp + variance w.r.t. the feature maps: (g_ref (H,W,C), g_src (N-1,H,W,C)).
    method "gather": atomic-free two-pass kernels (bit-reproducible, C = 32 / 16); "scatter": float atomics."""
    lib = _lib.load()
    H, W, Cc = ref.shape
    n_src, D = transforms.shape[0], transforms.shape[1]
    need = lib.mvs_cost_volume_bwd_workspace_bytes(n_src + 1, D, H, W, Cc) if method == "gather" else 0
    if need:
        ws = _CVWS.get(ref.device)
        if ws is None or ws.numel() < need:
            ws = _CVWS[ref.device] = torch.empty(need, device=ref.device, dtype=torch.uint8)
        g_ref, g_src = torch.empty_like(ref), torch.empty_like(src)
        _lib.check(lib.mvs_cost_volume_bwd_gather_f32(
            _lib.ptr(ref), _lib.ptr(src), _lib.ptr(transforms), n_src + 1, D, H, W, Cc, _lib.ptr(g1), _lib.ptr(g2),
            C.c_void_p(ws.data_ptr()), ws.numel(), _lib.ptr(g_ref), _lib.ptr(g_src), _lib.stream_ptr()),
            "mvs_cost_volume_bwd_gather_f32")
        return g_ref, g_src
    g_ref = torch.zeros_like(ref)
    g_src = torch.zeros_like(src)
    _lib.check(lib.mvs_cost_volume_bwd_f32(_lib.ptr(ref), _lib.ptr(src), _lib.ptr(transforms), n_src + 1, D, H, W, Cc,
                                           _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(g_ref), _lib.ptr(g_src),
                                           _lib.stream_ptr()), "mvs_cost_volume_bwd_f32")
    return g_ref, g_src


def _pad_channels(x, w, axis, to=16):
    """The MFMA convolutions tile Cin in 16s: zero-pad an 8-channel gradient (and the kernel's Cin axis)."""
    cin = x.shape[-1]
    if cin >= to:
        return x, w
    xp = torch.zeros(x.shape[:-1] + (to,), device=x.device, dtype=x.dtype)
    xp[..., :cin] = x
    shp = list(w.shape); shp[axis] = to
    wp = torch.zeros(shp, device=w.device, dtype=w.dtype)
    wp.narrow(axis, 0, cin).copy_(w)
    return xp, wp


def conv_s1_input_grad(g_y, w):
    """Input gradient of y = conv3d(x, w (3,3,3,Cin,Cout), stride 1): conv3d(g_y, flip(w)^T)."""
    wt = w.flip(0, 1, 2).permute(0, 1, 2, 4, 3).contiguous()          # (3,3,3,Cout,Cin) read as Cin'=Cout, Cout'=Cin
    if g_y.shape[-1] == 8 and wt.shape[4] != 32:          # 8 -> 32 has its own kernel (conv3d_k8.hip: taps paired along w)
        g_y, wt = _pad_channels(g_y, wt, 3)
    return conv3d(g_y, wt, 1)


def conv_s2_input_grad(g_y, w):
    """Input gradient of a stride-2 SAME convolution = conv3d_transpose with the same kernel array."""
    return conv3d(g_y, w, transpose=True)


def deconv_input_grad(g_y, w):
    """Input gradient of conv3d_transpose (w (3,3,3,Cout,Cin)) = stride-2 convolution with the same array."""
    if g_y.shape[-1] == 8:
        g_y, w = _pad_channels(g_y, w, 3)
    return conv3d(g_y, w, 2)


# ------------------------------------------------------------------------------------------------
# RegNetUS0 with saved activations
# ------------------------------------------------------------------------------------------------

# a layer's input gradient from the gradient of its raw output and its own kernel array, by the layer's kind
INPUT_GRAD = {S1: conv_s1_input_grad, S2: conv_s2_input_grad, UP: deconv_input_grad}
# how many layers read the same input activation: it is recomputed once and dropped behind the last of them
_READERS = {srcs: sum(l.srcs == srcs for l in REGNET_LAYERS) for srcs in {l.srcs for l in REGNET_LAYERS}}


def _pieces(slab):
    """Hands out consecutive pieces of one zeroed slab: one fill for all layers' sums instead of one each."""
    used = [0]

    def take(n):
        used[0] += n
        return slab[used[0] - n:used[0]]
    return take


def _pair_fuses(cost, p):
    """Whether mvs_conv3d_pair_f32 is built for this volume: both of its readers in one pass over it."""
    base = REGNET_LAYER[REGNET_PAIR[0]].cout_of(p[REGNET_PAIR[0]]["w"])
    return cost.shape[3] == 32 and base == 8 and not (cost.shape[0] | cost.shape[1] | cost.shape[2]) & 1


def regnet_forward_train(cost, p: Dict[str, Dict[str, torch.Tensor]], sync: Optional[SyncBN] = None):
    """cost (D,H,W,32); p[name] = {'w', 'gamma', 'beta'}.  Returns (reg (D,H,W), saved).  `sync`: cross-replica
    BatchNorm statistics (SyncBN)."""
    y, st, aff = {}, {}, {}
    world = sync.world if sync is not None else 1
    couts = {l.name: l.cout_of(p[l.name]["w"]) for l in REGNET_LAYERS}
    # every layer's (2, Cout) float64 BatchNorm sums from ONE zeroed slab
    take = _pieces(torch.zeros(sum(2 * couts[n] for n in BN_LAYERS), device=cost.device, dtype=torch.float64))
    stats = lambda name: take(2 * couts[name]).view(2, couts[name])

    def batch_norm(name, out, s):
        if world > 1:
            sync.all_reduce(s)
        y[name], st[name] = out, s
        aff[name] = bn_finalize(s, (out.numel() // couts[name]) * world, p[name]["gamma"], p[name]["beta"])

    fused = _pair_fuses(cost, p)
    for l in REGNET_LAYERS:
        if l.name in y:                                    # 3dconv0_1 came out of the fused pass
            continue
        if fused and l.name in REGNET_PAIR:
            s_pair = [stats(n) for n in REGNET_PAIR]
            outs = conv3d_pair(cost, *(p[n]["w"] for n in REGNET_PAIR), *s_pair)
            for n, out, s in zip(REGNET_PAIR, outs, s_pair):
                batch_norm(n, out, s)
            continue
        s = stats(l.name) if l.bn else None
        out = conv3d(y.get(l.p1, cost), p[l.name]["w"], l.stride, aff.get(l.p1), y.get(l.p2), aff.get(l.p2), s, l.kind == UP)
        if l.bn:
            batch_norm(l.name, out, s)
    return out[..., 0], (cost, y, st, aff, sync)


def regnet_backward(saved, p, g_reg):
    """g_reg (D,H,W) -> (grads {name: {'w','gamma','beta'}}, g_cost_a, g_cost_b): the cost volume has two
    consumers (3dconv0_1, 3dconv1_0); their input gradients are returned separately and summed on load by
    the cost-volume backward."""
    cost, y, st, aff, sync = saved
    G: Dict[str, Dict[str, torch.Tensor]] = {}
    nsl = _lib.load().mvs_bn_bwd_sum_slots()
    take = _pieces(torch.zeros(nsl * sum(2 * y[n].shape[-1] for n in st), device=g_reg.device, dtype=torch.float64))
    pending = {(None, REGNET_ORDER[-1]): g_reg.contiguous()[..., None]}      # (consumer, producer) -> gradient of a(producer)
    acts, readers = {(): cost}, dict(_READERS)             # producers -> the activation their consumers read, while it has readers

    def input_act(l):
        if l.srcs not in acts:
            acts[l.srcs] = bn_relu(*(t for n in l.srcs for t in (y[n], aff[n])))
        readers[l.srcs] -= 1
        return acts[l.srcs] if readers[l.srcs] else acts.pop(l.srcs)

    def layer_backward(l):
        name, w = l.name, p[l.name]["w"]
        # a shared activation is recomputed ahead of its first reader's BatchNorm backward, any other behind it: the order of
        # launches this pass has always had
        x = input_act(l) if _READERS[l.srcs] > 1 or not l.bn else None
        g_y = [pending.pop((c, name)) for c in REGNET_CONSUMERS[name] or (None,)]
        if l.bn:
            g_y, gg, gb = bn_relu_bwd(y[name], st[name], aff[name], p[name]["gamma"], *g_y, sync=sync,
                                      sums=take(nsl * 2 * y[name].shape[-1]))
            G[name] = {"gamma": gg, "beta": gb}
        else:
            g_y, = g_y
            G[name] = {}
        if x is None:
            x = input_act(l)
        dw = conv3d_wgrad(*((g_y, x) if l.wgrad_gradient_first else (x, g_y)), l.stride)
        if l.wgrad_mirrored:
            # roles swapped (rows = the 8-channel gradient with its taps, columns = the 32 volume channels): the kernel packs 8
            # taps per MFMA row tile; R(tap, c8, c32) = dW(2 - tap, c32, c8)
            dw = dw.flip(0, 1, 2).permute(0, 1, 2, 4, 3).contiguous()
        G[name]["w"] = dw
        del x
        g_x = INPUT_GRAD[l.kind](g_y, w)
        for src in l.srcs or (None,):
            pending[(name, src)] = g_x

    for name in REGNET_BACKWARD_ORDER:
        layer_backward(REGNET_LAYER[name])
    return (G,) + tuple(pending.pop((n, None)) for n in REGNET_PAIR)


# ------------------------------------------------------------------------------------------------
# autograd seam
# ------------------------------------------------------------------------------------------------

def flatten_params(p) -> List[torch.Tensor]:
    return [p[n][key] for n, key in REGNET_SLOTS]


def unflatten_params(flat) -> Dict[str, Dict[str, torch.Tensor]]:
    p = {n: {} for n in REGNET_ORDER}
    for (n, key), t in zip(REGNET_SLOTS, flat):
        p[n][key] = t
    return p


class PlaneSweepDepth(torch.autograd.Function):
    """features (N,H,W,C) [view 0 = reference], transforms (N-1,D,8) -> depth map (H,W); differentiable
    w.r.t. the features and the RegNetUS0 parameters (cameras are data).  The probability map carries a gradient too
    (it is an input channel of the refinement network, model.py:753-811); its bucket indices do not."""

    @staticmethod
    def forward(ctx, features, transforms, depth_start, depth_interval, inverse_depth, sync, into, *flat):
        """`into`: None, or one tensor per entry of `flat` (the variables' slices of a flat gradient buffer): the backward then adds
        the parameter gradients there itself -- one launch for all of them (mvs_add_many_f32) -- and hands autograd nothing."""
        from .model import softargmin_prob
        ctx.into = into
        p = unflatten_params([t.detach() for t in flat])
        features = features.detach().contiguous()
        cost = cost_volume(features[0], features[1:], transforms, variant="eager")      # model.py:330-332
        reg, saved = regnet_forward_train(cost, p, sync)
        depth, prob = softargmin_prob(reg, depth_start, depth_interval, inverse_depth)
        ctx.saved = (features, transforms, reg, saved, p)
        ctx.scalars = (float(depth_start), float(depth_interval), bool(inverse_depth))
        return depth, prob

    @staticmethod
    def backward(ctx, g_depth, g_prob):
        features, transforms, reg, saved, p = ctx.saved
        start, interval, inverse = ctx.scalars
        g_reg = softargmin_bwd(reg, g_depth, start, interval, inverse, g_prob)
        G, ga, gb = regnet_backward(saved, p, g_reg)
        g_ref, g_src = cost_volume_bwd(features[0], features[1:], transforms, ga, gb)
        g_feat = torch.cat([g_ref[None], g_src], 0)
        flat = flatten_params(G)
        ctx.saved = None
        if ctx.into is not None:
            import ctypes as C
            flat = [g.contiguous() for g in flat]
            n = len(flat)
            _lib.check(_lib.load().mvs_add_many_f32(n, (C.c_void_p * n)(*[g.data_ptr() for g in flat]),
                                                    (C.c_void_p * n)(*[t.data_ptr() for t in ctx.into]),
                                                    (C.c_longlong * n)(*[g.numel() for g in flat]), _lib.stream_ptr()), "mvs_add_many_f32")
            return (g_feat, None, None, None, None, None, None) + (None,) * n
        return (g_feat, None, None, None, None, None, None) + tuple(flat)


def plane_sweep_depth(features, transforms, depth_start, depth_interval, params, inverse_depth=False, sync=None,
                      accumulate_into_grads=False):
    """`sync`: a SyncBN for cross-replica BatchNorm statistics under torch.distributed (default: per-replica).
    `accumulate_into_grads`: the leaves carry pre-allocated contiguous `.grad` tensors (train.FlatParameters) and the backward adds
    the parameter gradients into them itself, in one launch; autograd then sees no gradient for them."""
    flat = flatten_params(params)
    into = None
    if accumulate_into_grads:
        into = [p.grad for p in flat]
        if any(g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.shape != p.shape for g, p in zip(into, flat)):
            raise ValueError("accumulate_into_grads needs a contiguous float32 .grad of the variable's shape on every leaf")
    return PlaneSweepDepth.apply(features, transforms, depth_start, depth_interval, inverse_depth, sync, into, *flat)
