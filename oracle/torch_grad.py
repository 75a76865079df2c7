"""Gradient checker for the training path: the features -> depth composition of
mvsnet/model.py:257-372 (`inference`: eager variance :315-334, RegNetUS0 mvsnetworks.py:122-158 with
batch-statistics BatchNorm network.py:492-509, soft-argmin model.py:343-366) written with differentiable
torch-CPU float64 ops, so that torch autograd plays the role TensorFlow's autodiff has in the reference
(train.py:428-429); further down the recurrent regulariser with its classification loss, the UNetDS2GN towers and the
regression loss (loss.py:31-92, 134-220), which tests/train_reference.py composes into whole training steps.
TEST INFRASTRUCTURE ONLY: never imported by ``mvsnet_amd``.  Parity unpinned by the
reference (no tests / fixtures there; see mvsnet_oracle.py header); the forward value of this file is
checked against the strict numpy restatement in tests/test_cpu_restatement.py.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import mvsnet_oracle as O


def warp_all_planes(src, t8):
    """src (C,H,W), t8 (D,8) -> (D,C,H,W); tf.contrib.image.transform BILINEAR with zero fill per tap
    (homography_warping.py:251-252) == grid_sample(bilinear, zeros, align_corners=True)."""
    C, H, W = src.shape
    D = t8.shape[0]
    dt = src.dtype
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    t = t8.view(D, 8, 1, 1)
    proj = t[:, 6] * xs + t[:, 7] * ys + 1.0
    sx = (t[:, 0] * xs + t[:, 1] * ys + t[:, 2]) / proj
    sy = (t[:, 3] * xs + t[:, 4] * ys + t[:, 5]) / proj
    grid = torch.stack([sx * (2.0 / max(W - 1, 1)) - 1.0, sy * (2.0 / max(H - 1, 1)) - 1.0], dim=-1)
    return F.grid_sample(src[None].expand(D, C, H, W), grid, mode="bilinear", padding_mode="zeros",
                         align_corners=True)


def cost_volume(features, t8):
    """features (N,H,W,C) tensor, t8 (N-1,D,8) tensor -> (C,D,H,W): cost = Q/N - (S/N)^2 (model.py:330-332)."""
    f = features.permute(0, 3, 1, 2)
    n = float(f.shape[0])
    S, Q = f[0][None], (f[0] * f[0])[None]
    for v in range(1, f.shape[0]):
        w = warp_all_planes(f[v], t8[v - 1])
        S = S + w
        Q = Q + w * w
    return (Q / n - (S / n) ** 2).permute(1, 0, 2, 3)


def _pad_same(x, stride):
    pads = []
    for n in reversed(x.shape[-3:]):
        _, pb, pa = O.same_pad(int(n), 3, stride)
        pads += [pb, pa]
    return F.pad(x, pads)


def _conv(x, w, stride):
    return F.conv3d(_pad_same(x, stride), w.permute(4, 3, 0, 1, 2), stride=stride)


def _deconv(x, w):
    y = F.conv_transpose3d(x, w.permute(4, 3, 0, 1, 2), stride=2)
    D, H, W = x.shape[-3:]
    return y[..., : 2 * D, : 2 * H, : 2 * W]


def _bn_relu(x, p, eps=1e-5):
    return F.relu(F.batch_norm(x, None, None, p["gamma"], p["beta"], training=True, eps=eps))


def regnet_us0(cost, p, bn_relu=None):
    """cost (C,D,H,W) -> (D,H,W), or a batch (B,C,D,H,W) -> (B,D,H,W) whose BatchNorm statistics run over the whole
    batch (what cross-replica BatchNorm computes with one sample per replica); p[name] = {'w','gamma','beta'} tensors
    in the TensorFlow layouts.  `bn_relu(name, x, p[name])`: what normalises and rectifies layer `name` (default: _bn_relu;
    tests/train_reference.py records the pre-activations through it)."""
    batched = cost.dim() == 5
    x = cost if batched else cost[None]
    act = bn_relu or (lambda _n, t, q: _bn_relu(t, q))
    cb = lambda t, n, s: act(n, _conv(t, p[n]["w"], s), p[n])
    db = lambda t, n: act(n, _deconv(t, p[n]["w"]), p[n])
    c1_0 = cb(x, "3dconv1_0", 2); c2_0 = cb(c1_0, "3dconv2_0", 2); c3_0 = cb(c2_0, "3dconv3_0", 2)
    c0_1 = cb(x, "3dconv0_1", 1); c1_1 = cb(c1_0, "3dconv1_1", 1); c2_1 = cb(c2_0, "3dconv2_1", 1)
    c3_1 = cb(c3_0, "3dconv3_1", 1)
    c4 = db(c3_1, "3dconv4_0") + c2_1
    c5 = db(c4, "3dconv5_0") + c1_1
    c6 = db(c5, "3dconv6_0") + c0_1
    out = _conv(c6, p["3dconv6_2"]["w"], 1)[:, 0]
    return out if batched else out[0]


def soft_argmin(reg, depth_start, depth_interval):
    D = reg.shape[0]
    P = torch.softmax(-reg, dim=0)
    z = torch.from_numpy(O.depth_values(D, depth_start, depth_interval, False, np.float64)).to(reg.dtype)
    return (P * z[:, None, None]).sum(0)


def depth_from_features(features, t8, depth_start, depth_interval, p, bn_relu=None):
    """features (N,H,W,C), t8 (N-1,D,8) -> depth (H,W), differentiable in features and p."""
    return soft_argmin(regnet_us0(cost_volume(features, t8), p, bn_relu), depth_start, depth_interval)


# ---- recurrent regulariser (model.py:505-599) and classification loss (loss.py:223-267) ------------------------

def _conv2d_same(x, w, b):
    """x (1,C,H,W), w TF layout (3,3,Cin,Cout): tf.layers.conv2d(padding='same')."""
    return F.conv2d(x, w.permute(3, 2, 0, 1), b, padding=1)


def _layer_norm(x, gamma, beta, eps=1e-12):
    """tf.contrib.layers.layer_norm on one sample (convgru.py:30-31): moments over (C,H,W)."""
    mean = x.mean()
    var = ((x - mean) ** 2).mean()
    return (x - mean) / torch.sqrt(var + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


def conv_gru_cell(x, h, p):
    """ConvGRUCell.__call__ (convgru.py:82-122) in its own shape: concatenate, convolve, split."""
    Fn = h.shape[1]
    g = _conv2d_same(torch.cat([x, h], 1), p["gates_w"], p["gates_b"])
    r = torch.sigmoid(_layer_norm(g[:, :Fn], p["reset_gamma"], p["reset_beta"]))
    u = torch.sigmoid(_layer_norm(g[:, Fn:], p["update_gamma"], p["update_beta"]))
    c = _conv2d_same(torch.cat([x, r * h], 1), p["out_w"], p["out_b"])
    y = torch.tanh(_layer_norm(c, p["out_gamma"], p["out_beta"]))
    return u * h + (1.0 - u) * y


def recurrent_reg(features, t8, gp):
    """features (N,H,W,C), t8 (N-1,D,8) -> regularised cost (D,H,W), plane by plane (model.py:563-589)."""
    cost = cost_volume(features, t8)                              # (C,D,H,W)
    _C, D, H, W = cost.shape
    f = [int(gp[k]["out_b"].shape[0]) for k in ("gru1", "gru2", "gru3")]
    s = [torch.zeros((1, n, H, W), dtype=cost.dtype) for n in f]
    planes = []
    for d in range(D):
        s[0] = conv_gru_cell(-cost[:, d][None], s[0], gp["gru1"])
        s[1] = conv_gru_cell(s[0], s[1], gp["gru2"])
        s[2] = conv_gru_cell(s[1], s[2], gp["gru3"])
        planes.append(_conv2d_same(s[2], gp["prob_w"], gp["prob_b"])[0, 0])
    return torch.stack(planes, 0)


def classification_loss(reg, gt, depth_start, depth_interval):
    """loss.py:223-247 on one sample: reg (D,H,W) -> softmax over planes -> masked cross entropy against the
    one-hot of round((gt - start) / interval); gt (H,W), zeros = invalid."""
    D = reg.shape[0]
    prob = torch.softmax(reg, 0)
    mask = (gt != 0).to(reg.dtype)
    index = torch.round(mask * (gt - depth_start) / depth_interval).to(torch.int64)
    onehot = torch.zeros_like(prob)
    inside = (index >= 0) & (index < D)
    onehot.scatter_(0, index.clamp(0, D - 1)[None], inside[None].to(reg.dtype))
    ce = -(onehot * torch.log(prob)).sum(0)
    return (mask * ce).sum() / (mask.sum() + 1e-7)


# ---- UNetDS2GN towers (mvsnetworks.py:53-115; conv_gn / deconv_gn network.py:217-276, 350-409) ------------------
# Dtype-generic on purpose: run on float32 tensors the same expressions give the float32 noise floor that the device
# tests derive their bound from (tests/test_gpu_towers_backward.py).

def _pad_same2d(x, k, stride):
    """x (V,C,H,W): TensorFlow SAME padding on the two trailing axes."""
    pads = []
    for n in reversed(x.shape[-2:]):
        _, pb, pa = O.same_pad(int(n), k, stride)
        pads += [pb, pa]
    return F.pad(x, pads)


def _conv2d_nchw(x, w, stride):
    return F.conv2d(_pad_same2d(x, int(w.shape[0]), stride), w.permute(3, 2, 0, 1), stride=stride)


def _deconv2d_nchw(x, w, stride=2):
    k = int(w.shape[0])
    y = F.conv_transpose2d(x, w.permute(3, 2, 0, 1), stride=stride)
    H, W = x.shape[-2:]
    pb_h, pb_w = O.same_pad(stride * H, k, stride)[1], O.same_pad(stride * W, k, stride)[1]
    return y[..., pb_h:pb_h + stride * H, pb_w:pb_w + stride * W]


def _gn_relu_nchw(x, gamma, beta, relu, eps=1e-5):
    y = F.group_norm(x, max(1, x.shape[1] // 8), gamma, beta, eps=eps)
    return F.relu(y) if relu else y


def conv2d_same(x, w, stride):
    """x (V,H,W,Cin), w TF layout (k,k,Cin,Cout) -> (V,ceil(H/stride),ceil(W/stride),Cout): tf.layers.conv2d SAME, no bias."""
    return _conv2d_nchw(x.permute(0, 3, 1, 2), w, stride).permute(0, 2, 3, 1)


def deconv2d_same(x, w):
    """x (V,H,W,Cin), w TF layout (3,3,Cout,Cin) -> (V,2H,2W,Cout): tf.layers.conv2d_transpose SAME stride 2, no bias."""
    return _deconv2d_nchw(x.permute(0, 3, 1, 2), w).permute(0, 2, 3, 1)


def group_norm_relu(x, gamma, beta, relu):
    """x (V,H,W,C): per view, groups of 8 channels, biased variance, eps 1e-5 (network.py:239-273), then ReLU if `relu`."""
    return _gn_relu_nchw(x.permute(0, 3, 1, 2), gamma, beta, relu).permute(0, 2, 3, 1)


def unet_layer(name, kind, x, p, k, stride):
    """One row of O.UNET_LAYERS on x (V,C,H,W): 'cg' conv + GroupNorm + ReLU, 'dg' transposed conv + GroupNorm, 'c' conv."""
    if kind == "dg":
        return _gn_relu_nchw(_deconv2d_nchw(x, p["w"], stride), p["gamma"], p["beta"], False)
    y = _conv2d_nchw(x, p["w"], stride)
    return _gn_relu_nchw(y, p["gamma"], p["beta"], True) if kind == "cg" else y


def unet_ds2gn(images, p, layer=unet_layer):
    """images (V,H,W,3), p[name] = {'w','gamma','beta'} tensors in the TensorFlow layouts ('w' only for conv10_2) ->
    (V,H/4,W/4,32), differentiable in images and p.  `layer`: what computes one row of the table -- the sensitivity tests
    (tests/test_towers_oracle_host.py) substitute a deliberately wrong one for a single layer."""
    layers = {"data": images.permute(0, 3, 1, 2)}
    for name, kind, srcs, k, _mult, stride in O.UNET_LAYERS:
        x = layers[srcs[0]] if len(srcs) == 1 else torch.cat([layers[s] for s in srcs], 1)
        layers[name] = layer(name, kind, x, p[name], k, stride)
    return layers["conv10_2"].permute(0, 2, 3, 1)


def unet_ds2gn_gradients(images, params, g, dtype=torch.float64, layer=unet_layer):
    """numpy images (V,H,W,3), params[name][key], g (V,H/4,W/4,32) -> (features, {(name, key): gradient of sum(features * g)})
    as numpy arrays, everything computed in `dtype`."""
    mk = lambda a, grad=False: torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(grad)
    p = {name: {key: mk(v, True) for key, v in d.items()} for name, d in params.items()}
    f = unet_ds2gn(mk(images), p, layer)
    (f * mk(g)).sum().backward()
    return f.detach().numpy(), {(name, key): t.grad.numpy() for name, d in p.items() for key, t in d.items()}


# ---- regression loss (loss.py:31-92, 134-220) --------------------------------------------------------------------------
# Written from the reference, NOT from mvsnet_amd/loss.py (the code under test in tests/test_gpu_train_step.py); dtype-generic
# like the towers above.

def power_loss(y_true, y_pred, interval, alpha, beta):
    """loss.py:31-92 (no_interval_norm=False): 10 mean_true^beta / interval^alpha x the sum over valid pixels of
    (|y_true - y_pred| + 0.005 y_true)^alpha / (y_true^beta x number of valid pixels); (B,H,W,1) -> (B,)."""
    mask = (y_true != 0).to(y_pred.dtype)                                   # :56
    num_valid = mask.sum(dim=(1, 2, 3)).abs() + 1e-6                        # :58-59
    if beta == 0.0:                                                        # :62-67
        denominator = num_valid.view(-1, 1, 1, 1)
    else:
        denominator = torch.pow(y_true + 1e-9, beta) * num_valid.view(-1, 1, 1, 1)
    numerator = (y_true - y_pred).abs() + 0.005 * y_true                   # :70-71
    if alpha != 1.0:
        numerator = torch.pow(numerator, alpha)                            # :72-74
    loss = (numerator * mask / denominator).sum(dim=(1, 2, 3))              # :76-78
    mean_true = (y_true * mask).sum() / num_valid                           # :81-82
    return loss * (10.0 * torch.pow(mean_true, beta) / torch.pow(interval.view(-1), alpha))     # :87-89


def gradient_loss_terms(y_true, y_pred):
    """The arguments of the two log(1 + .) sums of loss.py:134-158 BEFORE the absolute value, their pair masks and the mask.  The reference
    slices the first two axes of whatever it is given -- for the (B,H,W,1) batch the "vertical" term differences the batch axis
    (empty below three samples) and the "horizontal" one the image rows; reproduced as written."""
    mask = (y_true != 0).to(y_pred.dtype)                                   # :140
    diff = y_true - y_pred                                                 # :142
    v_mask, h_mask = mask[0:-2, :] * mask[2:, :], mask[:, 0:-2] * mask[:, 2:]           # :145, :149
    v = (diff[0:-2, :] - diff[2:, :]) * v_mask                             # :144-146
    h = (diff[:, 0:-2] - diff[:, 2:]) * h_mask                             # :148-150
    return v, h, v_mask, h_mask, mask


def gradient_loss(y_true, y_pred):
    """loss.py:134-158 with log=True."""
    v, h, _vm, _hm, mask = gradient_loss_terms(y_true, y_pred)
    return (torch.log(1.0 + v.abs()).sum() + torch.log(1.0 + h.abs()).sum()) / mask.sum()       # :152-158


def regression_loss(est, gt, depth_start, depth_end, loss_type="power", alpha=0.25, beta=0.0, grad_loss=True):
    """mvsnet_regression_loss (loss.py:189-220) on est, gt (B,H,W,1) in est's dtype: (loss, less_one, less_three, debug),
    differentiable in est.  interval = (end - start) / 191 whatever the number of planes (:194); 'original' (:15-28) and 'power'
    losses; the gradient loss enters with 0.5 (:208-210).  The reference adds the scalar gradient loss to a per-sample vector;
    the sum over the samples returned here is that vector's only entry at batch size one, the size the trainer runs."""
    dt = est.dtype
    as_t = lambda v: torch.as_tensor(np.asarray(v, np.float64).reshape(-1)).to(dt)
    gt = gt.to(dt)
    interval = (as_t(depth_end) - as_t(depth_start)) / 191.0                 # :194
    mask = (gt != 0).to(dt)
    if loss_type == "original":                                            # :15-28
        denom = mask.sum(dim=(1, 2, 3)).abs() + 1e-6
        loss = (((mask * (gt - est)).abs().sum(dim=(1, 2, 3)) / interval) / denom).sum()
    elif loss_type == "power":
        loss = power_loss(gt, est, interval, alpha, beta).sum()
    else:
        raise NotImplementedError(loss_type)
    debug = None
    if grad_loss:
        debug = gradient_loss(gt, est)
        loss = loss + 0.5 * debug                                          # :208-210
    rel = (gt - est).abs() / interval.view(-1, 1, 1, 1)                    # :168-170
    denom = mask.sum().abs() + 1e-6
    less_one = (mask * (rel <= 1.0).to(dt)).sum() / denom                   # :171-173
    less_three = (mask * (rel <= 3.0).to(dt)).sum() / denom                 # :185-187
    return loss, less_one, less_three, debug
