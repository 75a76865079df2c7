"""Float64 reference of ONE optimisation step of mvsnet_amd.train.Trainer (tests/test_gpu_train_step.py, tests/test_train_step_host.py;
no GPU): images -> UNetDS2GN towers -> variance cost volume -> RegNetUS0 -> soft-argmin -> power loss + gradient loss (or: -> ConvGRU
cells -> classification loss), differentiated by torch-CPU autograd (oracle/torch_grad.py; TensorFlow's autodiff in the reference,
mvsnet/train.py:428-429), and the update TensorFlow's optimisers apply to it (mvsnet/train.py:255-266, 444).

The step is TEACHER-FORCED: it starts from parameters, slots and global_step downloaded from the device (float32 values are exact in
float64), so nothing accumulates from step to step and no division by a noisy quantity sits between the two sides of a comparison.
Dtype-generic: run in float32 the same expressions give the float32 noise floor the device's bound is derived from.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mvsnet_oracle as O
from oracle import torch_grad as TG
from mvsnet_amd import synthetic as S

MARGIN = 3.0               # device bound = MARGIN x the float32 CPU run's largest distance from float64 (tests/test_gpu_towers_backward.py)
KINK_FACTOR = 10.0         # every kink margin must exceed this many float32-vs-float64 distances of the quantity that crosses it
LOSS_ARGS = dict(loss_type="power", alpha=0.25, beta=0.0, grad_loss=True)      # Trainer's defaults (train.py:121-134 of the reference)
GATE_WINDOW = 0.02         # whole_step(condition=True) moves a beta in front of a ReLU by at most this much
SEED = {"3DCNN": 0, "GRU": 0}   # of the initialisation (Trainer(seed=...))
ZERO_GRADIENT = ("prob_conv/bias",)      # true gradient identically zero: held to an absolute bound, not a relative one


# ---- the problem -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def step_problem(mode="normal", regularization="3DCNN"):
    """The batch of tests/test_gpu_backward.py::_train_batch: N = 3 views of 64 x 96, D = 16 planes, so 16 x 24 feature maps and a
    coarsest RegNetUS0 level of 2 x 2 x 3 -- the smallest volume at which every level has more than a couple of voxels per BatchNorm
    channel.  Transforms in float64 and in float32 from the strict numpy restatement (the device computes its own,
    homography_transforms).  Shared and cached: nobody writes to it."""
    N, H, W, D = 3, 64, 96, 16
    images = S.make_images(N, H, W, seed=0)
    cams = S.make_cams(N, H // 4, W // 4, D)
    start, interval, end = float(cams[0, 1, 3, 0]), float(cams[0, 1, 3, 1]), float(cams[0, 1, 3, 3])
    xs = np.linspace(0.31, 0.69, W // 4, dtype=np.float32)[None, :].repeat(H // 4, 0)
    gt = (start + interval * (D - 1) * xs)[:, :, None].astype(np.float32)
    gt[0, :3, 0] = 0.0                                                      # a few invalid pixels
    t8 = {}
    for dt in (np.float64, np.float32):
        Hs = np.stack([O.get_homographies(cams[0], cams[v], D, start, interval, dt) for v in range(1, N)])
        t8[dt] = O.homography_to_transform8(Hs, dt)
    for a in (images, cams, gt, t8[np.float64], t8[np.float32]):
        a.setflags(write=False)
    return dict(mode=mode, regularization=regularization, images=images, cams=cams, gt=gt, depth_num=D, start=start,
                interval=interval, end=end, t8_64=t8[np.float64], t8_32=t8[np.float32])


def with_ground_truth(problem, gt):
    """The same problem with another ground truth."""
    q = dict(problem)
    q["gt"] = np.asarray(gt, np.float32)
    return q


def variable_keys(problem):
    """{variable name: (group, layer, field)} of the configuration's trainable variables."""
    from mvsnet_amd import tf_checkpoint
    return {v: k for k, v in tf_checkpoint.variable_names(problem["mode"], problem["regularization"]).items()}


def initial_parameters(problem, seed=None):
    """{variable name: float32 array}, native shapes: what Trainer(mode, regularization=..., seed=seed) starts from."""
    from mvsnet_amd import train as T
    mode = problem["mode"]
    seed = SEED[problem["regularization"]] if seed is None else seed
    groups = {"unet": T.glorot_uniform_like(S.make_unet_params(mode), seed)}
    if problem["regularization"] == "GRU":
        from mvsnet_amd.gru_train import glorot_gru_params
        groups["gru"] = glorot_gru_params(S.make_gru_params(mode, in_channels=4 * S.base_filter(mode)), seed + 1)
    else:
        groups["regnet"] = T.glorot_uniform_like(S.make_regnet_params(mode), seed + 1)
    out = {}
    for var, (group, layer, field) in variable_keys(problem).items():
        out[var] = np.asarray(groups[group][field] if layer is None else groups[group][layer][field], np.float32)
    return out


def grouped(params, problem):
    """{variable name: value} -> {group: {layer: {field: value}}}, the nesting the oracle's networks take."""
    groups = {}
    for var, (group, layer, field) in variable_keys(problem).items():
        g = groups.setdefault(group, {})
        if layer is None:
            g[field] = params[var]
        else:
            g.setdefault(layer, {})[field] = params[var]
    return groups


# ---- loss and gradient ---------------------------------------------------------------------------------------------------

class StepResult(tuple):
    """(loss, less_one, less_three, depth, {variable name: gradient}) as numpy float64 values of a run in `dtype`, plus what the
    kink margins need: .problem (with the ground truth the run used), .params (the parameters it used, float32), .sensitive -- the
    tensor whose float32 noise moves the outputs towards a kink (the depth map; for the recurrent regulariser the regularised cost,
    whose argmax is the depth map) -- and .pre {layer: the input of its ReLU}."""
    problem = None
    params = None
    sensitive = None
    pre = None


def _clear_of_zero(x, beta):
    """x: a ReLU layer's input (B,C,...), beta (C,) float64 holding float32 values -> the float32 beta (as float64) that moves
    every channel to the middle of the widest gap its inputs leave within +-GATE_WINDOW of zero."""
    flat = x.transpose(0, 1).reshape(x.shape[1], -1).numpy()
    shift = np.zeros(flat.shape[0])
    for c, v in enumerate(flat):
        edges = np.concatenate([[-GATE_WINDOW], np.sort(v[np.abs(v) < GATE_WINDOW]), [GATE_WINDOW]])
        k = int(np.argmax(np.diff(edges)))
        shift[c] = -0.5 * (edges[k] + edges[k + 1])
    return torch.tensor((beta.numpy() + shift).astype(np.float32).astype(np.float64))


def tracking_ground_truth(depth, problem):
    """A ground truth that keeps a FIXED pattern of distances from the given (float64) depth map, in units u of the loss's interval
    (end - start) / 191: rows r add (+0.5, +2, -0.5, -2)[r mod 4], columns c add (0, +4, -6)[c mod 3]; the problem's invalid pixels
    stay invalid.  By construction, whatever the estimate: |gt - est| >= 0.5 u (the power loss's kink), every |gt - est| / u is at
    least 0.5 from 1 and from 3 (2 of 12 pixels within one interval, 5 of 12 within three), and the gradient loss's arguments --
    differences two rows apart in one column -- are +-1 u or +-4 u.  u = 0.22 here against a float32 noise of the depth map of 2e-4.
    A fixed ramp cannot give this: the estimate moves by whole intervals per update, and 381 pixels leave one of the five kinks
    within 10 x that noise in about two steps of five."""
    u = (problem["end"] - problem["start"]) / 191.0
    H, W = depth.shape
    rows = np.array([0.5, 2.0, -0.5, -2.0])[np.arange(H) % 4][:, None]
    cols = np.array([0.0, 4.0, -6.0])[np.arange(W) % 3][None, :]
    gt = (np.asarray(depth, np.float64) + u * (rows + cols)).astype(np.float32)[:, :, None]
    gt[problem["gt"] == 0] = 0.0
    return gt


def _forward(groups, problem, dtype, seen):
    """images -> depth map or regularised cost; `seen(name, make, p)` is handed what computes every ReLU's input and returns what
    the ReLU is applied to."""
    mk = lambda a: torch.tensor(np.asarray(a), dtype=dtype)

    def tower_layer(name, kind, x, p, k, stride):
        if kind != "cg":
            return TG.unet_layer(name, kind, x, p, k, stride)
        y = TG.unet_layer(name, "c", x, p, k, stride)
        gn = lambda: F.group_norm(y, max(1, y.shape[1] // 8), p["gamma"], p["beta"], eps=1e-5)     # network.py:239-273
        return F.relu(seen(name, gn, p))

    def bn_relu(name, x, p):
        return F.relu(seen(name, lambda: F.batch_norm(x, None, None, p["gamma"], p["beta"], training=True, eps=1e-5), p))

    t8 = mk(problem["t8_64"] if dtype == torch.float64 else problem["t8_32"])
    feats = TG.unet_ds2gn(mk(problem["images"]), groups["unet"], tower_layer)
    if problem["regularization"] == "GRU":
        return TG.recurrent_reg(feats, t8, groups["gru"])
    return TG.depth_from_features(feats, t8, problem["start"], problem["interval"], groups["regnet"], bn_relu)


def whole_step(params, problem, dtype=torch.float64, loss=TG.regression_loss, condition=False):
    """params {variable name: array of the native shape} -> StepResult.  3DCNN: TG.unet_ds2gn -> TG.depth_from_features -> `loss`
    (TG.regression_loss with Trainer's flags; the sensitivity tests substitute deliberately wrong ones); GRU: TG.unet_ds2gn ->
    TG.recurrent_reg -> TG.classification_loss, the depth map winner-take-all and the accuracies in units of |depth_interval|
    (loss.py:253-265).

    `condition` (float64 only) makes the step well conditioned while it is evaluated; the caller hands result.params and
    result.problem to whatever it compares with.
      * ReLU gates.  A gate is a kink of the loss like the |.| of the loss itself, and a network of this size has a few ReLU inputs
        within float32 noise of zero whatever the seed (about 1e6 inputs of density ~0.4 per unit around zero; noise 1e-6 in the
        towers, 5e-5 behind the 12-voxel BatchNorm levels).  Such a gate opens in one float32 evaluation and stays shut in another:
        ONE flipped gate of 3dconv6_0 moves that layer's kernel gradient by 1.7e-3 of its largest entry, twenty times the float32
        floor of the whole step (measured: the float32 CPU run of the unconditioned first step flips one).  So, layer by layer in
        the order of evaluation, every beta in front of a ReLU moves by at most GATE_WINDOW to where its channel's inputs leave the
        widest gap around zero.  The moved betas are float32 values.
      * The loss's own kinks (3DCNN): the ground truth follows the depth map of this run, tracking_ground_truth."""
    keys = variable_keys(problem)
    assert set(params) == set(keys), sorted(set(params) ^ set(keys))
    assert not condition or dtype == torch.float64
    mk = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    leaves = {var: mk(a).requires_grad_(True) for var, a in params.items()}
    pre = {}

    def seen(name, make, p):
        if condition:
            with torch.no_grad():
                p["beta"].copy_(_clear_of_zero(make(), p["beta"]))
        x = make()
        pre[name] = x.detach().numpy().astype(np.float64)
        return x

    out = _forward(grouped(leaves, problem), problem, dtype, seen)
    start, interval = problem["start"], problem["interval"]
    if condition and problem["regularization"] != "GRU":
        problem = with_ground_truth(problem, tracking_ground_truth(out.detach().numpy(), problem))
    gt = mk(problem["gt"][:, :, 0])
    if problem["regularization"] == "GRU":
        value = TG.classification_loss(out, gt, start, interval)
        with torch.no_grad():                                              # loss.py:253-265
            depth = torch.argmax(torch.softmax(out, 0), 0).to(dtype) * interval + start
            mask = (gt != 0).to(dtype)
            rel = (gt - depth).abs() / abs(interval)
            denom = mask.sum().abs() + 1e-6
            less_one, less_three = (mask * (rel <= 1.0).to(dtype)).sum() / denom, (mask * (rel <= 3.0).to(dtype)).sum() / denom
    else:
        depth = out
        value, less_one, less_three, _debug = loss(depth[None, :, :, None], gt[None, :, :, None], [start], [problem["end"]],
                                                   **LOSS_ARGS)
    value.backward()
    f = lambda x: x.detach().numpy().astype(np.float64)
    res = StepResult((float(value.detach()), float(less_one), float(less_three), f(depth),
                      {var: f(x.grad) for var, x in leaves.items()}))
    res.problem, res.sensitive, res.pre = problem, f(out), pre
    res.params = {var: x.detach().numpy().astype(np.float32) for var, x in leaves.items()}
    return res


def kink_margins(result):
    """The smallest distance of a run to each point where its loss is not differentiable or one of its outputs jumps, in depth
    units (the regularised cost's for 'argmax gap') so that they compare with an absolute distance of result.sensitive:
      'abs error'      min |gt - est| over valid pixels: the kink of the power loss's |.| (loss.py:71);
      'grad argument'  the smallest absolute argument of the gradient loss's log(1 + |.|) terms over their masks (loss.py:144-155);
      'less one/three' min | |gt - est| / interval_191 - k | x interval_191 over valid pixels, k = 1, 3: where an accuracy flips.
    Recurrent regulariser: the cross entropy is smooth in the regularised cost, and its depth map is the cost's argmax.  An untrained
    sweep leaves near-ties between neighbouring planes at a few pixels whatever the seed, so the argmax is no condition: the
    comparison leaves out the pixels undecided_pixels names and counts them against the accuracies.  Conditions:
      'index tie'      min | frac((gt - start) / interval) - 0.5 | x |interval| over valid pixels: where the class index jumps;
      'less one/three' as above for the winner-take-all depth and |depth_interval|.
    And per ReLU layer, in units of its input: ('relu', layer) = min |input|."""
    p = result.problem
    gt, depth = np.asarray(p["gt"][:, :, 0], np.float64), result[3]
    valid = gt != 0
    err = np.abs(gt - depth)[valid]
    out = {}
    if p["regularization"] == "GRU":
        unit = abs(p["interval"])
        index = (gt[valid] - p["start"]) / p["interval"]
        out["index tie"] = float(np.abs(index - np.floor(index) - 0.5).min() * unit)
    else:
        out["abs error"] = float(err.min())
        t = lambda a: torch.tensor(a[None, :, :, None])
        v, h, vm, hm, _m = TG.gradient_loss_terms(t(gt), t(depth))
        args = np.concatenate([np.abs(v.numpy())[vm.numpy() != 0], np.abs(h.numpy())[hm.numpy() != 0]])
        out["grad argument"] = float(args.min())
        unit = (p["end"] - p["start"]) / 191.0
    out["less one"] = float(np.abs(err / unit - 1.0).min() * unit)
    out["less three"] = float(np.abs(err / unit - 3.0).min() * unit)
    for name, x in result.pre.items():
        out["relu", name] = float(np.abs(x).min())
    return out


def scalar_bound(measured_floor):
    """The bound for the loss and the depth map: MARGIN x the float32 run's own relative distance -- but that distance is ONE sample
    (of one scalar, for the loss), which luck can put below what float32 can represent at all, so never less than MARGIN x 2^-23,
    the spacing of float32 relative to the value."""
    return MARGIN * max(measured_floor, 2.0 ** -23)


def undecided_pixels(result, noise):
    """Recurrent regulariser: (H,W) mask of the pixels whose two largest regularised costs are within KINK_FACTOR x the float32
    noise of the cost -- their winner-take-all plane is not decided at float32.  All False for the 3D CNN (soft-argmin)."""
    if result.problem["regularization"] != "GRU":
        return np.zeros(result[3].shape, bool)
    top = np.sort(result.sensitive, axis=0)
    return ~((top[-1] - top[-2]) > KINK_FACTOR * noise[None])


def float32_noise(r32, r64):
    """What the margins are compared with: the absolute float32-vs-float64 distance of .sensitive (under None) and of every ReLU
    layer's input (under ('relu', layer))."""
    noise = {("relu", name): float(np.abs(r32.pre[name] - x).max()) for name, x in r64.pre.items()}
    noise[None] = float(np.abs(r32.sensitive - r64.sensitive).max())
    return noise


def unsuitable(result, noise):
    """[(margin name, margin, its noise)] of the margins that do not exceed KINK_FACTOR x their float32 noise: a comparison across
    such a margin would compare two different branches, not two roundings."""
    bad = []
    for k, v in kink_margins(result).items():
        n = noise.get(k, noise[None])
        if not v > KINK_FACTOR * n:
            bad.append((k, v, n))
    return bad


@functools.lru_cache(maxsize=None)
def floor(mode, regularization):
    """The float32 CPU run of the conditioned first step against the float64 one, cached per configuration and shared (nobody
    writes to it): dict(r64, r32, gradients={variable: tensor_distance}, gradient_floor, depth, loss, noise).  Variables whose
    true gradient is identically zero (prob_conv/bias: a softmax over the planes does not see a bias shared by all planes) have no
    relative distance and are left out of `gradients`."""
    from _helpers import tensor_distance
    problem = step_problem(mode, regularization)
    r64 = whole_step(initial_parameters(problem), problem, torch.float64, condition=True)
    r32 = whole_step(r64.params, r64.problem, torch.float32)
    grads = {v: tensor_distance(r32[4][v], g) for v, g in r64[4].items() if v not in ZERO_GRADIENT}
    return dict(r64=r64, r32=r32, gradients=grads, gradient_floor=max(grads.values()), depth=tensor_distance(r32[3], r64[3]),
                loss=abs(r32[0] - r64[0]) / abs(r64[0]), noise=float32_noise(r32, r64))


# ---- the update -----------------------------------------------------------------------------------------------------------

_f32 = lambda v: float(np.float32(v))          # the kernels receive their hyper-parameters as float32


def exponential_decay(base_lr, global_step, stepvalue, gamma):
    """tf.train.exponential_decay(base_lr, global_step, decay_steps=stepvalue, decay_rate=gamma), staircase=False
    (mvsnet/train.py:256-257)."""
    return base_lr * gamma ** (float(global_step) / float(stepvalue))


def optimizer_update(kind, w, g, slots, global_step, base_lr, stepvalue, gamma, scale=1.0):
    """One update of TensorFlow's optimiser `kind` as mvsnet/train.py:257-266 sets it up, in float64 on float32 inputs:
    (w, g, slots before, global_step before) -> (w after, slots after, global_step + 1).  `scale`: average_gradients' 1 / towers
    (train.py:155-187).
      rmsprop   tf.train.RMSPropOptimizer(learning_rate=lr) (train.py:259): decay 0.9, momentum 0.0, epsilon 1e-10 (its defaults),
                slots (rms, momentum), rms starting at ONE:  rms += (g^2 - rms) (1 - decay); mom = momentum mom + lr g / sqrt(rms + eps);
                w -= mom
      momentum  tf.train.MomentumOptimizer(lr, momentum=0.9, use_nesterov=False) (train.py:262-263): accum = 0.9 accum + g; w -= lr accum
      adam      tf.train.AdamOptimizer(learning_rate=lr) (train.py:266): beta1 0.9, beta2 0.999, epsilon 1e-8 (its defaults), t = the
                number of this update counted from one:  lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t); m += (g - m)(1 - beta1);
                v += (g^2 - v)(1 - beta2); w -= lr_t m / (sqrt(v) + eps)
    lr = exponential_decay at global_step BEFORE the update (train.py:256-257; apply_gradients increments it afterwards, :444)."""
    w, gs = np.asarray(w, np.float64), np.asarray(g, np.float64) * _f32(scale)
    a = np.array(slots[0], np.float64)
    lr = exponential_decay(base_lr, global_step, stepvalue, gamma)
    if kind == "rmsprop":
        decay, momentum, eps = _f32(0.9), _f32(0.0), _f32(1e-10)            # train.py:259: RMSPropOptimizer's defaults
        a = a + (gs * gs - a) * (1.0 - decay)
        b = momentum * np.asarray(slots[1], np.float64) + _f32(lr) * gs / np.sqrt(a + eps)
        return w - b, [a, b], global_step + 1
    if kind == "momentum":
        a = _f32(0.9) * a + gs                                              # train.py:262-263: momentum=0.9
        return w - _f32(lr) * a, [a], global_step + 1
    if kind == "adam":
        beta1, beta2, eps = 0.9, 0.999, _f32(1e-8)                          # train.py:266: AdamOptimizer's defaults
        t = global_step + 1
        lr_t = _f32(lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
        a = a + (gs - a) * (1.0 - _f32(beta1))
        b = np.asarray(slots[1], np.float64)
        b = b + (gs * gs - b) * (1.0 - _f32(beta2))
        return w - lr_t * a / (np.sqrt(b) + eps), [a, b], global_step + 1
    raise NotImplementedError(kind)


def initial_slots(kind, n):
    """TensorFlow's slot initialisers: RMSProp's `rms` at one, everything else at zero."""
    if kind == "rmsprop":
        return [np.ones(n), np.zeros(n)]
    return [np.zeros(n)] * (1 if kind == "momentum" else 2)


def ulp_f32(x):
    """Spacing of float32 at |x| (x given in float64)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def rounding_slack(kind, g, slots, global_step, base_lr, stepvalue, gamma, scale=1.0):
    """(absolute allowance for slot 0, for the parameter delta), per element: what float32 rounding INSIDE a cancelling sum costs.
    Momentum's accum = 0.9 accum + g and Adam's m += (g - m) 0.1 subtract two numbers of opposite sign once the gradient turns
    against the moving average (it never does in tests/test_gpu_backward.py::_optimizer_steps, which feeds one gradient three
    times): the float32 result is good to an ulp of the larger OPERAND, not to 1e-5 of the possibly tiny result, and the update
    formed from it inherits that error times lr (Adam: lr_t / (sqrt(v) + eps)).  RMSProp's rms += (g^2 - rms) 0.1 keeps at least
    0.9 rms: no cancellation, no allowance."""
    gs = np.abs(np.asarray(g, np.float64) * _f32(scale))
    lr = exponential_decay(base_lr, global_step, stepvalue, gamma)
    if kind == "momentum":
        e = ulp_f32(np.maximum(_f32(0.9) * np.abs(slots[0]), gs))
        return e, _f32(lr) * e
    if kind == "adam":
        t = global_step + 1
        e = ulp_f32(np.maximum(np.abs(slots[0]), gs))
        v = np.asarray(slots[1], np.float64)
        v = v + (gs * gs - v) * (1.0 - _f32(0.999))
        return e, _f32(lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)) * e / (np.sqrt(v) + _f32(1e-8))
    return np.zeros_like(gs), np.zeros_like(gs)


def update_errors(w_before, w_after, w_expected, slack=0.0):
    """The update bound, per element: the kernel forms the update in float32 and rounds w - update once, so
    |delta_device - delta_expected| <= 1/2 ulp_f32(w_after) + 1e-5 |delta_expected| + slack (1e-5: the relative tolerance
    tests/test_gpu_backward.py::_assert_optimizer grants these kernels; slack: rounding_slack's second value).  Returns
    (error, bound) arrays; the deltas are exact in float64."""
    w_before = np.asarray(w_before, np.float64)
    delta_dev, delta_exp = np.asarray(w_after, np.float64) - w_before, np.asarray(w_expected, np.float64) - w_before
    return np.abs(delta_dev - delta_exp), 0.5 * ulp_f32(w_after) + 1e-5 * np.abs(delta_exp) + slack
