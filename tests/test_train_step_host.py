"""Host side of the whole-step oracle (tests/train_reference.py; no GPU): the loss restatement against the strict numpy one and
against central differences, hand-computed updates of the three optimisers, that the inputs of tests/test_gpu_train_step.py keep
clear of every kink, and that the comparison that file makes CAN fail -- the float32 CPU run stands in for the device, and each
deliberately wrong step of the kind the assembly could make lands outside the bound the GPU test uses.

Measured on one CPU (the floors move with the float32 summation order, i.e. the thread count: 9.4e-05 .. 1.2e-04 for normal / 3DCNN),
conditioned first step (margins in depth units, `noise` = the absolute float32-vs-float64
distance of the depth map -- for the recurrent regulariser of the regularised cost; `gate` = the smallest ratio over the ReLU layers
of min |ReLU input| to that layer's own float32 noise):
  configuration   abs error  grad argument  less one  less three  noise     gate           gradient floor   depth     loss
  normal, 3DCNN   0.111      0.222          0.111     0.111       1.57e-04  17 (3dconv6_0) 9.35e-05         3.45e-07  1.67e-07
  lite, 3DCNN     0.111      0.222          0.111     0.111       1.44e-04  18 (3dconv6_0) 1.71e-04         3.15e-07  2.77e-08
  normal, GRU     index tie 0.282, less one / three 0.271         2.07e-05  22 (2dconv8_2) 3.66e-05         2.87e-08  5.81e-08
(3DCNN: the margins are those tracking_ground_truth builds in, 0.5 and 1 loss intervals of 0.222; all exceed 700 x the noise.  GRU:
5 of 384 pixels have an undecided winner-take-all plane and are left out of the depth comparison.)  Without the conditioning the
same batch has a gradient-loss argument of 1.7e-2, an accuracy threshold 3.7e-3 from a pixel and ReLU inputs down to 1.8e-6, of
which the float32 run flips one: gradient floor 1.7e-3 instead of 9e-5.
"""
import math

import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from oracle import torch_grad as TG
from _helpers import tensor_distance
import train_reference as R

CONFIGS = [("normal", "3DCNN"), ("lite", "3DCNN"), ("normal", "GRU")]


# ---- the loss restatement ----------------------------------------------------------------------------------------------

def _depth_and_gt():
    fl = R.floor("normal", "3DCNN")
    prob = R.step_problem("normal", "3DCNN")
    return fl["r64"][3][None, :, :, None], np.asarray(prob["gt"], np.float64)[None], prob


@pytest.mark.parametrize("grad_loss", [True, False])
def test_loss_restatement_equals_the_numpy_metrics(grad_loss):
    """loss_type 'original' is what O.regression_metrics states: loss, both accuracies and the gradient loss to 1e-12, on the
    float64 depth map of the problem against its ramp (accuracies strictly between 0 and 1)."""
    est, gt, prob = _depth_and_gt()
    want = O.regression_metrics(est, gt, [prob["start"]], [prob["end"]], grad_loss=grad_loss)
    got = TG.regression_loss(torch.tensor(est), torch.tensor(gt), [prob["start"]], [prob["end"]], loss_type="original",
                             grad_loss=grad_loss)
    assert 0 < want[1] < want[2] < 1
    for g, w in zip(got[:3], want[:3]):
        assert abs(float(g) - w) <= 1e-12 * abs(w), (float(g), w)
    if grad_loss:
        assert abs(float(got[3]) - want[3]) <= 1e-12 * abs(want[3])
    else:
        assert got[3] is None and want[3] is None


def test_power_loss_by_hand():
    """Two valid pixels and an invalid one, alpha = 0.25, beta = 0 (loss.py:31-92): 10 / interval^alpha x the mean over the valid
    pixels of (|gt - est| + 0.005 gt)^alpha; beta = 0.5 divides each pixel by gt^beta and multiplies by mean(gt)^beta."""
    gt = torch.tensor([500.0, 0.0, 600.0], dtype=torch.float64).view(1, 3, 1, 1)
    est = torch.tensor([498.0, 777.0, 603.5], dtype=torch.float64).view(1, 3, 1, 1)
    start, end = 425.0, 425.0 + 191.0 * 2.0                                 # interval 2
    a, b = (2.0 + 2.5) ** 0.25, (3.5 + 3.0) ** 0.25
    want = 10.0 / 2.0 ** 0.25 * (a + b) / (2.0 + 1e-6)
    got = TG.regression_loss(est, gt, [start], [end], "power", 0.25, 0.0, grad_loss=False)
    assert abs(float(got[0]) - want) <= 1e-12 * want
    assert float(got[1]) == pytest.approx(0.5, abs=1e-6) and float(got[2]) == pytest.approx(1.0, abs=1e-6)   # 1 and 1.75 intervals
    want = 10.0 * (1100.0 / (2.0 + 1e-6)) ** 0.5 / 2.0 ** 0.25 * (a / (500.0 + 1e-9) ** 0.5 + b / (600.0 + 1e-9) ** 0.5) / (2.0 + 1e-6)
    got = TG.regression_loss(est, gt, [start], [end], "power", 0.25, 0.5, grad_loss=False)
    assert abs(float(got[0]) - want) <= 1e-12 * want


def test_loss_gradient_agrees_with_central_differences():
    """Trainer's flags (power loss, alpha 0.25, gradient loss) on the conditioned problem: autograd of the restatement against
    central differences in float64 at a valid pixel of each row class, an invalid pixel (gradient exactly zero) and a corner."""
    fl = R.floor("normal", "3DCNN")
    prob = fl["r64"].problem
    est0, gt = fl["r64"][3], torch.tensor(np.asarray(prob["gt"], np.float64)[None])
    f = lambda e: TG.regression_loss(e[None, :, :, None], gt, [prob["start"]], [prob["end"]], **R.LOSS_ARGS)[0]
    e = torch.tensor(est0, requires_grad=True)
    f(e).backward()
    h = 1e-5
    for r, c in [(0, 1), (4, 7), (5, 8), (6, 9), (7, 10), (15, 23)]:
        d = np.zeros_like(est0); d[r, c] = h
        num = (float(f(torch.tensor(est0 + d))) - float(f(torch.tensor(est0 - d)))) / (2 * h)
        got = float(e.grad[r, c])
        assert abs(got - num) <= 1e-7 * max(abs(num), 1e-3), ((r, c), got, num)
    assert float(e.grad[0, 1]) == 0.0 and prob["gt"][0, 1, 0] == 0.0


# ---- the update formulas -------------------------------------------------------------------------------------------------

W, G0, G1 = [1.0, -2.0, 0.5], [0.5, -1.0, 2.0], [-0.25, 4.0, 1.0]
LR = [0.1, 0.1 * 0.5 ** 0.5]           # exponential_decay(0.1, step, 2, 0.5) at step 0, 1: 0.1, 0.0707107
KAT_RTOL = 2e-5                        # the formulas take the float32 values of the hyper-parameters: 1 - float32(0.999) is 1.3e-5 from 0.001


def _two_steps(kind, scale=1.0):
    w, slots, step = np.array(W), R.initial_slots(kind, 3), 0
    out = []
    for g in (G0, G1):
        w, slots, step = R.optimizer_update(kind, w, np.array(g), slots, step, 0.1, 2, 0.5, scale)
        out.append((w, slots, step))
    return out


def test_rmsprop_update_by_hand():
    (w1, s1, t1), (w2, s2, t2) = _two_steps("rmsprop")
    for i in range(3):
        ms1 = 1.0 + (G0[i] ** 2 - 1.0) * 0.1                              # the rms slot starts at ONE
        u1 = LR[0] * G0[i] / math.sqrt(ms1 + 1e-10)
        ms2 = ms1 + (G1[i] ** 2 - ms1) * 0.1
        u2 = LR[1] * G1[i] / math.sqrt(ms2 + 1e-10)                       # momentum 0: the slot is the last update
        assert s1[0][i] == pytest.approx(ms1, rel=KAT_RTOL) and s1[1][i] == pytest.approx(u1, rel=KAT_RTOL)
        assert s2[0][i] == pytest.approx(ms2, rel=KAT_RTOL) and s2[1][i] == pytest.approx(u2, rel=KAT_RTOL)
        assert w1[i] - W[i] == pytest.approx(-u1, rel=KAT_RTOL) and w2[i] - W[i] == pytest.approx(-u1 - u2, rel=KAT_RTOL)
    assert s1[0][0] == pytest.approx(0.925, rel=KAT_RTOL) and w1[0] == pytest.approx(1.0 - 0.05 / math.sqrt(0.925), rel=KAT_RTOL)
    assert (t1, t2) == (1, 2)


def test_momentum_update_by_hand():
    (w1, s1, t1), (w2, s2, t2) = _two_steps("momentum")
    for i in range(3):
        a1 = G0[i]
        a2 = 0.9 * a1 + G1[i]
        assert s1[0][i] == pytest.approx(a1, rel=KAT_RTOL) and s2[0][i] == pytest.approx(a2, rel=KAT_RTOL)
        assert w1[i] - W[i] == pytest.approx(-LR[0] * a1, rel=KAT_RTOL)
        assert w2[i] - W[i] == pytest.approx(-LR[0] * a1 - LR[1] * a2, rel=KAT_RTOL)
    assert w2[2] == pytest.approx(0.5 - 0.2 - 0.0707106781 * 2.8, rel=KAT_RTOL) and (t1, t2) == (1, 2)


def test_adam_update_by_hand():
    (w1, s1, t1), (w2, s2, t2) = _two_steps("adam")
    for i in range(3):
        m1, v1 = 0.1 * G0[i], 0.001 * G0[i] ** 2
        lr1 = LR[0] * math.sqrt(1 - 0.999) / (1 - 0.9)                    # t = 1
        u1 = lr1 * m1 / (math.sqrt(v1) + 1e-8)
        m2, v2 = m1 + (G1[i] - m1) * 0.1, v1 + (G1[i] ** 2 - v1) * 0.001
        lr2 = LR[1] * math.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)          # t = 2
        u2 = lr2 * m2 / (math.sqrt(v2) + 1e-8)
        assert s1[0][i] == pytest.approx(m1, rel=KAT_RTOL) and s1[1][i] == pytest.approx(v1, rel=KAT_RTOL)
        assert s2[0][i] == pytest.approx(m2, rel=KAT_RTOL) and s2[1][i] == pytest.approx(v2, rel=KAT_RTOL)
        assert w1[i] - W[i] == pytest.approx(-u1, rel=KAT_RTOL) and w2[i] - W[i] == pytest.approx(-u1 - u2, rel=KAT_RTOL)
        assert abs(u1) == pytest.approx(0.1, rel=1e-6)                     # Adam's first step is lr x sign(g)
    assert (t1, t2) == (1, 2)


def test_gradient_scale_enters_before_the_squares():
    """scale = 1 / towers (average_gradients): the update of (g, scale 0.5) is the update of g / 2."""
    for kind in ("rmsprop", "momentum", "adam"):
        a = R.optimizer_update(kind, np.array(W), np.array(G0), R.initial_slots(kind, 3), 0, 0.1, 2, 0.5, 0.5)
        b = R.optimizer_update(kind, np.array(W), np.array(G0) / 2, R.initial_slots(kind, 3), 0, 0.1, 2, 0.5, 1.0)
        assert np.array_equal(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


# ---- the inputs are suitable ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,regularization", CONFIGS)
def test_inputs_keep_clear_of_every_kink(mode, regularization):
    """From the float64 run of the conditioned first step and the float32 run of the same step: every kink margin exceeds ten times
    the float32 noise of the quantity that would cross it, no ReLU gate differs between the two runs, and the float32 run is float32
    noise away, not another computation.  (The optimiser plays no part: one figure per network.)"""
    fl = R.floor(mode, regularization)
    r64, r32, noise = fl["r64"], fl["r32"], fl["noise"]
    margins = R.kink_margins(r64)
    gates = {k[1]: margins[k] / noise[k] for k in margins if isinstance(k, tuple)}
    worst = min(gates, key=gates.get)
    print("\n%s %s: margins %s; noise %.3e; tightest ReLU layer %s at %.1f x its noise; gradient floor %.3e (%s), depth %.3e, "
          "loss %.3e; undecided pixels %d" % (mode, regularization, {k: "%.3e" % v for k, v in margins.items() if not isinstance(k, tuple)},
                                              noise[None], worst, gates[worst], fl["gradient_floor"],
                                              max(fl["gradients"], key=fl["gradients"].get), fl["depth"], fl["loss"],
                                              int(R.undecided_pixels(r64, noise).sum())))
    assert not R.unsuitable(r64, noise), "inputs unsuitable: %s" % R.unsuitable(r64, noise)
    assert all(np.array_equal(r64.pre[k] > 0, r32.pre[k] > 0) for k in r64.pre)
    assert (r32[1], r32[2]) == pytest.approx((r64[1], r64[2]), abs=1e-6) and 0 < r64[1] < r64[2] < 1
    assert 0 < fl["gradient_floor"] < 1e-3 and 0 < fl["depth"] < 1e-5
    assert R.undecided_pixels(r64, noise).mean() < 0.05
    moved = max(float(np.abs(r64.params[v] - a).max()) for v, a in R.initial_parameters(r64.problem).items())
    assert 0 < moved <= R.GATE_WINDOW * (1 + 1e-6)
    if regularization == "3DCNN":
        assert r64[1] == pytest.approx(2 / 12, abs=0.01) and r64[2] == pytest.approx(5 / 12, abs=0.01)


def test_tracking_ground_truth_has_the_margins_it_promises():
    prob = R.step_problem("normal", "3DCNN")
    depth = np.random.RandomState(0).uniform(430, 460, (16, 24))
    gt = R.tracking_ground_truth(depth, prob)
    u = (prob["end"] - prob["start"]) / 191.0
    valid = gt[:, :, 0] != 0
    rel = np.abs(gt[:, :, 0].astype(np.float64) - depth)[valid] / u
    assert (~valid).sum() == 3 and rel.min() > 0.499
    assert np.abs(rel - 1).min() > 0.499 and np.abs(rel - 3).min() > 0.499
    d = gt[:, :, 0].astype(np.float64) - depth
    assert np.abs(np.abs(d[:-2] - d[2:])[valid[:-2] & valid[2:]] / u - np.array([1.0, 4.0] * 7)[:, None].repeat(24, 1)[valid[:-2] & valid[2:]]).max() < 1e-3


# ---- the bound rejects wrong steps -------------------------------------------------------------------------------------

def _gradient_bound():
    fl = R.floor("normal", "3DCNN")
    return fl, R.MARGIN * fl["gradient_floor"]


def _outside(grads, fl, bound):
    return {v: d for v, d in ((v, tensor_distance(grads[v], fl["r64"][4][v])) for v in fl["gradients"]) if not d <= bound}


def test_the_stand_in_is_inside_the_gradient_bound():
    fl, bound = _gradient_bound()
    assert not _outside(fl["r32"][4], fl, bound)


def test_the_bound_rejects_a_gamma_gradient_added_twice():
    fl, bound = _gradient_bound()
    grads = dict(fl["r32"][4])
    grads["2dconv5_1/gn/gamma"] = 2.0 * grads["2dconv5_1/gn/gamma"]
    assert set(_outside(grads, fl, bound)) == {"2dconv5_1/gn/gamma"}


def _wrong_loss(what):
    def loss(est, gt, start, end, **kw):
        if what == "pixel dropped":                                        # one valid pixel missing from the mask
            gt = gt.clone()
            assert gt[0, 8, 12, 0] != 0
            gt[0, 8, 12, 0] = 0.0
            return TG.regression_loss(est, gt, start, end, **kw)
        value, l1, l3, g_loss = TG.regression_loss(est, gt, start, end, **kw)
        return value + 0.5 * g_loss, l1, l3, g_loss                        # the gradient loss's 0.5 dropped
    return loss


@pytest.mark.parametrize("what", ["pixel dropped", "half dropped"])
def test_the_bound_rejects_a_wrong_loss(what):
    """The float32 run with a deliberately wrong loss leaves the gradient bound (and the loss bound)."""
    fl, bound = _gradient_bound()
    bad = R.whole_step(fl["r64"].params, fl["r64"].problem, torch.float32, loss=_wrong_loss(what))
    out = _outside(bad[4], fl, bound)
    d_loss = abs(bad[0] - fl["r64"][0]) / abs(fl["r64"][0])
    print("\n%s: %d of %d tensors outside %.3e, worst %.3e; loss off by %.3e (bound %.3e)" %
          (what, len(out), len(fl["gradients"]), bound, max(out.values(), default=0.0), d_loss, R.scalar_bound(fl["loss"])))
    assert out and d_loss > R.scalar_bound(fl["loss"])
    assert tensor_distance(bad[3], fl["r64"][3]) <= R.scalar_bound(fl["depth"])         # the forward pass is untouched


def _kernel_in_float32(kind, w, g, slots, global_step, base_lr=1e-3, stepvalue=2, gamma=0.5, scale=1.0, **wrong):
    """The stand-in for the device's update: the kernels' expressions (mvsnet_amd/csrc/optimizer.hip) in numpy float32, with
    the hyper-parameters Trainer.apply_gradients hands them (or deliberately wrong ones)."""
    f = np.float32
    w, gi = w.astype(f), g.astype(f) * f(scale)
    a = slots[0].astype(f) if wrong.get("rms_start") is None else np.full_like(w, wrong["rms_start"])
    lr = R.exponential_decay(base_lr, global_step + wrong.get("lr_step_offset", 0), stepvalue, gamma)
    if kind == "rmsprop":
        ms = a + (gi * gi - a) * (f(1) - f(0.9))
        return w - f(lr) * gi / np.sqrt(ms + f(1e-10))
    t = global_step + wrong.get("adam_t_offset", 1)
    lr_t = f(lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
    m = a + (gi - a) * (f(1) - f(0.9))
    v = slots[1].astype(f) + (gi * gi - slots[1].astype(f)) * (f(1) - f(0.999))
    return w - lr_t * m / (np.sqrt(v) + f(1e-8))


@pytest.mark.parametrize("kind,step,wrong", [("adam", 0, {}), ("rmsprop", 1, {}), ("adam", 1, {"adam_t_offset": 0}),
                                             ("adam", 1, {"lr_step_offset": 1}), ("rmsprop", 1, {"lr_step_offset": 1}),
                                             ("rmsprop", 0, {"scale": 0.5}), ("rmsprop", 0, {"rms_start": 0.0})])
def test_the_update_bound_rejects_wrong_updates(kind, step, wrong):
    """A float32 evaluation of the kernel's expressions on the float32 run's own gradient is inside the per-element update bound;
    with Adam's t one step late, the learning rate of global_step + 1, a gradient scale of 0.5 or an `rms` slot from zero it is
    outside at most elements.  (Slots: one earlier update from the initial ones, so that `rms` is not one everywhere.)"""
    fl = R.floor("normal", "3DCNN")
    for var in ("3dconv0_1/kernel", "2dconv5_1/gn/gamma"):
        w, g = fl["r64"].params[var], fl["r32"][4][var].astype(np.float32)
        slots = R.initial_slots(kind, 1)
        slots = [np.broadcast_to(s, w.shape) for s in slots]
        if step:
            _w, slots, _t = R.optimizer_update(kind, w, 0.7 * g, slots, 0, 1e-3, 2, 0.5)
            slots = [s.astype(np.float32) for s in slots]
        expected = R.optimizer_update(kind, w, g, slots, step, 1e-3, 2, 0.5, 1.0)[0]
        slack = R.rounding_slack(kind, g, slots, step, 1e-3, 2, 0.5)[1]
        err, bound = R.update_errors(w, _kernel_in_float32(kind, w, g, slots, step, **wrong), expected, slack)
        share = float((err > bound).mean())
        print("%s %s %s: %.1f%% of the elements outside the bound" % (kind, var, wrong or "correct", 100 * share))
        assert share == 0.0 if not wrong else share > 0.5, (var, share)
