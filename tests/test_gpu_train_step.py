"""Whole optimisation steps of mvsnet_amd.train.Trainer against the float64 oracle of tests/train_reference.py: three TEACHER-FORCED
steps per configuration.  Before every step the device's parameters, slots and global_step are downloaded (float32 is exact in
float64) and the oracle evaluates the same step from them, so nothing accumulates and no division by a noisy quantity sits between
the two sides:
  * loss and gradient: the device's loss, accuracies, depth map and ALL of params.grad after loss.backward(), variable by variable;
  * update: from the device's OWN gradient, what TensorFlow's formulas (mvsnet/train.py:255-266) give for every parameter delta,
    every slot and global_step; the gradient buffer is exactly zero afterwards.
stepvalue = 2 and gamma = 0.5 make the (non-staircase) learning rate differ visibly at steps 0, 1, 2; Adam sees t = 1, 2, 3.

Conditioning.  The oracle run moves every beta in front of a ReLU by at most 0.02 so that no ReLU input sits within float32 noise of
zero, and (3D CNN) builds the step's ground truth around its own depth map (whole_step(condition=True), tracking_ground_truth: why,
and the margins); the moved betas are uploaded before the device runs the step.  Every margin is re-asserted at every step from the
float64 run: a violation fails with "inputs unsuitable" instead of comparing across a kink.  tests/test_train_step_host.py shows on
the CPU that the bounds below reject a doubled gamma gradient, a pixel missing from the mask, the gradient loss's 0.5 dropped, Adam's
t one step late, the learning rate of global_step + 1, a gradient scale of 0.5 and an `rms` slot from zero.

Gradient bound: measured, not chosen -- 3 x the largest tensor_distance any gradient tensor of the float32 CPU run of the first step
has from the float64 run (another float32 summation order on the device, not another arithmetic; the convention of
tests/test_gpu_towers_backward.py).  Loss (relative) and depth map (tensor_distance): 3 x the same run's distance, but never below
3 x 2^-23 (train_reference.scalar_bound).  Accuracies: equal.  Update bound: derived -- the kernel forms the update in float32 and
rounds w - update once: |delta_device - delta_expected| <= 1/2 ulp_f32(w_after) + 1e-5 |delta_expected| per element; slots rtol 1e-5
(tests/test_gpu_backward.py::_assert_optimizer).  Momentum's accumulator and Adam's m are sums that cancel once the gradient turns
against the average; there float32 is good to an ulp of the larger operand only, and both bounds gain exactly that
(train_reference.rounding_slack; without it 119 % .. 524 % of the delta bound at a handful of the 2.4 million elements, steps 1 and 2).

Not held here: the refinement tower's gradients (no differentiable float64 restatement of that tower exists) and multi-replica steps.

Measured on an MI355X (worst tensor over the three steps; the bound is 3 x the float32 CPU floor of the FIRST step, which depends on
the host's float32 summation order -- 9.4e-05 .. 1.2e-04 for normal / 3DCNN on one CPU with other thread counts):
  configuration            float32 CPU floor           bound      worst device tensor, step          share of the bound
  normal, 3DCNN, rmsprop   1.16e-04 2dconv8_0 beta     3.48e-04   2dconv8_2 gamma   1.66e-04, 2      48 %  (31 %, 31 % in two other runs)
  normal, 3DCNN, momentum  1.16e-04                    3.48e-04   conv9_0 gamma     1.07e-04, 0      31 %
  normal, 3DCNN, adam      1.16e-04                    3.48e-04   conv9_0 gamma     1.07e-04, 0      31 %
  lite, 3DCNN, rmsprop     5.80e-05 2dconv0_1 beta     1.74e-04   2dconv8_2 gamma   1.30e-04, 1      75 %  (69 %, 70 %)
  normal, GRU, rmsprop     3.48e-05 2dconv3_0 gamma    1.04e-04   2dconv8_2 gamma   8.85e-05, 1      85 %  (58 %, 56 %)
(worst of three runs.)  lite and GRU use MORE THAN HALF of their bound, GRU up to 85 %: the margin is thin there.  Their floors
happen to be low -- the same lite step measured 1.7e-04 on the CPU under another thread count, and the float32 CPU run itself is
6.1e-05 = 58 % of the GRU bound at steps 1 and 2 of a CPU trajectory -- while the device's distances are those of the other
configurations.  The device is not bit-reproducible from run to run (float atomics in its reductions), RMSProp amplifies that
into different parameters at steps 1 and 2, and the worst of 125 tensors moves between 42 % and 85 % of the bound with it.
Loss: 2 % .. 66 % of its bound (3.6e-07 .. 1.1e-06 relative); depth map: 24 % .. 35 % (8 % for the winner-take-all map, where 2 .. 5 of
384 pixels are undecided and left out); accuracies equal in every step.  Update: every element within its bound, the worst at
exactly the half ulp of the final rounding; largest |delta| 1e-4 .. 4.7e-3.  Each test takes 0.6 .. 4.7 s (the first of a
configuration pays for the cached float32 floor), the file 13 s.
"""
import numpy as np
import pytest
import torch

from _helpers import tensor_distance
import train_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE_LR, STEPVALUE, GAMMA, STEPS = 1e-3, 2, 0.5, 3
ZERO_GRADIENT_ATOL = 1e-5          # prob_conv/bias, true gradient zero: what test_recurrent_regularisation_gradients_match_autograd grants
CONFIGS = [("normal", "3DCNN", "rmsprop"), ("normal", "3DCNN", "momentum"), ("normal", "3DCNN", "adam"),
           ("lite", "3DCNN", "rmsprop"), ("normal", "GRU", "rmsprop")]


def _host(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy().copy()


def _native(tr, flat, problem):
    """{variable: float32 array of the native shape} and {variable: float32 array of the padded entries} of a flat buffer."""
    shapes = {v: a.shape for v, a in R.initial_parameters(problem).items()}
    named = tr.params.named_arrays(flat)
    native, padding = {}, {}
    for var, a in named.items():
        sl = tuple(slice(0, k) for k in shapes[var])
        native[var] = a[sl].copy()
        rest = np.ones(a.shape, bool)
        rest[sl] = False
        padding[var] = a[rest]
    return native, padding


def _upload(tr, native):
    """Writes native-shape values into the device's flat parameter buffer (padded entries untouched)."""
    host = _host(tr.params.data)
    for _k, var, o, shape in tr.params.index:
        view = host[o:o + int(np.prod(shape))].reshape(shape)
        view[tuple(slice(0, k) for k in native[var].shape)] = native[var]
    with torch.no_grad():
        tr.params.data.copy_(torch.from_numpy(host))


def _trainer(mode, regularization, optimizer, **kw):
    from mvsnet_amd import train as T
    return T.Trainer(mode, DEV, optimizer=optimizer, base_lr=BASE_LR, stepvalue=STEPVALUE, gamma=GAMMA,
                     seed=R.SEED[regularization], regularization=regularization, **kw)


@pytest.mark.parametrize("mode,regularization,optimizer", CONFIGS)
def test_teacher_forced_steps_match_the_float64_oracle(mode, regularization, optimizer, lib_built):
    problem = R.step_problem(mode, regularization)
    fl = R.floor(mode, regularization)
    g_bound = R.MARGIN * fl["gradient_floor"]
    loss_bound, depth_bound = R.scalar_bound(fl["loss"]), R.scalar_bound(fl["depth"])
    tr = _trainer(mode, regularization, optimizer)
    print("\n%s %s %s: float32 CPU floor %.3e (%s), gradient bound %.3e, loss bound %.3e, depth bound %.3e" %
          (mode, regularization, optimizer, fl["gradient_floor"], max(fl["gradients"], key=fl["gradients"].get), g_bound,
           loss_bound, depth_bound))
    failures = []
    for k in range(STEPS):
        # ---- before the step: the device's state, conditioned by the oracle run
        native, padding = _native(tr, tr.params.data, problem)
        assert all(float(np.abs(p).max(initial=0.0)) == 0.0 for p in padding.values()), "padded parameters moved"
        if k == 0:
            assert all(np.array_equal(native[v], a) for v, a in R.initial_parameters(problem).items())
            r64 = fl["r64"]
        else:
            r64 = R.whole_step(native, problem, torch.float64, condition=True)
        bad = R.unsuitable(r64, fl["noise"])
        assert not bad, "inputs unsuitable at step %d: %s" % (k, bad)
        _upload(tr, r64.params)
        assert tr.global_step == k
        # ---- loss and gradient
        loss, l1, l3, depth = tr.loss(problem["images"].copy(), problem["cams"].copy(), r64.problem["gt"].copy(), problem["depth_num"])
        loss.backward()
        grad, g_pad = _native(tr, tr.params.grad, problem)
        assert all(float(np.abs(p).max(initial=0.0)) == 0.0 for p in g_pad.values()), "padded gradients are not zero"
        rows = []
        for var, ref in r64[4].items():
            if var in R.ZERO_GRADIENT:
                assert np.abs(ref).max() < 1e-12 and np.abs(grad[var]).max() <= ZERO_GRADIENT_ATOL, (var, grad[var])
            else:
                rows.append((var, tensor_distance(grad[var], ref)))
        worst = max(rows, key=lambda r: r[1])
        d_loss = abs(float(loss.detach()) - r64[0]) / abs(r64[0])
        skip = R.undecided_pixels(r64, fl["noise"])
        d_depth = tensor_distance(_host(depth)[~skip], r64[3][~skip])
        valid = float((problem["gt"] != 0).sum())
        counts = [abs(float(a.detach()) - b) * valid for a, b in ((l1, r64[1]), (l3, r64[2]))]
        print("step %d: worst gradient %s %.3e = %.0f%% of the bound; loss %.3e (%.0f%%), depth %.3e (%.0f%%), accuracies off by "
              "%.2f / %.2f pixels, %d undecided" % (k, worst[0], worst[1], 100 * worst[1] / g_bound, d_loss, 100 * d_loss / loss_bound,
                                                    d_depth, 100 * d_depth / depth_bound, counts[0], counts[1], int(skip.sum())))
        failures += [(k, var, d, g_bound) for var, d in rows if not d <= g_bound]
        if not d_loss <= loss_bound:
            failures.append((k, "loss", d_loss, loss_bound))
        if not d_depth <= depth_bound:
            failures.append((k, "depth", d_depth, depth_bound))
        failures += [(k, "accuracy", c, skip.sum()) for c in counts if not c <= skip.sum() + 0.01]
        # ---- update, from the device's own gradient
        w0, g0 = tr.params.named_arrays(tr.params.data), tr.params.named_arrays(tr.params.grad)
        w0 = {v: a.copy() for v, a in w0.items()}
        s0 = [{v: a.copy() for v, a in tr.params.named_arrays(s).items()} for s in tr.slots]
        tr.apply_gradients()
        w1 = tr.params.named_arrays(tr.params.data)
        s1 = [tr.params.named_arrays(s) for s in tr.slots]
        assert float(tr.params.grad.abs().max()) == 0.0 and tr.global_step == k + 1
        worst_u = (0.0, None)
        for var in w0:
            exp_w, exp_s, exp_t = R.optimizer_update(optimizer, w0[var], g0[var], [s[var] for s in s0], k, BASE_LR, STEPVALUE, GAMMA)
            assert exp_t == tr.global_step
            slot_slack, delta_slack = R.rounding_slack(optimizer, g0[var], [s[var] for s in s0], k, BASE_LR, STEPVALUE, GAMMA)
            err, bound = R.update_errors(w0[var], w1[var], exp_w, delta_slack)
            share = float((err / bound).max())
            worst_u = max(worst_u, (share, var))
            if not share <= 1.0:
                failures.append((k, var + " delta", share, 1.0))
            for i, e in enumerate(exp_s):
                off = np.abs(s1[i][var] - e) - (1e-5 * np.abs(e) + (slot_slack if i == 0 else 0.0))
                if not off.max() <= 0:
                    failures.append((k, "%s slot %d" % (var, i), float(off.max()), 0.0))
        moved = max(float(np.abs(w1[v].astype(np.float64) - w0[v]).max()) for v in w0)
        print("        update: worst element at %.0f%% of its bound (%s); largest |delta| %.3e, learning rate %.4e" %
              (100 * worst_u[0], worst_u[1], moved, R.exponential_decay(BASE_LR, k, STEPVALUE, GAMMA)))
        assert moved > 0
    assert not failures, failures


def test_validation_between_steps_changes_nothing(lib_built):
    """A validate_step between two training steps leaves parameters, slots and global_step bit-identical and the gradient buffer
    at zero (a gradient left over from it would enter the next update)."""
    problem = R.step_problem("normal", "3DCNN")
    args = (problem["images"].copy(), problem["cams"].copy(), problem["gt"].copy(), problem["depth_num"])
    tr = _trainer("normal", "3DCNN", "adam")
    tr.train_step(*args)
    before = [tr.params.data.clone()] + [s.clone() for s in tr.slots]
    loss, l1, l3 = tr.validate_step(*args)
    assert np.isfinite(float(loss)) and not loss.requires_grad
    assert float(tr.params.grad.abs().max()) == 0.0 and tr.global_step == 1
    assert all(torch.equal(a, b) for a, b in zip(before, [tr.params.data] + tr.slots))
    tr.train_step(*args)
    assert tr.global_step == 2 and not torch.equal(before[0], tr.params.data)


@pytest.mark.parametrize("optimizer", ["rmsprop", "momentum", "adam"])
def test_refine_only_leaves_the_main_network_and_its_slots_alone(optimizer, lib_built):
    """refine_only: the reference creates the main network's variables with trainable=False (mvsnet/train.py:312-315), so
    compute_gradients never sees them and no optimiser slot of theirs is touched.  One step: every non-refine variable is
    bit-identical and its slots are as initialised (an update over the whole buffer with zeroed gradients decays RMSProp's `rms`
    slot from 1 towards 0: 0.9 after one step); the refinement tower's variables and slots move; the gradient buffer is zero."""
    problem = R.step_problem("normal", "3DCNN")
    full = np.repeat(np.repeat(problem["gt"], 4, axis=0), 4, axis=1)
    tr = _trainer("normal", "3DCNN", optimizer, refinement=True, refinement_train_mode="refine_only")
    w0 = tr.params.named_arrays(tr.params.data)
    w0 = {v: a.copy() for v, a in w0.items()}
    tr.train_step(problem["images"].copy(), problem["cams"].copy(), problem["gt"].copy(), problem["depth_num"], full)
    w1 = tr.params.named_arrays(tr.params.data)
    s1 = [tr.params.named_arrays(s) for s in tr.slots]
    assert float(tr.params.grad.abs().max()) == 0.0 and tr.global_step == 1
    groups = set()
    for (group, _l, _f), var, _o, _shape in tr.params.index:
        groups.add(group)
        if group == "refine":
            if var.endswith("/kernel"):
                assert not np.array_equal(w1[var], w0[var]), var
                assert all(not np.array_equal(s[var], i) for s, i in zip(s1[:1], R.initial_slots(optimizer, 1)[:1])), var
        else:
            assert np.array_equal(w1[var], w0[var]), var
            for s, init in zip(s1, R.initial_slots(optimizer, 1)):
                assert np.array_equal(s[var], np.broadcast_to(init.astype(np.float32), s[var].shape)), (var, float(s[var].min()))
    assert groups == {"unet", "regnet", "refine"}
