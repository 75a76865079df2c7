"""RegNetUS0's layer table (mvsnet_amd/regnet_layers.py) and the training pass that walks it (mvsnet_amd/backward.py), without a
GPU or the library: the table and what is derived from it against literals; `regnet_forward_train` + `regnet_backward` on CPU
float64 tensors, with torch stand-ins for the six single-op wrappers they call, against float64 autograd of
`oracle.torch_grad.regnet_us0`; the sequence of wrapper calls against the lists the hand-written walk made before the table
existed; `synthetic.make_regnet_params` against digests of what it drew then.

The stand-ins know nothing of the table: F.conv3d / F.conv_transpose3d with SAME padding, and F.batch_norm's autograd for the
BatchNorm backward.  The input-gradient helpers (`conv_s1_input_grad`, `conv_s2_input_grad`, `deconv_input_grad`) are the
module's own and run on the stand-in `conv3d`, so their flip / transpose / pad logic is exercised."""
import functools
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_grad as TG
from mvsnet_amd import synthetic as S
from mvsnet_amd import backward as B
from mvsnet_amd import model as M
from mvsnet_amd import regnet_layers as R

# name, kind, (cin, cout) at 'normal' (32-channel volume, base 8), at 'lite' (16; base 4), p1, p2 as indices into this list:
# the p1 / p2 columns of NET[] in csrc/regnet.hip, -1 = the raw cost volume / none
TABLE = [
    ("3dconv1_0", "s2", (32, 16), (16, 8), -1, -1), ("3dconv2_0", "s2", (16, 32), (8, 16), 0, -1),
    ("3dconv3_0", "s2", (32, 64), (16, 32), 1, -1), ("3dconv0_1", "s1", (32, 8), (16, 4), -1, -1),
    ("3dconv1_1", "s1", (16, 16), (8, 8), 0, -1), ("3dconv2_1", "s1", (32, 32), (16, 16), 1, -1),
    ("3dconv3_1", "s1", (64, 64), (32, 32), 2, -1), ("3dconv4_0", "up", (64, 32), (32, 16), 6, -1),
    ("3dconv5_0", "up", (32, 16), (16, 8), 7, 5), ("3dconv6_0", "up", (16, 8), (8, 4), 8, 4),
    ("3dconv6_2", "s1", (8, 1), (4, 1), 9, 3),
]
CONSUMERS = {
    None: ("3dconv1_0", "3dconv0_1"), "3dconv1_0": ("3dconv2_0", "3dconv1_1"), "3dconv2_0": ("3dconv3_0", "3dconv2_1"),
    "3dconv3_0": ("3dconv3_1",), "3dconv0_1": ("3dconv6_2",), "3dconv1_1": ("3dconv6_0",), "3dconv2_1": ("3dconv5_0",),
    "3dconv3_1": ("3dconv4_0",), "3dconv4_0": ("3dconv5_0",), "3dconv5_0": ("3dconv6_0",), "3dconv6_0": ("3dconv6_2",),
    "3dconv6_2": (),
}
# name -> the input-gradient helper, (gradient is conv3d_wgrad's first operand, stride), weight gradient mirrored
BACKWARD = {
    "3dconv1_0": ("conv_s2_input_grad", (False, 2), False), "3dconv2_0": ("conv_s2_input_grad", (False, 2), False),
    "3dconv3_0": ("conv_s2_input_grad", (False, 2), False), "3dconv0_1": ("conv_s1_input_grad", (True, 1), True),
    "3dconv1_1": ("conv_s1_input_grad", (False, 1), False), "3dconv2_1": ("conv_s1_input_grad", (False, 1), False),
    "3dconv3_1": ("conv_s1_input_grad", (False, 1), False), "3dconv4_0": ("deconv_input_grad", (True, 2), False),
    "3dconv5_0": ("deconv_input_grad", (True, 2), False), "3dconv6_0": ("deconv_input_grad", (True, 2), False),
    "3dconv6_2": ("conv_s1_input_grad", (False, 1), False),
}
BACKWARD_ORDER = ("3dconv6_2", "3dconv6_0", "3dconv0_1", "3dconv5_0", "3dconv1_1", "3dconv4_0", "3dconv2_1", "3dconv3_1",
                  "3dconv3_0", "3dconv2_0", "3dconv1_0")
# what flatten_params returned when it walked REGNET_ORDER itself
SLOTS = [(name, key) for name, *_ in TABLE for key in (("w", "gamma", "beta") if name != "3dconv6_2" else ("w",))]
# sha256 over every array of make_regnet_params(mode, random_affine=...) (name, key, dtype, shape, bytes; in the dict's order),
# taken when the function carried its own list of the layers
DIGESTS = {
    ("normal", False): "084f730ab0faf09a355b5454af0370fd87af2024791893379b9f11751a0d9f9c",
    ("normal", True): "682e5cddf400af4bfecd31d226a3bcf65a606a5868bf79f35dfc0c3eb6f5c890",
    ("lite", False): "009c03b283d59ab45d3b42fc0388f4813969c0768d1a0df8e73d07a6a99c4ffe",
    ("lite", True): "d058e2db289427c4593488fda451838cecc3a0a6398da8b74e3a61cd8fcdaf71",
    ("ultralite", False): "528ea6ae6a8e376bd2a78b0a17ad64aa231e6f2339459ead2d5457fa634418fd",
    ("ultralite", True): "b0c45af7010103b9e69d2a01de2aba2db01ee85d380009b577e25847c12bdc80",
}


# ---- the table against literals ------------------------------------------------------------------------------------------

def test_the_table_against_literals():
    names = [row[0] for row in TABLE]
    assert [(l.name, l.kind) for l in R.REGNET_LAYERS] == [row[:2] for row in TABLE]
    assert [l.channels(32, 8) for l in R.REGNET_LAYERS] == [row[2] for row in TABLE]
    assert [l.channels(16, 4) for l in R.REGNET_LAYERS] == [row[3] for row in TABLE]
    at = lambda name: -1 if name is None else names.index(name)
    assert [(at(l.p1), at(l.p2)) for l in R.REGNET_LAYERS] == [row[4:] for row in TABLE]
    assert [l.bn for l in R.REGNET_LAYERS] == [True] * 10 + [False]
    assert R.REGNET_ORDER == M.REGNET_ORDER == tuple(names) and B.BN_LAYERS == R.BN_LAYERS == tuple(names[:-1])
    assert R.REGNET_CONSUMERS == CONSUMERS
    assert R.REGNET_PAIR == ("3dconv0_1", "3dconv1_0")          # the order of conv3d_pair's operands and of the returned gradients


def test_routes_and_weight_gradient_operands():
    for l in R.REGNET_LAYERS:
        route, wgrad, mirrored = BACKWARD[l.name]
        assert B.INPUT_GRAD[l.kind] is getattr(B, route)
        assert ((l.wgrad_gradient_first, l.stride), l.wgrad_mirrored) == (wgrad, mirrored)


def test_the_backward_order_puts_consumers_first():
    assert R.REGNET_BACKWARD_ORDER == BACKWARD_ORDER and R.backward_order_is_valid()
    at = {name: i for i, name in enumerate(BACKWARD_ORDER)}
    assert all(at[c] < at[name] for name, readers in CONSUMERS.items() if name for c in readers)
    assert not R.backward_order_is_valid(tuple(reversed(BACKWARD_ORDER)))
    assert not R.backward_order_is_valid(BACKWARD_ORDER[1:])
    swapped = list(BACKWARD_ORDER)
    swapped[3], swapped[5] = swapped[5], swapped[3]               # 4_0 ahead of its consumer 5_0
    assert not R.backward_order_is_valid(tuple(swapped))


def test_the_slots_and_their_round_trip():
    assert list(R.REGNET_SLOTS) == SLOTS and len(SLOTS) == 31
    p = {name: {key: "%s/%s" % (name, key) for key in ("w", "gamma", "beta")[:3 if name != "3dconv6_2" else 1]} for name, *_ in TABLE}
    flat = B.flatten_params(p)
    assert flat == ["%s/%s" % slot for slot in SLOTS]
    assert B.unflatten_params(flat) == p
    assert [list(q) for q in B.unflatten_params(flat).values()] == [list(q) for q in p.values()]


@pytest.mark.parametrize("mode,random_affine", sorted(DIGESTS))
def test_make_regnet_params_draws_what_it_drew(mode, random_affine):
    params = S.make_regnet_params(mode, random_affine=random_affine)
    h = hashlib.sha256()
    for name, q in params.items():
        for key, a in q.items():
            h.update(("%s:%s:%s:%s" % (name, key, a.dtype, a.shape)).encode())
            h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == DIGESTS[(mode, random_affine)]
    base = S.base_filter(mode)
    assert {n: tuple(q["w"].shape) for n, q in params.items()} == {l.name: l.w_shape(*l.channels(4 * base, base)) for l in R.REGNET_LAYERS}


# ---- the walk on CPU float64 tensors ---------------------------------------------------------------------------------------

def _ncdhw(x):
    return x.permute(3, 0, 1, 2)[None]


def _same(x, stride):
    """TensorFlow's SAME padding of a 3-tap kernel: the odd element goes behind."""
    pads = []
    for n in reversed(x.shape[-3:]):
        total = max((-(-n // stride) - 1) * stride + 3 - n, 0)
        pads += [total // 2, total - total // 2]
    return F.pad(x, pads)


def _conv(x, w, stride):
    return F.conv3d(_same(_ncdhw(x), stride), w.permute(4, 3, 0, 1, 2), stride=stride)[0].permute(1, 2, 3, 0)


def _deconv(x, w):
    D, H, W, _ = x.shape
    return F.conv_transpose3d(_ncdhw(x), w.permute(4, 3, 0, 1, 2), stride=2)[0, :, :2 * D, :2 * H, :2 * W].permute(1, 2, 3, 0)


def _act(y, affine):
    return y if affine is None else F.relu(y * affine[0] + affine[1])


class _Lib:
    """Stands in for the library where only the slab's slot count is asked."""

    def mvs_bn_bwd_sum_slots(self):
        return 8


class StandIns:
    """The six wrappers on CPU tensors.  Every call is recorded as (op, operand names, operand shapes, further arguments): an
    operand is named after the tensor handed in ("cost", "w:3dconv1_0"), after the call that made it ("#3", "#0.1" for the second
    output of call 0), or "?" where the walk derived it itself (a mirrored kernel, a zero-padded gradient)."""
    OPS = ("conv3d", "conv3d_pair", "bn_finalize", "bn_relu", "bn_relu_bwd", "conv3d_wgrad")

    def __init__(self, named):
        self.calls, self.keep, self.names = [], [], {}           # `keep` holds every named tensor, so that no address comes twice
        for label, t in named.items():
            self._name(t, label)

    def _name(self, t, label):
        self.keep.append(t)
        self.names[t.data_ptr()] = label

    def _record(self, op, operands, extra, outs):
        k = len(self.calls)
        self.calls.append((op, tuple(None if t is None else self.names.get(t.data_ptr(), "?") for t in operands),
                           tuple(tuple(t.shape) for t in operands if t is not None)) + extra)
        outs = [o.contiguous() for o in outs]
        for i, o in enumerate(outs):
            self._name(o, "#%d" % k if len(outs) == 1 else "#%d.%d" % (k, i))
        return outs

    @staticmethod
    def _sums(stats, y):
        if stats is not None:
            flat = y.reshape(-1, y.shape[-1])
            stats += torch.stack([flat.sum(0), (flat * flat).sum(0)])

    def conv3d(self, x, w, stride=1, x_affine=None, skip=None, skip_affine=None, stats=None, transpose=False):
        a = _act(x, x_affine) + (_act(skip, skip_affine) if skip is not None else 0)
        y, = self._record("conv3d", (x, w, skip), ("transpose" if transpose else stride, x_affine is not None, stats is not None),
                          [_deconv(a, w) if transpose else _conv(a, w, stride)])
        self._sums(stats, y)
        return y

    def conv3d_pair(self, x, w1, w2, stats1=None, stats2=None):
        y1, y2 = self._record("conv3d_pair", (x, w1, w2), (stats1 is not None, stats2 is not None), [_conv(x, w1, 1), _conv(x, w2, 2)])
        self._sums(stats1, y1)
        self._sums(stats2, y2)
        return y1, y2

    def bn_finalize(self, stats, count, gamma, beta, eps=1e-5):
        mean = stats[0] / count
        scale = gamma / torch.sqrt(stats[1] / count - mean * mean + eps)
        return tuple(self._record("bn_finalize", (gamma, beta), (int(count),), [scale, beta - mean * scale]))

    def bn_relu(self, y, affine=None, y2=None, affine2=None):
        return self._record("bn_relu", (y, y2), (), [_act(y, affine) + (_act(y2, affine2) if y2 is not None else 0)])[0]

    def bn_relu_bwd(self, y, stats, affine, gamma, g1, g2=None, eps=1e-5, sync=None, sums=None):
        yl, gl, bl = (t.detach().clone().requires_grad_(True) for t in (y, gamma, torch.zeros_like(gamma)))
        beta = affine[1] + affine[0] * stats[0] * y.shape[-1] / y.numel()         # shift = beta - mean * scale
        F.relu(F.batch_norm(_ncdhw(yl), None, None, gl, bl + beta, training=True, eps=eps)).backward(_ncdhw(g1 if g2 is None else g1 + g2))
        return tuple(self._record("bn_relu_bwd", (y, gamma, g1, g2), (sums is not None,), [yl.grad, gl.grad, bl.grad]))

    def conv3d_wgrad(self, big, small, stride):
        w = torch.zeros((3, 3, 3, big.shape[-1], small.shape[-1]), dtype=big.dtype, requires_grad=True)
        (_conv(big, w, stride) * small).sum().backward()            # linear in w: the gradient at any w
        return self._record("conv3d_wgrad", (big, small), (stride,), [w.grad])[0]


@functools.lru_cache(maxsize=None)
def walk(mode, D, H, W):
    """One forward + backward of the walk and of the oracle: (the calls, {array: max-norm relative distance}).  Computed once per
    case and shared by the tests; nothing of it is changed afterwards."""
    params = S.make_regnet_params(mode, seed=5, random_affine=True)
    rs = np.random.RandomState(6)
    cost = torch.tensor(rs.standard_normal((D, H, W, params["3dconv1_0"]["w"].shape[3])) ** 2)        # a variance: not negative
    g_reg = torch.tensor(rs.standard_normal((D, H, W)))
    p = {n: {k: torch.tensor(np.asarray(a, np.float64)) for k, a in q.items()} for n, q in params.items()}
    stand = StandIns(dict({"cost": cost, "g_reg": g_reg}, **{"%s:%s" % (k, n): t for n, q in p.items() for k, t in q.items()}))
    with pytest.MonkeyPatch.context() as mp:
        for op in StandIns.OPS:
            mp.setattr(B, op, getattr(stand, op))
        mp.setattr(B._lib, "load", lambda: _Lib())
        reg, saved = B.regnet_forward_train(cost, p)
        G, g_cost_a, g_cost_b = B.regnet_backward(saved, p, g_reg)
    po = {n: {k: t.clone().requires_grad_(True) for k, t in q.items()} for n, q in p.items()}
    co = cost.permute(3, 0, 1, 2).clone().requires_grad_(True)
    ro = TG.regnet_us0(co, po)
    (ro * g_reg).sum().backward()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert sorted(G) == sorted(po) and all(sorted(G[n]) == sorted(po[n]) for n in po)
    dist = {"reg": rel(reg, ro.detach()), "g_cost_a + g_cost_b": rel(g_cost_a + g_cost_b, co.grad.permute(1, 2, 3, 0))}
    dist.update({"%s:%s" % (k, n): rel(G[n][k], t.grad) for n, q in po.items() for k, t in q.items()})
    return stand.calls, dist


CASES = [("normal", 8, 8, 16), ("normal", 16, 8, 24), ("lite", 8, 8, 16)]


@pytest.mark.parametrize("case", CASES, ids=["fused-8x8x16", "fused-16x8x24", "unfused-8x8x16"])
def test_the_walk_matches_float64_autograd(case):
    """Every parameter gradient, the cost volume's and the forward value, 1e-10 max-norm relative per array: both sides are
    float64 (the walk measures 4.5e-14, 7.4e-15 and 1.9e-13 on the three cases); a wrong route, operand order or producer gives an
    error of order one.  At (8,8,16) the coarsest level is 1 x 1 x 2, the smallest at which all three stride-2 steps exist."""
    _calls, dist = walk(*case)
    assert len(dist) == 2 + 31
    print({k: "%.1e" % v for k, v in dist.items()})
    assert max(dist.values()) < 1e-10, max(dist, key=dist.get)


def test_the_call_sequence_of_the_fused_pass():
    calls, _ = walk(*CASES[0])
    # the pair, 10 forward convs + 10 input gradients, 7 recomputed activations, 10 BatchNorm backwards, 11 weight gradients
    assert [sum(c[0] == op for c in calls) for op in StandIns.OPS] == [20, 1, 10, 7, 10, 11]
    assert calls == FUSED_CALLS


def test_the_call_sequence_of_the_unfused_pass():
    calls, _ = walk(*CASES[2])
    assert [sum(c[0] == op for c in calls) for op in StandIns.OPS] == [22, 0, 10, 7, 10, 11]
    assert calls == UNFUSED_CALLS


# What the hand-written walk called, in order, at (8,8,16): 32 channels, base 8 (the fused first pass) and 16 channels, base 4.
# conv3d: (x, w, skip), then stride or "transpose", whether x carries an affine, whether sums are taken; bn_finalize: the count;
# bn_relu_bwd: (y, gamma, g1, g2), whether it got a piece of the slab; conv3d_wgrad: (big, small), stride.
FUSED_CALLS = [
    ('conv3d_pair', ('cost', 'w:3dconv0_1', 'w:3dconv1_0'), ((8, 8, 16, 32), (3, 3, 3, 32, 8), (3, 3, 3, 32, 16)), True, True),
    ('bn_finalize', ('gamma:3dconv0_1', 'beta:3dconv0_1'), ((8,), (8,)), 1024),
    ('bn_finalize', ('gamma:3dconv1_0', 'beta:3dconv1_0'), ((16,), (16,)), 128),
    ('conv3d', ('#0.1', 'w:3dconv2_0', None), ((4, 4, 8, 16), (3, 3, 3, 16, 32)), 2, True, True),
    ('bn_finalize', ('gamma:3dconv2_0', 'beta:3dconv2_0'), ((32,), (32,)), 16),
    ('conv3d', ('#3', 'w:3dconv3_0', None), ((2, 2, 4, 32), (3, 3, 3, 32, 64)), 2, True, True),
    ('bn_finalize', ('gamma:3dconv3_0', 'beta:3dconv3_0'), ((64,), (64,)), 2),
    ('conv3d', ('#0.1', 'w:3dconv1_1', None), ((4, 4, 8, 16), (3, 3, 3, 16, 16)), 1, True, True),
    ('bn_finalize', ('gamma:3dconv1_1', 'beta:3dconv1_1'), ((16,), (16,)), 128),
    ('conv3d', ('#3', 'w:3dconv2_1', None), ((2, 2, 4, 32), (3, 3, 3, 32, 32)), 1, True, True),
    ('bn_finalize', ('gamma:3dconv2_1', 'beta:3dconv2_1'), ((32,), (32,)), 16),
    ('conv3d', ('#5', 'w:3dconv3_1', None), ((1, 1, 2, 64), (3, 3, 3, 64, 64)), 1, True, True),
    ('bn_finalize', ('gamma:3dconv3_1', 'beta:3dconv3_1'), ((64,), (64,)), 2),
    ('conv3d', ('#11', 'w:3dconv4_0', None), ((1, 1, 2, 64), (3, 3, 3, 32, 64)), 'transpose', True, True),
    ('bn_finalize', ('gamma:3dconv4_0', 'beta:3dconv4_0'), ((32,), (32,)), 16),
    ('conv3d', ('#13', 'w:3dconv5_0', '#9'), ((2, 2, 4, 32), (3, 3, 3, 16, 32), (2, 2, 4, 32)), 'transpose', True, True),
    ('bn_finalize', ('gamma:3dconv5_0', 'beta:3dconv5_0'), ((16,), (16,)), 128),
    ('conv3d', ('#15', 'w:3dconv6_0', '#7'), ((4, 4, 8, 16), (3, 3, 3, 8, 16), (4, 4, 8, 16)), 'transpose', True, True),
    ('bn_finalize', ('gamma:3dconv6_0', 'beta:3dconv6_0'), ((8,), (8,)), 1024),
    ('conv3d', ('#17', 'w:3dconv6_2', '#0.0'), ((8, 8, 16, 8), (3, 3, 3, 8, 1), (8, 8, 16, 8)), 1, True, False),
    ('bn_relu', ('#17', '#0.0'), ((8, 8, 16, 8), (8, 8, 16, 8))),
    ('conv3d_wgrad', ('#20', 'g_reg'), ((8, 8, 16, 8), (8, 8, 16, 1)), 1),
    ('conv3d', ('g_reg', '?', None), ((8, 8, 16, 1), (3, 3, 3, 1, 8)), 1, False, False),
    ('bn_relu_bwd', ('#17', 'gamma:3dconv6_0', '#22', None), ((8, 8, 16, 8), (8,), (8, 8, 16, 8)), True),
    ('bn_relu', ('#15', '#7'), ((4, 4, 8, 16), (4, 4, 8, 16))),
    ('conv3d_wgrad', ('#23.0', '#24'), ((8, 8, 16, 8), (4, 4, 8, 16)), 2),
    ('conv3d', ('?', '?', None), ((8, 8, 16, 16), (3, 3, 3, 16, 16)), 2, False, False),
    ('bn_relu_bwd', ('#0.0', 'gamma:3dconv0_1', '#22', None), ((8, 8, 16, 8), (8,), (8, 8, 16, 8)), True),
    ('conv3d_wgrad', ('#27.0', 'cost'), ((8, 8, 16, 8), (8, 8, 16, 32)), 1),
    ('conv3d', ('#27.0', '?', None), ((8, 8, 16, 8), (3, 3, 3, 8, 32)), 1, False, False),
    ('bn_relu_bwd', ('#15', 'gamma:3dconv5_0', '#26', None), ((4, 4, 8, 16), (16,), (4, 4, 8, 16)), True),
    ('bn_relu', ('#13', '#9'), ((2, 2, 4, 32), (2, 2, 4, 32))),
    ('conv3d_wgrad', ('#30.0', '#31'), ((4, 4, 8, 16), (2, 2, 4, 32)), 2),
    ('conv3d', ('#30.0', 'w:3dconv5_0', None), ((4, 4, 8, 16), (3, 3, 3, 16, 32)), 2, False, False),
    ('bn_relu', ('#0.1', None), ((4, 4, 8, 16),)),
    ('bn_relu_bwd', ('#7', 'gamma:3dconv1_1', '#26', None), ((4, 4, 8, 16), (16,), (4, 4, 8, 16)), True),
    ('conv3d_wgrad', ('#34', '#35.0'), ((4, 4, 8, 16), (4, 4, 8, 16)), 1),
    ('conv3d', ('#35.0', '?', None), ((4, 4, 8, 16), (3, 3, 3, 16, 16)), 1, False, False),
    ('bn_relu_bwd', ('#13', 'gamma:3dconv4_0', '#33', None), ((2, 2, 4, 32), (32,), (2, 2, 4, 32)), True),
    ('bn_relu', ('#11', None), ((1, 1, 2, 64),)),
    ('conv3d_wgrad', ('#38.0', '#39'), ((2, 2, 4, 32), (1, 1, 2, 64)), 2),
    ('conv3d', ('#38.0', 'w:3dconv4_0', None), ((2, 2, 4, 32), (3, 3, 3, 32, 64)), 2, False, False),
    ('bn_relu', ('#3', None), ((2, 2, 4, 32),)),
    ('bn_relu_bwd', ('#9', 'gamma:3dconv2_1', '#33', None), ((2, 2, 4, 32), (32,), (2, 2, 4, 32)), True),
    ('conv3d_wgrad', ('#42', '#43.0'), ((2, 2, 4, 32), (2, 2, 4, 32)), 1),
    ('conv3d', ('#43.0', '?', None), ((2, 2, 4, 32), (3, 3, 3, 32, 32)), 1, False, False),
    ('bn_relu_bwd', ('#11', 'gamma:3dconv3_1', '#41', None), ((1, 1, 2, 64), (64,), (1, 1, 2, 64)), True),
    ('bn_relu', ('#5', None), ((1, 1, 2, 64),)),
    ('conv3d_wgrad', ('#47', '#46.0'), ((1, 1, 2, 64), (1, 1, 2, 64)), 1),
    ('conv3d', ('#46.0', '?', None), ((1, 1, 2, 64), (3, 3, 3, 64, 64)), 1, False, False),
    ('bn_relu_bwd', ('#5', 'gamma:3dconv3_0', '#49', None), ((1, 1, 2, 64), (64,), (1, 1, 2, 64)), True),
    ('conv3d_wgrad', ('#42', '#50.0'), ((2, 2, 4, 32), (1, 1, 2, 64)), 2),
    ('conv3d', ('#50.0', 'w:3dconv3_0', None), ((1, 1, 2, 64), (3, 3, 3, 32, 64)), 'transpose', False, False),
    ('bn_relu_bwd', ('#3', 'gamma:3dconv2_0', '#52', '#45'), ((2, 2, 4, 32), (32,), (2, 2, 4, 32), (2, 2, 4, 32)), True),
    ('conv3d_wgrad', ('#34', '#53.0'), ((4, 4, 8, 16), (2, 2, 4, 32)), 2),
    ('conv3d', ('#53.0', 'w:3dconv2_0', None), ((2, 2, 4, 32), (3, 3, 3, 16, 32)), 'transpose', False, False),
    ('bn_relu_bwd', ('#0.1', 'gamma:3dconv1_0', '#55', '#37'), ((4, 4, 8, 16), (16,), (4, 4, 8, 16), (4, 4, 8, 16)), True),
    ('conv3d_wgrad', ('cost', '#56.0'), ((8, 8, 16, 32), (4, 4, 8, 16)), 2),
    ('conv3d', ('#56.0', 'w:3dconv1_0', None), ((4, 4, 8, 16), (3, 3, 3, 32, 16)), 'transpose', False, False),
]
UNFUSED_CALLS = [
    ('conv3d', ('cost', 'w:3dconv1_0', None), ((8, 8, 16, 16), (3, 3, 3, 16, 8)), 2, False, True),
    ('bn_finalize', ('gamma:3dconv1_0', 'beta:3dconv1_0'), ((8,), (8,)), 128),
    ('conv3d', ('#0', 'w:3dconv2_0', None), ((4, 4, 8, 8), (3, 3, 3, 8, 16)), 2, True, True),
    ('bn_finalize', ('gamma:3dconv2_0', 'beta:3dconv2_0'), ((16,), (16,)), 16),
    ('conv3d', ('#2', 'w:3dconv3_0', None), ((2, 2, 4, 16), (3, 3, 3, 16, 32)), 2, True, True),
    ('bn_finalize', ('gamma:3dconv3_0', 'beta:3dconv3_0'), ((32,), (32,)), 2),
    ('conv3d', ('cost', 'w:3dconv0_1', None), ((8, 8, 16, 16), (3, 3, 3, 16, 4)), 1, False, True),
    ('bn_finalize', ('gamma:3dconv0_1', 'beta:3dconv0_1'), ((4,), (4,)), 1024),
    ('conv3d', ('#0', 'w:3dconv1_1', None), ((4, 4, 8, 8), (3, 3, 3, 8, 8)), 1, True, True),
    ('bn_finalize', ('gamma:3dconv1_1', 'beta:3dconv1_1'), ((8,), (8,)), 128),
    ('conv3d', ('#2', 'w:3dconv2_1', None), ((2, 2, 4, 16), (3, 3, 3, 16, 16)), 1, True, True),
    ('bn_finalize', ('gamma:3dconv2_1', 'beta:3dconv2_1'), ((16,), (16,)), 16),
    ('conv3d', ('#4', 'w:3dconv3_1', None), ((1, 1, 2, 32), (3, 3, 3, 32, 32)), 1, True, True),
    ('bn_finalize', ('gamma:3dconv3_1', 'beta:3dconv3_1'), ((32,), (32,)), 2),
    ('conv3d', ('#12', 'w:3dconv4_0', None), ((1, 1, 2, 32), (3, 3, 3, 16, 32)), 'transpose', True, True),
    ('bn_finalize', ('gamma:3dconv4_0', 'beta:3dconv4_0'), ((16,), (16,)), 16),
    ('conv3d', ('#14', 'w:3dconv5_0', '#10'), ((2, 2, 4, 16), (3, 3, 3, 8, 16), (2, 2, 4, 16)), 'transpose', True, True),
    ('bn_finalize', ('gamma:3dconv5_0', 'beta:3dconv5_0'), ((8,), (8,)), 128),
    ('conv3d', ('#16', 'w:3dconv6_0', '#8'), ((4, 4, 8, 8), (3, 3, 3, 4, 8), (4, 4, 8, 8)), 'transpose', True, True),
    ('bn_finalize', ('gamma:3dconv6_0', 'beta:3dconv6_0'), ((4,), (4,)), 1024),
    ('conv3d', ('#18', 'w:3dconv6_2', '#6'), ((8, 8, 16, 4), (3, 3, 3, 4, 1), (8, 8, 16, 4)), 1, True, False),
    ('bn_relu', ('#18', '#6'), ((8, 8, 16, 4), (8, 8, 16, 4))),
    ('conv3d_wgrad', ('#21', 'g_reg'), ((8, 8, 16, 4), (8, 8, 16, 1)), 1),
    ('conv3d', ('g_reg', '?', None), ((8, 8, 16, 1), (3, 3, 3, 1, 4)), 1, False, False),
    ('bn_relu_bwd', ('#18', 'gamma:3dconv6_0', '#23', None), ((8, 8, 16, 4), (4,), (8, 8, 16, 4)), True),
    ('bn_relu', ('#16', '#8'), ((4, 4, 8, 8), (4, 4, 8, 8))),
    ('conv3d_wgrad', ('#24.0', '#25'), ((8, 8, 16, 4), (4, 4, 8, 8)), 2),
    ('conv3d', ('#24.0', 'w:3dconv6_0', None), ((8, 8, 16, 4), (3, 3, 3, 4, 8)), 2, False, False),
    ('bn_relu_bwd', ('#6', 'gamma:3dconv0_1', '#23', None), ((8, 8, 16, 4), (4,), (8, 8, 16, 4)), True),
    ('conv3d_wgrad', ('#28.0', 'cost'), ((8, 8, 16, 4), (8, 8, 16, 16)), 1),
    ('conv3d', ('#28.0', '?', None), ((8, 8, 16, 4), (3, 3, 3, 4, 16)), 1, False, False),
    ('bn_relu_bwd', ('#16', 'gamma:3dconv5_0', '#27', None), ((4, 4, 8, 8), (8,), (4, 4, 8, 8)), True),
    ('bn_relu', ('#14', '#10'), ((2, 2, 4, 16), (2, 2, 4, 16))),
    ('conv3d_wgrad', ('#31.0', '#32'), ((4, 4, 8, 8), (2, 2, 4, 16)), 2),
    ('conv3d', ('?', '?', None), ((4, 4, 8, 16), (3, 3, 3, 16, 16)), 2, False, False),
    ('bn_relu', ('#0', None), ((4, 4, 8, 8),)),
    ('bn_relu_bwd', ('#8', 'gamma:3dconv1_1', '#27', None), ((4, 4, 8, 8), (8,), (4, 4, 8, 8)), True),
    ('conv3d_wgrad', ('#35', '#36.0'), ((4, 4, 8, 8), (4, 4, 8, 8)), 1),
    ('conv3d', ('?', '?', None), ((4, 4, 8, 16), (3, 3, 3, 16, 8)), 1, False, False),
    ('bn_relu_bwd', ('#14', 'gamma:3dconv4_0', '#34', None), ((2, 2, 4, 16), (16,), (2, 2, 4, 16)), True),
    ('bn_relu', ('#12', None), ((1, 1, 2, 32),)),
    ('conv3d_wgrad', ('#39.0', '#40'), ((2, 2, 4, 16), (1, 1, 2, 32)), 2),
    ('conv3d', ('#39.0', 'w:3dconv4_0', None), ((2, 2, 4, 16), (3, 3, 3, 16, 32)), 2, False, False),
    ('bn_relu', ('#2', None), ((2, 2, 4, 16),)),
    ('bn_relu_bwd', ('#10', 'gamma:3dconv2_1', '#34', None), ((2, 2, 4, 16), (16,), (2, 2, 4, 16)), True),
    ('conv3d_wgrad', ('#43', '#44.0'), ((2, 2, 4, 16), (2, 2, 4, 16)), 1),
    ('conv3d', ('#44.0', '?', None), ((2, 2, 4, 16), (3, 3, 3, 16, 16)), 1, False, False),
    ('bn_relu_bwd', ('#12', 'gamma:3dconv3_1', '#42', None), ((1, 1, 2, 32), (32,), (1, 1, 2, 32)), True),
    ('bn_relu', ('#4', None), ((1, 1, 2, 32),)),
    ('conv3d_wgrad', ('#48', '#47.0'), ((1, 1, 2, 32), (1, 1, 2, 32)), 1),
    ('conv3d', ('#47.0', '?', None), ((1, 1, 2, 32), (3, 3, 3, 32, 32)), 1, False, False),
    ('bn_relu_bwd', ('#4', 'gamma:3dconv3_0', '#50', None), ((1, 1, 2, 32), (32,), (1, 1, 2, 32)), True),
    ('conv3d_wgrad', ('#43', '#51.0'), ((2, 2, 4, 16), (1, 1, 2, 32)), 2),
    ('conv3d', ('#51.0', 'w:3dconv3_0', None), ((1, 1, 2, 32), (3, 3, 3, 16, 32)), 'transpose', False, False),
    ('bn_relu_bwd', ('#2', 'gamma:3dconv2_0', '#53', '#46'), ((2, 2, 4, 16), (16,), (2, 2, 4, 16), (2, 2, 4, 16)), True),
    ('conv3d_wgrad', ('#35', '#54.0'), ((4, 4, 8, 8), (2, 2, 4, 16)), 2),
    ('conv3d', ('#54.0', 'w:3dconv2_0', None), ((2, 2, 4, 16), (3, 3, 3, 8, 16)), 'transpose', False, False),
    ('bn_relu_bwd', ('#0', 'gamma:3dconv1_0', '#56', '#38'), ((4, 4, 8, 8), (8,), (4, 4, 8, 8), (4, 4, 8, 8)), True),
    ('conv3d_wgrad', ('cost', '#57.0'), ((8, 8, 16, 16), (4, 4, 8, 8)), 2),
    ('conv3d', ('#57.0', 'w:3dconv1_0', None), ((4, 4, 8, 8), (3, 3, 3, 16, 8)), 'transpose', False, False),
]
