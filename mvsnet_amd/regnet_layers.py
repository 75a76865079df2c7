"""The layer table of RegNetUS0 (mvsnet/cnn_wrapper/mvsnetworks.py:122-158) for the host code: the rows of `NET[]` in
csrc/regnet.hip with the layers' names.  The order of the weights arrays, the BatchNorm layers, the variables' flat order, every
layer's consumers and the order of the backward pass are derived from it here, once; synthetic.make_regnet_params,
model.RegNetWeights and the training pass (backward.py) read them.  No imports from the package: synthetic stays numpy-only.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

S1, S2, UP = "s1", "s2", "up"        # 3x3x3 SAME conv of stride 1, of stride 2, transposed conv of stride 2
COST = ONE = 0                       # ci: the cost volume's channels;  co: the single output channel


class RegNetLayer(NamedTuple):
    """`ci`, `co`: channels in multiples of the base filter count (or COST / ONE); `p1`, `p2`: the producers, the layer reads
    BN+ReLU(p1) [+ BN+ReLU(p2)], None = the raw cost volume / no second one; `bn`: BatchNorm + ReLU behind the conv."""
    name: str
    kind: str
    ci: int
    co: int
    p1: Optional[str]
    p2: Optional[str]
    bn: bool = True

    @property
    def srcs(self):
        return tuple(s_ for s_ in (self.p1, self.p2) if s_ is not None)

    @property
    def stride(self):
        return 1 if self.kind == S1 else 2

    @property
    def keys(self):
        """The layer's variables in the order trainers flatten them."""
        return ("w", "gamma", "beta") if self.bn else ("w",)

    @property
    def wgrad_mirrored(self):
        """The stride-1 conv on the raw cost volume: its weight gradient is taken with the operands' roles swapped and comes out
        mirrored and transposed (backward.regnet_backward)."""
        return self.kind == S1 and self.p1 is None

    @property
    def wgrad_gradient_first(self):
        """conv3d_wgrad(big, small, stride): `big` is the finer volume -- a transposed layer's output gradient, else the input."""
        return self.kind == UP or self.wgrad_mirrored

    def channels(self, cost_channels, base):
        return self.ci * base or cost_channels, self.co * base or 1

    def w_shape(self, cin, cout):
        """TensorFlow variable layouts: conv (3,3,3,Cin,Cout), transposed conv (3,3,3,Cout,Cin)."""
        return (3, 3, 3, cout, cin) if self.kind == UP else (3, 3, 3, cin, cout)

    def cout_of(self, w):
        return w.shape[3 if self.kind == UP else 4]


REGNET_LAYERS = (
    # encoder (mvsnetworks.py:130-136)
    RegNetLayer("3dconv1_0", S2, COST, 2, None, None),
    RegNetLayer("3dconv2_0", S2, 2, 4, "3dconv1_0", None),
    RegNetLayer("3dconv3_0", S2, 4, 8, "3dconv2_0", None),
    # same-resolution branches, only needed by the decoder (mvsnetworks.py:138-141)
    RegNetLayer("3dconv0_1", S1, COST, 1, None, None),
    RegNetLayer("3dconv1_1", S1, 2, 2, "3dconv1_0", None),
    RegNetLayer("3dconv2_1", S1, 4, 4, "3dconv2_0", None),
    RegNetLayer("3dconv3_1", S1, 8, 8, "3dconv3_0", None),
    # decoder with additive skips (mvsnetworks.py:146-157)
    RegNetLayer("3dconv4_0", UP, 8, 4, "3dconv3_1", None),
    RegNetLayer("3dconv5_0", UP, 4, 2, "3dconv4_0", "3dconv2_1"),
    RegNetLayer("3dconv6_0", UP, 2, 1, "3dconv5_0", "3dconv1_1"),
    # output conv, no BN / ReLU / bias (mvsnetworks.py:158)
    RegNetLayer("3dconv6_2", S1, 1, ONE, "3dconv6_0", "3dconv0_1", bn=False),
)
REGNET_LAYER = {l.name: l for l in REGNET_LAYERS}
REGNET_ORDER = tuple(REGNET_LAYER)                                              # order of the weights arrays
BN_LAYERS = tuple(l.name for l in REGNET_LAYERS if l.bn)
REGNET_SLOTS = tuple((l.name, key) for l in REGNET_LAYERS for key in l.keys)    # the variables, (layer, key), in flat order
# who reads a layer's activation, in the order of the table; under None: the readers of the raw cost volume
REGNET_CONSUMERS = {n: tuple(l.name for l in REGNET_LAYERS if n in (l.srcs or (None,))) for n in (None,) + REGNET_ORDER}
# the cost volume's two readers as mvs_conv3d_pair_f32 takes them: one pass over the volume where its shapes are built
REGNET_PAIR = ("3dconv0_1", "3dconv1_0")
# The backward pass's order.  Not the table's reversed: the gradient of the full-resolution sum 6_0 + 0_1 dies early and the
# activations two layers read (1_0 by 1_1 and 2_0, 2_0 by 2_1 and 3_0) are recomputed once and used while they live.
REGNET_BACKWARD_ORDER = ("3dconv6_2", "3dconv6_0", "3dconv0_1", "3dconv5_0", "3dconv1_1", "3dconv4_0", "3dconv2_1",
                         "3dconv3_1", "3dconv3_0", "3dconv2_0", "3dconv1_0")


def backward_order_is_valid(order=REGNET_BACKWARD_ORDER):
    """Every layer once, and after all of its consumers: their gradients are what its own backward starts from."""
    at = {n: i for i, n in enumerate(order)}
    return sorted(order) == sorted(REGNET_ORDER) and all(at[c] < at[n] for n in REGNET_ORDER for c in REGNET_CONSUMERS[n])


assert backward_order_is_valid()
assert set(REGNET_PAIR) == set(REGNET_CONSUMERS[None])
