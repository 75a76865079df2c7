"""Every weight-gradient kernel behind mvs_conv3d_wgrad_f32 at the seams of its own tiling and depth chunking: the case table.

A plain helper module (no fixtures, no GPU), after tests/conv_seam_cases.py: tests/test_wgrad_seam_cases_host.py asserts from the
float64 reference alone that a seam defect cannot hide inside the bounds at these cases and that the table covers `dispatch` of
conv3d_wgrad.hip, tests/test_gpu_wgrad_seams.py runs the cases.

    dW[tap][cb][cs] = sum_o  big[S o + tap - pad][cb] * small[o][cs]        (pad = 1 at stride 1, 0 at stride 2)

One row per instantiation `dispatch` reaches: the WG_CASE(CB, CT, S, TH) lines -- run<CB, CT, S, TH>, selected by Cbig = CB,
ceil(Csmall / 16) = CT and the stride -- and the two branches asked before them.  A workgroup owns a TH x 16 tile of `small`
voxels (8 x 32 in wgrad_c1_kernel, conv3d_c1.hip: TH, TW there) and a chunk of `small` planes.

  instantiation            Cbig  Csmall      stride  tile    kinds         layers of RegNetUS0 at base 8
  run<32, 1, 1, 8>         32    8           1       8 16    conv          -
  run<16, 1, 1, 8>         16    16          1       8 16    conv          3dconv1_1
  run<32, 2, 1, 8>         32    32, 24      1       8 16    conv          3dconv2_1
  run<64, 4, 1, 4>         64    64          1       4 16    conv          3dconv3_1
  run<8, 1, 1, 8>          8     8, 6        1       8 16    conv          -            (had no test: 8 -> 2..16 channels)
  run<32, 1, 2, 4>         32    16          2       4 16    conv deconv   3dconv1_0
  run<16, 2, 2, 4>         16    32          2       4 16    conv deconv   3dconv2_0, 3dconv5_0
  run<32, 4, 2, 4>         32    64, 56      2       4 16    conv deconv   3dconv3_0, 3dconv4_0
  run<8, 1, 2, 4>          8     16          2       4 16    conv deconv   3dconv6_0
  run<16, 1, 2, 4>         16    8           2       4 16    conv deconv   -            (had no test)
  run<64, 2, 2, 4>         64    24          2       4 16    conv deconv   -            (had no test)
  wgrad_flat_kernel<8,2,8> 8     32          1       8 16    conv          3dconv0_1 (operands swapped)
  wgrad_c1_kernel<8>       8     1           1       8 32    conv          3dconv6_2

Csmall: the first value runs at every shape, a second one at the base and the all-axes shape.  Every CT group has a Csmall that is
no multiple of 16 (8 under CT = 1, 24 under CT = 2, 56 under CT = 4): the `cs < a.CS` store guard and the zeroed LDS columns
beyond Csmall.  Csmall = 6 is no multiple of 4 either: the scalar staging of `small`.

Shapes, in `small` extents (Ds, Hs, Ws); big = S x small.  conv_seam_cases.tiled_shapes on the tile (0, th, tw): for an axis with
tile t the extents t - 1 (one partial tile -- with TH >= Hs and 16 >= Ws a `small` extent below the tile in both H and W never
occurs there, so (th - 1, tw - 1) is added), t + 1 (a whole tile and a one-voxel tile) and 2 t + 1, one axis at a time round
the base (th + 1, tw + 1), and (2 th + 1, 2 tw + 1); all at Ds = 5.  Depths Ds in {1, 2, 5, 7} at the base shape: `plan`
(make_plan's formulas, and the flat branch's own copy) cuts them into chunks of 1 | 2 | 3 + 2 | 3 + 3 + 1 planes, so a chunk
boundary re-stages its halo planes, and the last chunk is whole, short by one, or a single plane.  wgrad_c1_kernel takes a plane
per chunk at all of these (mvs_wgrad_c1_plan: chunks = min(1024 / (3 tiles), D)); C1_DEEP is the smallest volume of the row at
which it takes two planes per workgroup and ends in a chunk of one: for each H x W of the row the smallest D with
ceil(D / (1024 / (3 tiles))) = 2 and D odd, then the smallest D H W among them -- 87 x 9 x 33, the base extents (4 tiles: 85
chunks at most, 87 planes in 43 chunks of two and one of one).  c1_deep_candidates() recomputes the choice; the host test
asserts it.

Inputs are Gaussian, seeded per case; the expectation is oracle.torch_grad._conv / _deconv in float64 autograd, as
tests/test_gpu_backward.py's test_conv3d_weight_gradient_matches_autograd has it.
"""
import collections
import functools

import numpy as np
import torch

from oracle import torch_grad as TG
from tests.conv_seam_cases import tiled_shapes

WHOLE_BOUND = 2e-5                               # the project's whole-tensor relative L1 for a weight gradient
MVS_E_SHAPE = -2
DEPTHS = (1, 2, 5, 7)

Row = collections.namedtuple("Row", "name cb ct css stride tile kinds shapes")
Case = collections.namedtuple("Case", "name cb cs stride kind shape")             # shape = `small` extents (Ds, Hs, Ws)


def row_shapes(tile):
    th, tw = tile
    shapes = tiled_shapes((0, th, tw))                                           # base first, all-axes last, Ds = 5
    return tuple(shapes[:-1] + [(5, th - 1, tw - 1)] + [(d, th + 1, tw + 1) for d in DEPTHS if d != 5] + shapes[-1:])


def plan(row, shape):
    """-> (tiles, slices, planes per workgroup, chunks) for `small` extents: make_plan of conv3d_wgrad.hip, the flat branch's copy
    of it (one slice) and mvs_wgrad_c1_plan of conv3d_c1.hip."""
    Ds, Hs, Ws = shape
    th, tw = row.tile
    tiles = -(-Hs // th) * -(-Ws // tw)
    if row.name.startswith("wgrad_c1"):
        chunks = min(max(1024 // (3 * tiles), 1), Ds)
        slices = 3                                                               # blockIdx.y = kd
    else:
        qb = row.cb // 4
        tpg = 16 // qb
        ngrp = 3 * -(-9 // tpg)
        gpw = min(8 // row.ct, 4)
        slices = 1 if row.name.startswith("wgrad_flat") else -(-ngrp // (4 * gpw))
        chunks = min(max(1024 // (tiles * slices), 1), max(Ds // 2, 1))
    ppw = -(-Ds // chunks)
    return tiles, slices, ppw, -(-Ds // ppw)


def chunk_planes(row, shape):
    """The `small` planes of each chunk: [(od0, od1), ...]."""
    _, _, ppw, chunks = plan(row, shape)
    return [(c * ppw, min((c + 1) * ppw, shape[0])) for c in range(chunks)]


def workspace_bytes(row, cs, shape):
    """What mvs_conv3d_wgrad_workspace_bytes answers: one (27, CB, CS) float row per (tile, chunk)."""
    tiles, _, _, chunks = plan(row, shape)
    return tiles * chunks * 27 * row.cb * cs * 4


def _row(name, cb, ct, css, stride, tile, extra=()):
    kinds = ("conv", "deconv") if stride == 2 else ("conv",)
    return Row(name, cb, ct, tuple(css), stride, tile, kinds, row_shapes(tile) + tuple(extra))


C1_DEEP = (87, 9, 33)
ROWS = (
    _row("run<32, 1, 1, 8>", 32, 1, [8], 1, (8, 16)),
    _row("run<16, 1, 1, 8>", 16, 1, [16], 1, (8, 16)),
    _row("run<32, 2, 1, 8>", 32, 2, [32, 24], 1, (8, 16)),
    _row("run<64, 4, 1, 4>", 64, 4, [64], 1, (4, 16)),
    _row("run<8, 1, 1, 8>", 8, 1, [8, 6], 1, (8, 16)),
    _row("run<32, 1, 2, 4>", 32, 1, [16], 2, (4, 16)),
    _row("run<16, 2, 2, 4>", 16, 2, [32], 2, (4, 16)),
    _row("run<32, 4, 2, 4>", 32, 4, [64, 56], 2, (4, 16)),
    _row("run<8, 1, 2, 4>", 8, 1, [16], 2, (4, 16)),
    _row("run<16, 1, 2, 4>", 16, 1, [8], 2, (4, 16)),
    _row("run<64, 2, 2, 4>", 64, 2, [24], 2, (4, 16)),
    _row("wgrad_flat_kernel<8, 2, 8>", 8, 2, [32], 1, (8, 16)),
    _row("wgrad_c1_kernel<8>", 8, 1, [1], 1, (8, 32), extra=[C1_DEEP]),
)
ROW_OF = {r.name: r for r in ROWS}
UNTESTED_BEFORE = ("run<8, 1, 1, 8>", "run<16, 1, 2, 4>", "run<64, 2, 2, 4>")     # no test reached these three


def select(cb, cs, stride):
    """The instantiation `dispatch` reaches for (Cbig, Csmall, stride), or None where it answers MVS_E_SHAPE -- in its order."""
    if cs == 1 and cb == 8 and stride == 1:
        return "wgrad_c1_kernel<8>"
    if cb == 8 and cs == 32 and stride == 1:
        return "wgrad_flat_kernel<8, 2, 8>"
    ct = (cs + 15) // 16
    for r in ROWS:
        if r.name.startswith("run<") and (r.cb, r.ct, r.stride) == (cb, ct, stride):
            return r.name
    return None


def layer_operands(layer, cost_channels, base):
    """(Cbig, Csmall, stride) of a RegNetUS0 layer's weight gradient as backward.regnet_backward calls conv3d_wgrad: `big` is the
    finer volume -- a transposed layer's output gradient, the output gradient of the stride-1 conv on the raw cost volume (its
    operands are swapped), else the layer's input."""
    cin, cout = layer.channels(cost_channels, base)
    return (cout, cin, layer.stride) if layer.wgrad_gradient_first else (cin, cout, layer.stride)


def c1_deep_candidates():
    """For every H x W of the c1 row: the smallest D at which mvs_wgrad_c1_plan gives two planes per workgroup and a last chunk of
    one plane -> [(D H W voxels, (D, H, W))], smallest volume first."""
    row = ROW_OF["wgrad_c1_kernel<8>"]
    out = []
    for _, hs, ws in sorted(set((0, s[1], s[2]) for s in row_shapes(row.tile))):
        d = 1
        while True:
            _, _, ppw, chunks = plan(row, (d, hs, ws))
            if ppw == 2 and d - (chunks - 1) * ppw == 1:
                break
            d += 1
        out.append((d * hs * ws, (d, hs, ws)))
    return sorted(out)


def case_id(c):
    return "%s-%dto%d-s%d-%s-%s" % (c.name.replace(" ", "").replace("<", "[").replace(">", "]"), c.cb, c.cs, c.stride, c.kind,
                                    "x".join(map(str, c.shape)))


def _cases():
    out = []
    for r in ROWS:
        for k, cs in enumerate(r.css):
            shapes = r.shapes if k == 0 else (r.shapes[0], row_shapes(r.tile)[-1])
            for kind in r.kinds:
                out += [Case(r.name, r.cb, cs, r.stride, kind, s) for s in shapes]
    return tuple(out)


CASES = _cases()


def seam_shapes(row):
    """The base and the all-axes shape of a row: where the host test plants its defects."""
    return row.shapes[0], row_shapes(row.tile)[-1]


# ---- inputs and references ------------------------------------------------------------------------------------------------------
def case_arrays(c):
    """-> big (S Ds, S Hs, S Ws, CB), small (Ds, Hs, Ws, CS): float32 Gaussian, seeded per case."""
    rs = np.random.RandomState((c.cb * 1000 + c.cs * 10 + c.stride + 7 * sum(c.shape) + (3 if c.kind == "deconv" else 0)) % 2 ** 32)
    big = rs.standard_normal(tuple(c.stride * n for n in c.shape) + (c.cb,)).astype(np.float32)
    small = rs.standard_normal(tuple(c.shape) + (c.cs,)).astype(np.float32)
    return big, small


def wgrad_autograd(kind, big, small, stride, dtype=torch.float64):
    """dW (3, 3, 3, CB, CS) by torch-CPU autograd in `dtype`: a convolution has big = layer input and small = output gradient
    (w in the conv3d layout (3, 3, 3, Cin, Cout)), a transposed convolution big = output gradient and small = layer input (w in
    the conv3d_transpose layout (3, 3, 3, Cout, Cin))."""
    mk = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    w = torch.zeros((3, 3, 3, big.shape[-1], small.shape[-1]), dtype=dtype, requires_grad=True)
    if kind == "conv":
        y = TG._conv(mk(big).permute(3, 0, 1, 2)[None], w, stride)[0].permute(1, 2, 3, 0)
        (y * mk(small)).sum().backward()
    else:
        y = TG._deconv(mk(small).permute(3, 0, 1, 2)[None], w)[0].permute(1, 2, 3, 0)
        (y * mk(big)).sum().backward()
    return w.grad.numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(c):
    """The float64 weight gradient of a case.  Read-only."""
    big, small = case_arrays(c)
    ref = wgrad_autograd(c.kind, big, small, c.stride)
    ref.setflags(write=False)
    return ref


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


def per_tap(got, ref):
    """Relative L1 of each of the 27 (CB, CS) slabs: a defect confined to one tap does not average out.  -> (27,)"""
    g, r = np.asarray(got, np.float64).reshape(27, -1), np.asarray(ref, np.float64).reshape(27, -1)
    return np.abs(g - r).sum(1) / np.maximum(np.abs(r).sum(1), 1e-30)
