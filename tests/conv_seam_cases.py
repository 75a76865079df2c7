"""Every 3-D convolution launcher behind mvs_conv3d_f32 / mvs_deconv3d_f32 at the seams of its own tiling: the case table.

A plain helper module (no fixtures, no GPU): tests/test_conv_seam_cases_host.py asserts from the float64 reference alone that a
seam defect cannot hide inside the tolerance at these cases, tests/test_gpu_conv_seams.py runs them.

One row per launcher instantiation that the two entry points reach WITHOUT prepared weights.  Read from regnet.hip (the entry
points), conv3d_mfma.hip mvs_conv3d_dispatch, conv3d_os.hip mvs_conv3d_os_launch / os_variant_of, conv3d_s2_mfma.hip
mvs_conv3d_s2_mfma, deconv3d_mfma.hip mvs_deconv3d_mfma_launch, deconv3d_c8.hip mvs_deconv3d_c8_launch, conv3d_out.hip
mvs_conv3d_out_launch, conv3d_k8.hip mvs_conv3d_k8_launch, conv3d_c8.hip mvs_conv3d_c8_launch and conv3d_c1.hip
mvs_conv3d_in1_launch (that file's second launcher, mvs_wgrad_c1_launch, is a weight gradient: no convolution entry reaches it).
Tiles are (td, th, tw) in the units the launcher tiles -- OUTPUT voxels for stride 1 and 2, INPUT voxels for the transposed
kernels; td = - for the plane-march kernels, which cut depth into plane ranges (tests/test_gpu_halo_planes.py).  Forms: plain
(x and w alone), affine (input scale / shift + ReLU, BatchNorm sums), fused (affine, skip input with its own affine, sums),
skip (fused without sums: the output layer has no BatchNorm).

  kind  Cin -> Cout        launcher                              tile      forms         selected when                          file
  s1    4|8|16 -> 1        launch_out<Cin>                       - 8 32    plain skip    Cout == 1, no sums                     conv3d_out
  s1    1 -> 8|4           conv3d_in1_kernel<Cout>               - 8 32    plain         Cin == 1, plain only                   conv3d_c1
  s1    8 -> 32            conv3d_k8_kernel<32>                  - 8 16    plain         Cin == 8, Cout == 32, plain only       conv3d_k8
  s1    64 -> 64           launch_os<OS_S1, 64, 4, 2, 2, 1, 1>   2 4 4     plain fused   os_variant_of                          conv3d_os
  s1    32 -> 32           launch_os<OS_S1, 32, 2, 2, 2, 1, 2>   2 4 8     plain fused   os_variant_of                          conv3d_os
  s1    128 -> 128         launch_os<OS_S1, 128, 4, 2, 2, 1, 1>  2 4 4     plain fused   os_variant_of ('fat')                  conv3d_os
  s1    32 -> 8            launch_c8<false>                      - 8 16    plain affine  no skip input                          conv3d_c8
  s1    32 -> 8            launch_s1<32, 8, 8>                   - 8 16    fused         skip input                             conv3d_mfma
  s1    16 -> 16k          launch_s1<16, 16, 8>                  - 8 16    plain fused   Cout % 16 == 0                         conv3d_mfma
  s1    32 -> 16k (not 32) launch_s1<32, 16, 8, 8, 2>            - 8 8     plain fused   W % 16 != 0 and W % 8 == 0             conv3d_mfma
  s1    32 -> 16k (not 32) launch_s1<32, 16, 8>                  - 8 16    plain fused   W % 16 == 0 or W % 8 != 0              conv3d_mfma
  s1    64 -> 8k (not 64)  launch_s1<64, 8, 16, 4, 4>            - 16 4    plain fused   W % 16 != 0, W % 4 == 0, H % 16 == 0   conv3d_mfma
  s1    64 -> 8k (not 64)  launch_s1<64, 8, 4>                   - 4 16    plain fused   otherwise                              conv3d_mfma
  s1    16 -> 8            launch_s1<16, 8, 8>                   - 8 16    plain fused   Cout == 8                              conv3d_mfma
  s2    32 -> 64           launch_os<OS_S2, 32, 4, 2, 2, 1, 1>   2 4 4     plain fused   os_variant_of                          conv3d_os
  s2    64 -> 32           launch_os<OS_S2, 64, 2, 1, 2, 1, 1>   2 4 4     plain fused   os_variant_of ('fat')                  conv3d_os
  s2    64 -> 128          launch_os<OS_S2, 64, 4, 2, 2, 1, 1>   2 4 4     plain fused   os_variant_of ('fat')                  conv3d_os
  s2    32 -> 16k (not 64) launch_s2<32, 4>                      - 4 16    plain fused   Cout % 16 == 0                         conv3d_s2_mfma
  s2    16 -> 16k          launch_s2<16, 4>                      - 4 16    plain fused   Cout % 16 == 0                         conv3d_s2_mfma
  tr    64 -> 32           launch_os<OS_DECONV, 64, 2, 1, 2, 1, 1>   2 4 4   plain fused   os_variant_of                        conv3d_os
  tr    32 -> 16           launch_os<OS_DECONV, 32, 1, 2, 2, 2, 2>   2 8 8   plain fused   os_variant_of                        conv3d_os
  tr    128 -> 64          launch_os<OS_DECONV, 128, 2, 1, 2, 1, 1>  2 4 4   plain fused   os_variant_of ('fat')                conv3d_os
  tr    16 -> 8            launch_deconv_c8<16>                  - 8 16    plain fused   Cout == 8                              deconv3d_c8
  tr    64 -> 8k (not 32)  launch_deconv_c8<64>                  - 8 16    plain fused   Cout % 8 == 0                          deconv3d_c8
  tr    32 -> 16k (not 16) launch_deconv<32, 16, 8>              - 8 16    plain fused   Cout % 16 == 0                         deconv3d_mfma
  tr    16 -> 16k          launch_deconv<16, 16, 8>              - 8 16    plain fused   Cout % 16 == 0                         deconv3d_mfma

Not in the table: launch_deconv<16, 8, 8> and launch_deconv<64, 8, 8> are only taken when mvs_deconv3d_c8_launch answers
MVS_E_SHAPE for a volume of 2 GiB or more (32-bit buffer offsets) -- no float64 reference fits a test at that size; the fused pair
entry (mvs_conv3d_pair_f32: tests/test_gpu_pair_roles.py, test_gpu_pair_winograd.py); the opt-in bf16x3 family and everything
that needs prepared weights (the filled launches and FUSE2: test_gpu_conv_seams.py's whole-network shapes).

Shapes per row (tiled_shapes; Row.tile holds 0 for the `-` above): for an axis with tile t the extents t - 1 (one partial tile), t + 1 (a full tile and a one-voxel
tile) and 2 t + 1 (an interior tile with neighbours on both sides), one axis at a time around the base (t_h + 1, t_w + 1), and
(2 t_h + 1, 2 t_w + 1) with both last tiles one voxel wide.  Depth: 5 planes for the plane-march rows, 3 (blocks 2|1) and 5
(2|2|1) for the block rows.  Stride 2: the INPUT extents are chosen so that the output extents take those values, 2 o for an even
input axis and 2 o - 1 for an odd one (pad_before is 0 / 1); every axis sees both.  The rows selected by residues of W and H
list their shapes by hand: launch_s1<32, 16, 8, 8, 2> only ever sees W = 8 mod 16 (whole 8-wide tiles: 8, 24, 40), launch_s1<64,
8, 16, 4, 4> only W = 4, 8, 12 mod 16 and H = 0 mod 16, and the rows on the other side of each condition get W = 16, 17 (32 -> 16)
and W in {12, 20} x H = 24, W = 16 (64 -> 16).  A row with a channel group G runs its first Cout at every shape and the others
(more than one group per launch) at the base and the all-axes shape.

Inputs (case_inputs) are those of conv_case / deconv_case in tests/test_gpu_arena.py -- Gaussian x and skip, weights scaled by
1 / sqrt(27 Cin), scale 1 + 0.3 N, shift 0.2 N, seeded per case -- with one forced condition: the first quarter of the input
channels have shift = 0.1 + |0.2 N| >= 0.1, so that a halo staged as relu(shift) instead of 0 shows.  Expectations are
oracle.mvsnet_oracle.conv3d_same / conv3d_transpose_same in float64.

REFUSED lists (Cin, Cout, kind, form) combinations no launcher of these families takes: under conv impl `mfma` the entry point
answers MVS_E_SHAPE and writes nothing, under `auto` the shape-generic kernel runs.
"""
import collections
import functools

import numpy as np

from oracle import mvsnet_oracle as O

FORMS = ("plain", "affine", "fused", "skip")
OUT_RTOL, OUT_ATOL = 1e-4, 2e-5              # tests/test_gpu_parity.py: outputs of these layer kinds
SUM_RTOL, SUM_ATOL = 1e-4, 1e-3              # ... and their two BatchNorm sums
MVS_E_SHAPE = -2

Row = collections.namedtuple("Row", "launcher kind cin couts tile forms file shapes")
Case = collections.namedtuple("Case", "launcher kind cin cout shape seed")        # shape = INPUT (D, H, W)


def form_has(form):
    """-> (input affine, skip input, BatchNorm sums) of a form."""
    return form != "plain", form in ("fused", "skip"), form in ("affine", "fused")


# ---- the selection rules, written once from the dispatchers --------------------------------------------------------------------
OS_LAUNCHERS = {      # mvs_conv3d_os_launch: (kind, Cin, Cout) -> instantiation; the keys are what os_variant_of answers >= 0 for
    ("s1", 64, 64): "launch_os<OS_S1, 64, 4, 2, 2, 1, 1>",
    ("s1", 32, 32): "launch_os<OS_S1, 32, 2, 2, 2, 1, 2>",
    ("s2", 32, 64): "launch_os<OS_S2, 32, 4, 2, 2, 1, 1>",
    ("tr", 64, 32): "launch_os<OS_DECONV, 64, 2, 1, 2, 1, 1>",
    ("tr", 32, 16): "launch_os<OS_DECONV, 32, 1, 2, 2, 2, 2>",
    ("s2", 64, 32): "launch_os<OS_S2, 64, 2, 1, 2, 1, 1>",
    ("s2", 64, 128): "launch_os<OS_S2, 64, 4, 2, 2, 1, 1>",
    ("s1", 128, 128): "launch_os<OS_S1, 128, 4, 2, 2, 1, 1>",
    ("tr", 128, 64): "launch_os<OS_DECONV, 128, 2, 1, 2, 1, 1>",
}


def select(kind, cin, cout, form, D, H, W):
    """The launcher instantiation mvs_conv3d_f32 (kind s1, s2) / mvs_deconv3d_f32 (tr) reaches under conv impl `mfma` for an input
    of (D, H, W, cin) without prepared weights, or None where the entry answers MVS_E_SHAPE.  Volumes below 2 GiB only."""
    assert D * H * W * max(cin, cout) * 8 * 4 < 2 ** 31
    aff, skip, sums = form_has(form)
    if (kind, cin, cout) in OS_LAUNCHERS:                     # (no pair of the block kernels has Cout 1 or Cin 1 / 8, asked first)
        return OS_LAUNCHERS[(kind, cin, cout)]
    if kind == "s1":                                          # mvs_conv3d_dispatch, stride 1, in its order
        if cout == 1:
            return "launch_out<%d>" % cin if not sums and cin in (8, 4, 16) else None
        if cin == 1:
            return "conv3d_in1_kernel<%d>" % cout if form == "plain" and cout in (8, 4) else None
        if cin == 8:
            return "conv3d_k8_kernel<32>" if form == "plain" and cout == 32 else None
        if cin == 32 and cout == 8:
            return "launch_s1<32, 8, 8>" if skip else "launch_c8<false>"
        if cin == 16 and cout % 16 == 0:
            return "launch_s1<16, 16, 8>"
        if cin == 32 and cout % 16 == 0:
            return "launch_s1<32, 16, 8, 8, 2>" if W % 16 != 0 and W % 8 == 0 else "launch_s1<32, 16, 8>"
        if cin == 64 and cout % 8 == 0:
            return "launch_s1<64, 8, 16, 4, 4>" if W % 16 != 0 and W % 4 == 0 and H % 16 == 0 else "launch_s1<64, 8, 4>"
        if cin == 16 and cout == 8:
            return "launch_s1<16, 8, 8>"
        return None
    if kind == "s2":                                          # mvs_conv3d_s2_mfma
        if cout % 16 == 0 and cin in (32, 16):
            return "launch_s2<%d, 4>" % cin
        return None
    assert kind == "tr"                                       # mvs_deconv3d_mfma_launch
    if cout % 8 == 0 and ((cin == 16 and cout == 8) or cin == 64):
        return "launch_deconv_c8<%d>" % cin                   # (MVS_E_SHAPE from it only at 2 GiB and more)
    if cin == 32 and cout % 16 == 0:
        return "launch_deconv<32, 16, 8>"
    if cin == 16 and cout % 16 == 0:
        return "launch_deconv<16, 16, 8>"
    return None


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def tiled_shapes(tile):
    """Extents in the units the launcher tiles, one axis at a time around the base, then all axes at once."""
    td, th, tw = tile
    d0 = 3 if td else 5
    base = (d0, th + 1, tw + 1)
    shapes = [base, (d0, th - 1, tw + 1), (d0, 2 * th + 1, tw + 1), (d0, th + 1, tw - 1), (d0, th + 1, 2 * tw + 1)]
    if td:
        shapes.append((5, th + 1, tw + 1))
    shapes.append((5, 2 * th + 1, 2 * tw + 1))
    return shapes


def stride2_inputs(out_shapes):
    """Input extents 2 o (even, pad_before 0) or 2 o - 1 (odd, pad_before 1): the base both ways, the varied axis odd for the
    partial single tile and even otherwise, the all-axes shape odd."""
    base = out_shapes[0]
    res = [tuple(2 * o for o in base), tuple(2 * o - 1 for o in base)]
    for s in out_shapes[1:-1]:
        res.append(tuple(2 * o - 1 if o < b else 2 * o for o, b in zip(s, base)))
    res.append(tuple(2 * o - 1 for o in out_shapes[-1]))
    return res


def _row(launcher, kind, cin, couts, tile, forms, file, shapes=None):
    if shapes is None:
        shapes = tiled_shapes(tile)
        if kind == "s2":
            shapes = stride2_inputs(shapes)
    return Row(launcher, kind, cin, tuple(couts), tile, tuple(forms), file, tuple(shapes))


PF, PO = ("plain", "fused"), ("plain",)
ROWS = (
    _row("launch_out<8>", "s1", 8, [1], (0, 8, 32), ("plain", "skip"), "conv3d_out.hip"),
    _row("launch_out<4>", "s1", 4, [1], (0, 8, 32), ("plain", "skip"), "conv3d_out.hip"),
    _row("launch_out<16>", "s1", 16, [1], (0, 8, 32), ("plain", "skip"), "conv3d_out.hip"),
    _row("conv3d_in1_kernel<8>", "s1", 1, [8], (0, 8, 32), PO, "conv3d_c1.hip"),
    _row("conv3d_in1_kernel<4>", "s1", 1, [4], (0, 8, 32), PO, "conv3d_c1.hip"),
    _row("conv3d_k8_kernel<32>", "s1", 8, [32], (0, 8, 16), PO, "conv3d_k8.hip"),
    _row("launch_os<OS_S1, 64, 4, 2, 2, 1, 1>", "s1", 64, [64], (2, 4, 4), PF, "conv3d_os.hip"),
    _row("launch_os<OS_S1, 32, 2, 2, 2, 1, 2>", "s1", 32, [32], (2, 4, 8), PF, "conv3d_os.hip"),
    _row("launch_os<OS_S1, 128, 4, 2, 2, 1, 1>", "s1", 128, [128], (2, 4, 4), PF, "conv3d_os.hip"),
    _row("launch_c8<false>", "s1", 32, [8], (0, 8, 16), ("plain", "affine"), "conv3d_c8.hip"),
    _row("launch_s1<32, 8, 8>", "s1", 32, [8], (0, 8, 16), ("fused",), "conv3d_mfma.hip"),
    _row("launch_s1<16, 16, 8>", "s1", 16, [16, 32], (0, 8, 16), PF, "conv3d_mfma.hip"),
    # W = 8 mod 16 only: whole 8-wide tiles, one, three and five of them
    _row("launch_s1<32, 16, 8, 8, 2>", "s1", 32, [16, 48], (0, 8, 8), PF, "conv3d_mfma.hip",
         [(5, 9, 24), (5, 7, 24), (5, 17, 24), (5, 9, 8), (5, 9, 40), (5, 17, 40)]),
    # the tile's own extents (15, 17, 33 are neither 0 mod 16 nor 0 mod 8) and W = 16, the other way into this kernel
    _row("launch_s1<32, 16, 8>", "s1", 32, [16, 48], (0, 8, 16), PF, "conv3d_mfma.hip",
         tiled_shapes((0, 8, 16)) + [(5, 9, 16)]),
    # W = 4, 12, 20 (one, three, five 4-wide tiles), H = 16, 32, 48
    _row("launch_s1<64, 8, 16, 4, 4>", "s1", 64, [16, 24], (0, 16, 4), PF, "conv3d_mfma.hip",
         [(5, 16, 12), (5, 16, 20), (5, 16, 4), (5, 32, 12), (5, 48, 20)]),
    # the tile's own extents, then the other side of each of the three conditions above
    _row("launch_s1<64, 8, 4>", "s1", 64, [16, 24], (0, 4, 16), PF, "conv3d_mfma.hip",
         tiled_shapes((0, 4, 16)) + [(5, 24, 12), (5, 24, 20), (5, 16, 16)]),
    _row("launch_s1<16, 8, 8>", "s1", 16, [8], (0, 8, 16), PF, "conv3d_mfma.hip"),
    _row("launch_os<OS_S2, 32, 4, 2, 2, 1, 1>", "s2", 32, [64], (2, 4, 4), PF, "conv3d_os.hip"),
    _row("launch_os<OS_S2, 64, 2, 1, 2, 1, 1>", "s2", 64, [32], (2, 4, 4), PF, "conv3d_os.hip"),
    _row("launch_os<OS_S2, 64, 4, 2, 2, 1, 1>", "s2", 64, [128], (2, 4, 4), PF, "conv3d_os.hip"),
    _row("launch_s2<32, 4>", "s2", 32, [16, 32], (0, 4, 16), PF, "conv3d_s2_mfma.hip"),
    _row("launch_s2<16, 4>", "s2", 16, [32, 16], (0, 4, 16), PF, "conv3d_s2_mfma.hip"),
    _row("launch_os<OS_DECONV, 64, 2, 1, 2, 1, 1>", "tr", 64, [32], (2, 4, 4), PF, "conv3d_os.hip"),
    _row("launch_os<OS_DECONV, 32, 1, 2, 2, 2, 2>", "tr", 32, [16], (2, 8, 8), PF, "conv3d_os.hip"),
    _row("launch_os<OS_DECONV, 128, 2, 1, 2, 1, 1>", "tr", 128, [64], (2, 4, 4), PF, "conv3d_os.hip"),
    _row("launch_deconv_c8<16>", "tr", 16, [8], (0, 8, 16), PF, "deconv3d_c8.hip"),
    _row("launch_deconv_c8<64>", "tr", 64, [16, 8], (0, 8, 16), PF, "deconv3d_c8.hip"),
    _row("launch_deconv<32, 16, 8>", "tr", 32, [32], (0, 8, 16), PF, "deconv3d_mfma.hip"),
    _row("launch_deconv<16, 16, 8>", "tr", 16, [16, 32], (0, 8, 16), PF, "deconv3d_mfma.hip"),
)
ROW_OF = {r.launcher: r for r in ROWS}

# Seeds moved off 0, {case id: seed}: with seed 0 the case missed the 100x stray-lane margin of
# tests/test_conv_seam_cases_host.py.  One voxel is 1 / N of a sum held to rtol 1e-4, so at N of a few thousand voxels it shows
# 100 times over only where some channel's sum lies near zero (the absolute part of the bound then rules); the seed is the first
# one at which that is so and the seam and padding margins hold as well.  A property of the reference alone.
SEEDS = {
    's1-launch_c8[false]-32to8-5x9x17': 1,
    's1-launch_c8[false]-32to8-5x7x17': 1,
    's1-launch_c8[false]-32to8-5x9x15': 1,
    's1-launch_c8[false]-32to8-5x9x33': 1,
    's1-launch_c8[false]-32to8-5x17x33': 1,
    's1-launch_s1[32,8,8]-32to8-5x9x17': 1,
    's1-launch_s1[32,8,8]-32to8-5x17x17': 12,
    's1-launch_s1[32,8,8]-32to8-5x9x15': 1,
    's1-launch_s1[32,8,8]-32to8-5x9x33': 1,
    's1-launch_s1[32,8,8]-32to8-5x17x33': 18,
    's1-launch_s1[16,16,8]-16to16-5x9x17': 2,
    's1-launch_s1[16,16,8]-16to16-5x7x17': 1,
    's1-launch_s1[16,16,8]-16to16-5x9x33': 1,
    's1-launch_s1[16,16,8]-16to32-5x17x33': 3,
    's1-launch_s1[32,16,8,8,2]-32to16-5x9x24': 1,
    's1-launch_s1[32,16,8,8,2]-32to16-5x17x24': 2,
    's1-launch_s1[32,16,8,8,2]-32to16-5x9x8': 1,
    's1-launch_s1[32,16,8,8,2]-32to16-5x9x40': 1,
    's1-launch_s1[32,16,8,8,2]-32to16-5x17x40': 22,
    's1-launch_s1[32,16,8]-32to16-5x9x33': 1,
    's1-launch_s1[32,16,8]-32to16-5x17x33': 1,
    's1-launch_s1[32,16,8]-32to16-5x9x16': 1,
    's1-launch_s1[64,8,16,4,4]-64to16-5x16x20': 1,
    's1-launch_s1[64,8,16,4,4]-64to16-5x48x20': 2,
    's1-launch_s1[64,8,16,4,4]-64to24-5x48x20': 5,
    's1-launch_s1[64,8,4]-64to16-5x9x17': 3,
    's1-launch_s1[64,8,4]-64to16-5x5x33': 1,
    's1-launch_s1[64,8,4]-64to16-5x24x20': 3,
    's1-launch_s1[64,8,4]-64to24-5x16x16': 2,
    's1-launch_s1[16,8,8]-16to8-5x9x17': 1,
    's1-launch_s1[16,8,8]-16to8-5x7x17': 1,
    's1-launch_s1[16,8,8]-16to8-5x17x17': 4,
    's1-launch_s1[16,8,8]-16to8-5x9x15': 1,
    's1-launch_s1[16,8,8]-16to8-5x9x33': 7,
    's1-launch_s1[16,8,8]-16to8-5x17x33': 6,
    's2-launch_s2[32,4]-32to16-10x10x34': 2,
    's2-launch_s2[32,4]-32to16-10x10x66': 2,
    's2-launch_s2[16,4]-16to32-9x17x65': 2,
    's2-launch_s2[16,4]-16to16-9x17x65': 2,
    'tr-launch_os[OS_DECONV,32,1,2,2,2,2]-32to16-3x9x9': 1,
    'tr-launch_os[OS_DECONV,32,1,2,2,2,2]-32to16-5x17x17': 7,
    'tr-launch_deconv_c8[16]-16to8-5x17x17': 1,
    'tr-launch_deconv_c8[16]-16to8-5x9x15': 1,
    'tr-launch_deconv_c8[16]-16to8-5x9x33': 4,
    'tr-launch_deconv_c8[16]-16to8-5x17x33': 62,
    'tr-launch_deconv_c8[64]-64to16-5x9x17': 2,
    'tr-launch_deconv_c8[64]-64to16-5x7x17': 1,
    'tr-launch_deconv_c8[64]-64to16-5x17x17': 11,
    'tr-launch_deconv_c8[64]-64to16-5x9x33': 16,
    'tr-launch_deconv_c8[64]-64to16-5x17x33': 1,
    'tr-launch_deconv_c8[64]-64to8-5x17x33': 4,
    'tr-launch_deconv[32,16,8]-32to32-5x9x17': 1,
    'tr-launch_deconv[32,16,8]-32to32-5x17x17': 1,
    'tr-launch_deconv[32,16,8]-32to32-5x9x33': 4,
    'tr-launch_deconv[32,16,8]-32to32-5x17x33': 2,
    'tr-launch_deconv[16,16,8]-16to16-5x7x17': 4,
    'tr-launch_deconv[16,16,8]-16to16-5x17x17': 10,
    'tr-launch_deconv[16,16,8]-16to16-5x9x15': 1,
    'tr-launch_deconv[16,16,8]-16to16-5x9x33': 4,
    'tr-launch_deconv[16,16,8]-16to16-5x17x33': 8,
    'tr-launch_deconv[16,16,8]-16to32-5x9x17': 1,
}


def case_id(c):
    return "%s-%s-%dto%d-%s" % (c.kind, c.launcher.replace(" ", "").replace("<", "[").replace(">", "]"), c.cin, c.cout,
                                "x".join(map(str, c.shape)))


def _cases():
    out = []
    for r in ROWS:
        for k, cout in enumerate(r.couts):
            shapes = r.shapes if k == 0 else (r.shapes[0], r.shapes[-1])
            for s in shapes:
                c = Case(r.launcher, r.kind, r.cin, cout, s, 0)
                out.append(c._replace(seed=SEEDS.get(case_id(c), 0)))
    return tuple(out)


CASES = _cases()

# (Cin, Cout, kind, form, input shape): nothing in the MFMA families takes these -- each with the line that refuses it
REFUSED = (
    (8, 8, "s1", "plain", (3, 9, 17)),        # mvs_conv3d_k8_launch: Cout != 32
    (8, 16, "s1", "plain", (3, 9, 17)),       # the same
    (8, 32, "s1", "fused", (3, 9, 17)),       # mvs_conv3d_k8_launch: plain convolution only
    (1, 8, "s1", "fused", (3, 9, 33)),        # mvs_conv3d_in1_launch: plain convolution only
    (1, 16, "s1", "plain", (3, 9, 33)),       # mvs_conv3d_in1_launch: Cout is neither 8 nor 4
    (8, 1, "s1", "fused", (3, 9, 33)),        # mvs_conv3d_out_launch: the output layer has no BatchNorm sums
    (32, 1, "s1", "plain", (3, 9, 33)),       # mvs_conv3d_out_launch: Cin is none of 8, 4, 16
    (16, 24, "s1", "plain", (3, 9, 17)),      # mvs_conv3d_dispatch: Cin 16 takes Cout = 8 or a multiple of 16
    (32, 24, "s1", "fused", (3, 9, 17)),      # ... Cin 32 takes Cout = 8 or a multiple of 16
    (64, 12, "s1", "plain", (3, 5, 17)),      # ... Cin 64 takes multiples of 8
    (12, 6, "s1", "plain", (3, 5, 6)),        # ... no kernel for Cin 12
    (12, 6, "s2", "fused", (6, 10, 12)),      # mvs_conv3d_s2_mfma: Cout % 16
    (32, 24, "s2", "plain", (5, 9, 33)),      # the same
    (64, 16, "s2", "plain", (5, 9, 9)),       # mvs_conv3d_s2_mfma: Cin 64 outside the three block-kernel pairs
    (8, 4, "tr", "fused", (3, 5, 6)),         # mvs_deconv3d_mfma_launch: no kernel for Cin 8
    (32, 8, "tr", "plain", (3, 9, 17)),       # ... Cin 32 takes multiples of 16
    (16, 12, "tr", "plain", (3, 9, 17)),      # ... Cin 16 takes Cout = 8 or a multiple of 16
    (64, 12, "tr", "fused", (3, 9, 17)),      # ... Cin 64 takes multiples of 8
)


# ---- inputs and float64 expectations --------------------------------------------------------------------------------------------
def out_shape(kind, shape):
    if kind == "s1":
        return tuple(shape)
    return tuple((n + 1) // 2 for n in shape) if kind == "s2" else tuple(2 * n for n in shape)


def pad_before(n):
    """SAME padding in front of a stride-2 axis of n inputs (mvs_conv3d_dispatch)."""
    return 1 if n % 2 else 0


def conv64(kind, xin, wgt):
    if kind == "tr":
        return O.conv3d_transpose_same(xin, wgt, 2, np.float64)
    return O.conv3d_same(xin, wgt, 2 if kind == "s2" else 1, np.float64)


def staged_input(form, inp):
    """What the kernel convolves, in float64: the raw input, or relu(x scale + shift) (+ the same of the skip input)."""
    x = inp["x"].astype(np.float64)
    aff, skip, _ = form_has(form)
    if not aff:
        return x
    xin = np.maximum(x * inp["sc"] + inp["sh"], 0)
    if skip:
        xin = xin + np.maximum(inp["x2"].astype(np.float64) * inp["sc2"] + inp["sh2"], 0)
    return xin


Inputs = collections.namedtuple("Inputs", "arrays expect bn")


@functools.lru_cache(maxsize=None)
def case_inputs(kind, cin, cout, shape, seed=0):
    """-> (arrays, expect, bn): float32 operands by name, {form: float64 output} for every form, {form: float64 BN + ReLU of it}
    for the forms with sums.  Read-only."""
    D, H, W = shape
    stride = 2 if kind == "s2" else 1
    rs = np.random.RandomState((D + H + W + cin + cout + (7 if kind == "tr" else stride) + 1000 * seed) % 2 ** 32)
    f32 = np.float32
    x = rs.standard_normal((D, H, W, cin)).astype(f32)
    x2 = rs.standard_normal((D, H, W, cin)).astype(f32)
    wshape = (3, 3, 3, cout, cin) if kind == "tr" else (3, 3, 3, cin, cout)
    wgt = (rs.standard_normal(wshape) / np.sqrt(27 * cin)).astype(f32)
    sc = (1 + 0.3 * rs.standard_normal(cin)).astype(f32); sh = (0.2 * rs.standard_normal(cin)).astype(f32)
    sc2 = (1 + 0.3 * rs.standard_normal(cin)).astype(f32); sh2 = (0.2 * rs.standard_normal(cin)).astype(f32)
    gamma = (1 + 0.2 * rs.standard_normal(cout)).astype(f32); beta = (0.1 * rs.standard_normal(cout)).astype(f32)
    q = (cin + 3) // 4                                       # the forced condition: a quarter of the channels with shift >= 0.1
    sh[:q] = 0.1 + np.abs(sh[:q]); sh2[:q] = 0.1 + np.abs(sh2[:q])
    arrays = dict(x=x, x2=x2, w=wgt, sc=sc, sh=sh, sc2=sc2, sh2=sh2, gamma=gamma, beta=beta)
    expect, bn = {}, {}
    for form in FORMS:
        expect[form] = conv64(kind, staged_input(form, arrays), wgt)
        if form_has(form)[2]:
            bn[form] = O.batch_norm_train(expect[form], gamma, beta, 1e-5, True, np.float64)
    for a in list(arrays.values()) + list(expect.values()) + list(bn.values()):
        a.setflags(write=False)
    return Inputs(arrays, expect, bn)


def inputs_of(case):
    return case_inputs(case.kind, case.cin, case.cout, case.shape, case.seed)


def sums_of(e):
    """The two float64 BatchNorm sums of an output (.., C): (2, C)."""
    flat = e.reshape(-1, e.shape[-1])
    return np.stack([flat.sum(0), (flat ** 2).sum(0)])


def out_bound(e):
    return OUT_ATOL + OUT_RTOL * np.abs(e)


def sum_bound(s):
    return SUM_ATOL + SUM_RTOL * np.abs(s)


# ---- where a voxel sits in the row's tiling (failure messages) -----------------------------------------------------------------
def tile_coordinates(kind, tile, voxel):
    """An OUTPUT voxel (d, h, w) as text: per axis tile index and position in the tile, in the units the launcher tiles (a
    transposed kernel tiles input voxels: output o belongs to input o // 2, parity o % 2)."""
    parts = []
    for name, t, o in zip("dhw", tile, voxel):
        i, par = (o // 2, "+%d/2" % (o % 2)) if kind == "tr" else (o, "")
        parts.append("%s=%d" % (name, o) if not t else "%s=%d (tile %d, pos %d of %d%s)" % (name, o, i // t, i % t, t, par))
    return ", ".join(parts)


def describe_failures(kind, tile, got, exp, rtol=OUT_RTOL, atol=OUT_ATOL, limit=8):
    """None when got is within atol + rtol |exp| everywhere, else a message naming the worst voxels by tile and position."""
    err = np.abs(got.astype(np.float64) - exp)
    bad = ~(err <= atol + rtol * np.abs(exp))                # (NaN counts as bad)
    if not bad.any():
        return None
    vox = bad.any(axis=-1)
    score = np.where(np.isfinite(err), err, np.inf).max(axis=-1)
    order = np.argsort(-np.where(vox, score, -1.0), axis=None)[:limit]
    lines = ["%d of %d voxels outside rtol %g atol %g; tile (td, th, tw) = %s; worst:" % (vox.sum(), vox.size, rtol, atol, (tile,))]
    for flat in order:
        v = np.unravel_index(flat, vox.shape)
        if not vox[v]:
            break
        c = int(np.argmax(np.where(np.isfinite(err[v]), err[v], np.inf)))
        lines.append("  %s: channel %d got %r expected %r" % (tile_coordinates(kind, tile, v), c, float(got[v][c]), float(exp[v][c])))
    return "\n".join(lines)
