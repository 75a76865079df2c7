"""Preconditions of tests/test_gpu_wgrad_seams.py, asserted without a GPU: the table of tests/wgrad_seam_cases.py is the set of
kernels `dispatch` of conv3d_wgrad.hip reaches, every weight gradient of RegNetUS0 maps to a row, the shapes hold the seams they
are there for, and -- from the float64 reference alone -- a seam defect moves some per-tap distance to at least 100 times the
whole-tensor bound (2e-5), so it cannot hide in either criterion of the GPU test.

The weight gradient is linear in `small`, so each defect is the reference of a masked `small` added to or taken from the true
one.  At every row's base and all-axes shape (Ds = 5: chunks of 3 and 2 planes; one plane each for wgrad_c1_kernel), per kind:

  column    the last `small` column (w = Ws - 1: the one-voxel tile) is dropped;
  short     the last plane of a chunk -- the first chunk that ends on an interior plane: plane 2, or plane 1 for wgrad_c1_kernel -- is
            missing from the nine kd = 0 taps (a chunk that stops pairing one plane early);
  twice     that plane is counted twice in the nine kd = 2 taps: its big plane S od + 2 - pad is the halo plane both chunks
            stage.

Smallest margin over the table (largest per-tap distance of the defect / 2e-5; printed with pytest -s):

    defect    smallest margin    at
    column         8836          run[8,1,2,4]-8to16-s2-deconv-5x9x33
    short         22597          run[64,2,2,4]-64to24-s2-deconv-5x9x33
    twice         25121          run[32,2,1,8]-32to32-s1-conv-5x17x33
"""
import os
import re

import numpy as np
import pytest

from mvsnet_amd.regnet_layers import REGNET_LAYERS
from tests import wgrad_seam_cases as T

MARGIN = 100.0
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvsnet_amd", "csrc")


def _dispatch_text():
    with open(os.path.join(CSRC, "conv3d_wgrad.hip")) as f:
        src = f.read()
    return src[src.index("int dispatch("):src.index("extern \"C\" size_t mvs_conv3d_wgrad_workspace_bytes")]


def test_the_table_is_the_set_of_instantiations_dispatch_names():
    text = _dispatch_text()
    lines = re.findall(r"WG_CASE\((\d+), (\d+), (\d+), (\d+)\)", text)
    assert len(lines) == len(set(lines)) == 11, lines                      # no line twice: a second one is dead
    named = {"run<%s, %s, %s, %s>" % l for l in lines}
    assert "wgrad_flat_kernel<8, CTF, TH><<<" in text and "constexpr int TH = 8, CTF = 2;" in text
    assert "mvs_wgrad_c1_launch(" in text
    named |= {"wgrad_flat_kernel<8, 2, 8>", "wgrad_c1_kernel<8>"}
    assert named == set(T.ROW_OF) and len(T.ROWS) == 13
    for r in T.ROWS:
        if r.name.startswith("run<"):
            cb, ct, s, th = map(int, re.findall(r"\d+", r.name))
            assert (r.cb, r.ct, r.stride, r.tile) == (cb, ct, s, (th, 16)), r.name
        assert r.kinds == (("conv", "deconv") if r.stride == 2 else ("conv",)), r.name
        for cs in r.css:
            assert T.select(r.cb, cs, r.stride) == r.name, (r.name, cs)
    with open(os.path.join(CSRC, "conv3d_c1.hip")) as f:
        assert "constexpr int TH = 8, TW = 32," in f.read()                # the c1 row's tile
    assert T.ROW_OF["wgrad_c1_kernel<8>"].tile == (8, 32) and T.ROW_OF["wgrad_flat_kernel<8, 2, 8>"].tile == (8, 16)
    # every CT group runs a Csmall that is no multiple of 16
    for ct in (1, 2, 4):
        assert any(cs % 16 for r in T.ROWS if r.ct == ct and r.name.startswith("run<") for cs in r.css), ct
    assert set(T.UNTESTED_BEFORE) <= set(T.ROW_OF)


def test_every_weight_gradient_of_the_network_maps_to_a_row():
    seen = set()
    for layer in REGNET_LAYERS:
        cb, cs, stride = T.layer_operands(layer, 32, 8)
        name = T.select(cb, cs, stride)
        assert name in T.ROW_OF, (layer.name, cb, cs, stride)
        assert cs in T.ROW_OF[name].css, (layer.name, cs)                  # ... at the layer's own channel count
        seen.add(name)
    assert "wgrad_flat_kernel<8, 2, 8>" in seen and "wgrad_c1_kernel<8>" in seen
    assert T.select(12, 8, 1) is None and T.select(64, 64, 2) is None and T.select(8, 32, 2) is None


def test_the_shapes_hold_the_seams_they_are_there_for():
    assert len(set(map(T.case_id, T.CASES))) == len(T.CASES)
    for r in T.ROWS:
        th, tw = r.tile
        hw = {(s[1], s[2]) for s in r.shapes if s[0] == 5}
        assert hw == {(th + 1, tw + 1), (th - 1, tw + 1), (2 * th + 1, tw + 1), (th + 1, tw - 1), (th + 1, 2 * tw + 1),
                      (th - 1, tw - 1), (2 * th + 1, 2 * tw + 1)}, r.name
        assert {s[0] for s in r.shapes if (s[1], s[2]) == (th + 1, tw + 1)} >= set(T.DEPTHS), r.name
        base = (th + 1, tw + 1)
        if r.name.startswith("wgrad_c1"):
            assert all(T.chunk_planes(r, (d,) + base) == [(k, k + 1) for k in range(d)] for d in T.DEPTHS)
        else:                                                              # 1 | 2 | 3 + 2 | 3 + 3 + 1 planes
            assert [T.chunk_planes(r, (d,) + base) for d in T.DEPTHS] == [[(0, 1)], [(0, 2)], [(0, 3), (3, 5)], [(0, 3), (3, 6), (6, 7)]]
        for c in (c for c in T.CASES if c.name == r.name):
            assert c.shape in r.shapes and c.cs in r.css and c.kind in r.kinds
        first = [c for c in T.CASES if c.name == r.name and c.cs == r.css[0]]
        assert len(first) == len(r.shapes) * len(r.kinds), r.name          # the first Csmall at every shape, every kind
        for cs in r.css[1:]:
            assert {c.shape for c in T.CASES if c.name == r.name and c.cs == cs} == set(T.seam_shapes(r)), (r.name, cs)
    # the slices make_plan divides the 1024 workgroups by, from WGeom: 27 * CB * CS / 64 accumulator floats per lane do not fit
    slices = {r.name: T.plan(r, r.shapes[0])[1] for r in T.ROWS}
    assert slices["run<64, 4, 1, 4>"] == 4 and slices["run<64, 2, 2, 4>"] == 2 and slices["run<32, 4, 2, 4>"] == 2
    assert all(v == 1 for k, v in slices.items() if k.startswith("run<") and k not in ("run<64, 4, 1, 4>", "run<64, 2, 2, 4>", "run<32, 4, 2, 4>"))


def test_the_deep_c1_volume_is_the_smallest_with_two_planes_per_workgroup_and_a_last_chunk_of_one():
    r = T.ROW_OF["wgrad_c1_kernel<8>"]
    assert T.c1_deep_candidates()[0][1] == T.C1_DEEP and T.C1_DEEP in r.shapes
    tiles, _, ppw, chunks = T.plan(r, T.C1_DEEP)
    assert (tiles, ppw, chunks) == (4, 2, 44) and T.chunk_planes(r, T.C1_DEEP)[-1] == (86, 87)
    d, h, w = T.C1_DEEP
    assert T.plan(r, (d - 2, h, w))[2] == 1                                # two planes fewer: a plane per chunk again


def _defects(c, row):
    """-> {name: per-tap distance (27,) of the defective gradient from the true one}."""
    ref = T.reference(c)
    big, small = T.case_arrays(c)
    # the first chunk that ends inside the volume on a plane with neighbours on both sides (kd = 0 and kd = 2 both pair it)
    od0, od1 = next(ch for ch in T.chunk_planes(row, c.shape) if ch[1] - 1 >= 1 and ch[1] < c.shape[0])
    col = small.copy(); col[:, :, :-1] = 0                                # only the last column
    pl = np.zeros_like(small); pl[od1 - 1] = small[od1 - 1]               # only that chunk's last plane
    d_col = T.wgrad_autograd(c.kind, big, col, c.stride)
    d_pl = T.wgrad_autograd(c.kind, big, pl, c.stride)
    short = ref.copy(); short[0] -= d_pl[0]
    twice = ref.copy(); twice[2] += d_pl[2]
    return {"column": T.per_tap(ref - d_col, ref), "short": T.per_tap(short, ref), "twice": T.per_tap(twice, ref)}


SEAM_CASES = [c for c in T.CASES if c.shape in T.seam_shapes(T.ROW_OF[c.name])]
_smallest = {}


@pytest.mark.parametrize("c", SEAM_CASES, ids=list(map(T.case_id, SEAM_CASES)))
def test_a_seam_defect_shows_a_hundred_times_over_in_some_tap(c):
    row = T.ROW_OF[c.name]
    for name, dist in _defects(c, row).items():
        margin = float(dist.max()) / T.WHOLE_BOUND
        if name not in _smallest or margin < _smallest[name][0]:
            _smallest[name] = (margin, T.case_id(c))
        assert margin >= MARGIN, (name, margin)
        if name != "column":                                              # confined to nine taps: the others are exact
            kd = 0 if name == "short" else 2
            assert np.count_nonzero(dist) == 9 and np.all(dist[9 * kd:9 * kd + 9] > 0), name


def test_print_the_smallest_margins():
    for name, (margin, where) in sorted(_smallest.items()):
        print("\n    %-8s %10.0f          %s" % (name, margin, where))
    assert len(_smallest) in (0, 3)
