"""Preconditions of tests/test_gpu_conv_seams.py, asserted from the float64 reference alone (no GPU): at every case of
tests/conv_seam_cases.py a seam defect is at least 100 times the bound the GPU test holds the kernel to, so it cannot hide in it.

Convolution is linear in what the kernel stages, so "the output with part of the input zeroed / replaced" minus the true output is
the convolution of that part alone; every margin below is |such a difference| / (atol + rtol |true value|) with the GPU test's
rtol and atol (outputs 1e-4, 2e-5; BatchNorm sums 1e-4, 1e-3), for every form the row takes.

  seam      per seam plane of the row's tiling (h = k th, w = k tw; d = k td for the block rows) the input on one side of the seam
            is zeroed and the largest margin over the output voxels next to the seam on the OTHER side is taken.  Which inputs a
            neighbouring tile shares: stride 1 -- both directions (inputs >= s seen from output s - 1, inputs < s from output s);
            stride 2 -- inputs >= 2 s - pad_before from output s - 1, inputs <= 2 s - pad_before from output s (the tiles share
            ONE input plane); transposed (tiles in input voxels) -- inputs < s from output 2 s: an even output takes k = 2 of the
            input before it, nothing reaches forwards.  The margin of a case is the smallest over its seams and directions.
  padding   the forms with an input affine: out-of-volume positions hold relu(shift) instead of 0.  Smallest over the faces that
            HAVE out-of-volume taps of the largest margin on the face: all six for stride 1; for stride 2 the high faces and, where
            the input extent is odd (pad_before = 1), the low ones; for the transposed kernels the low faces only (output 2 n - 1
            takes input n - 1 alone, no kernel stages a halo behind the volume).
  stray     the forms with BatchNorm sums: one out-of-volume lane's output added to the sums.  Its value is the zero-padded
            convolution continued one position past the volume on a tiled axis (stride 1: position n takes k = 0 of plane n - 1;
            transposed: input lane n gives output 2 n its k = 2 term) -- for stride 2 every tap of such a position lies outside the
            volume and a stray lane adds exactly 0, so there the value is the face voxel counted twice (a lane clamped to the edge).
            Per stray voxel the margin is the largest over the channels and the two sums -- the GPU test asserts every channel of
            both -- and the margin of a case is the MEDIAN over the stray voxels of its three axes: a kernel that lets lanes past
            the volume into its sums adds a whole row, column or plane of them, at least half of which move the sums by this much.

Each margin must be >= 100; the smallest per row is printed (pytest -s) and recorded here as measured on the reference:

    launcher                                     seam   padding   stray   cases
    launch_out<8>                               11134       917       -       6
    launch_out<4>                               11219      1734       -       6
    launch_out<16>                              13988      2764       -       6
    conv3d_in1_kernel<8>                        27712         -       -       6
    conv3d_in1_kernel<4>                        24617         -       -       6
    conv3d_k8_kernel<32>                        41122         -       -       6
    launch_os<OS_S1, 64, 4, 2, 2, 1, 1>         29732      9302     219       7
    launch_os<OS_S1, 32, 2, 2, 2, 1, 2>         27339      9413     288       7
    launch_os<OS_S1, 128, 4, 2, 2, 1, 1>        31595     14360     577       7
    launch_c8<false>                            25335      9420     102       6
    launch_s1<32, 8, 8>                         34505      8021     107       6
    launch_s1<16, 16, 8>                        36409      9099     105       8
    launch_s1<32, 16, 8, 8, 2>                  28910      7961     104       8
    launch_s1<32, 16, 8>                        24796      8071     119       9
    launch_s1<64, 8, 16, 4, 4>                  40259      7960     107       6
    launch_s1<64, 8, 4>                         26472     10403     102      11
    launch_s1<16, 8, 8>                         29810      5683     152       6
    launch_os<OS_S2, 32, 4, 2, 2, 1, 1>         31974      7492     749       8
    launch_os<OS_S2, 64, 2, 1, 2, 1, 1>         29713      6995     527       8
    launch_os<OS_S2, 64, 4, 2, 2, 1, 1>         40740     11456     560       8
    launch_s2<32, 4>                            28230      6793     128       9
    launch_s2<16, 4>                            28222      7661     131       9
    launch_os<OS_DECONV, 64, 2, 1, 2, 1, 1>     21128      6591     195       7
    launch_os<OS_DECONV, 32, 1, 2, 2, 2, 2>     25331      5276     103       7
    launch_os<OS_DECONV, 128, 2, 1, 2, 1, 1>    26992      7863     220       7
    launch_deconv_c8<16>                        22683      5637     100       6
    launch_deconv_c8<64>                        27084      6691     112       8
    launch_deconv<32, 16, 8>                    28585      7334     106       6
    launch_deconv<16, 16, 8>                    24395      6626     107       8

The stray-lane margin is the tight one: one voxel is 1 / N of a sum that is held to rtol 1e-4, so at a few thousand voxels it is
100 bounds only where some channel's sum lies near zero.  61 of the 209 cases carry a seed other than 0 for that reason
(conv_seam_cases.SEEDS); no shape and no margin was changed.
"""
import numpy as np
import pytest

from tests import conv_seam_cases as T

MARGIN = 100.0

# The (Cin, Cout) pairs the launch lines of the dispatchers name, for a reviewer to diff against the code: (file, the line's
# instantiation, kind, Cin, Cout or the channel group its Cout is a multiple of).
LAUNCH_LINES = [
    ("conv3d_out.hip", "launch_out<8>", "s1", 8, 1),
    ("conv3d_out.hip", "launch_out<4>", "s1", 4, 1),
    ("conv3d_out.hip", "launch_out<16>", "s1", 16, 1),
    ("conv3d_c1.hip", "conv3d_in1_kernel<8>", "s1", 1, 8),
    ("conv3d_c1.hip", "conv3d_in1_kernel<4>", "s1", 1, 4),
    ("conv3d_k8.hip", "conv3d_k8_kernel<32>", "s1", 8, 32),
    ("conv3d_c8.hip", "launch_c8<false>", "s1", 32, 8),
    ("conv3d_mfma.hip", "launch_s1<32, 8, 8>", "s1", 32, 8),
    ("conv3d_mfma.hip", "launch_s1<16, 16, 8>", "s1", 16, 16),
    ("conv3d_mfma.hip", "launch_s1<32, 16, 8, 8, 2>", "s1", 32, 16),
    ("conv3d_mfma.hip", "launch_s1<32, 16, 8>", "s1", 32, 16),
    ("conv3d_mfma.hip", "launch_s1<64, 8, 16, 4, 4>", "s1", 64, 8),
    ("conv3d_mfma.hip", "launch_s1<64, 8, 4>", "s1", 64, 8),
    ("conv3d_mfma.hip", "launch_s1<16, 8, 8>", "s1", 16, 8),
    ("conv3d_os.hip", "launch_os<OS_S1, 64, 4, 2, 2, 1, 1>", "s1", 64, 64),
    ("conv3d_os.hip", "launch_os<OS_S1, 32, 2, 2, 2, 1, 2>", "s1", 32, 32),
    ("conv3d_os.hip", "launch_os<OS_S2, 32, 4, 2, 2, 1, 1>", "s2", 32, 64),
    ("conv3d_os.hip", "launch_os<OS_DECONV, 64, 2, 1, 2, 1, 1>", "tr", 64, 32),
    ("conv3d_os.hip", "launch_os<OS_DECONV, 32, 1, 2, 2, 2, 2>", "tr", 32, 16),
    ("conv3d_os.hip", "launch_os<OS_S2, 64, 2, 1, 2, 1, 1>", "s2", 64, 32),
    ("conv3d_os.hip", "launch_os<OS_S2, 64, 4, 2, 2, 1, 1>", "s2", 64, 128),
    ("conv3d_os.hip", "launch_os<OS_S1, 128, 4, 2, 2, 1, 1>", "s1", 128, 128),
    ("conv3d_os.hip", "launch_os<OS_DECONV, 128, 2, 1, 2, 1, 1>", "tr", 128, 64),
    ("conv3d_s2_mfma.hip", "launch_s2<32, 4>", "s2", 32, 16),
    ("conv3d_s2_mfma.hip", "launch_s2<16, 4>", "s2", 16, 16),
    ("deconv3d_c8.hip", "launch_deconv_c8<16>", "tr", 16, 8),
    ("deconv3d_c8.hip", "launch_deconv_c8<64>", "tr", 64, 8),
    ("deconv3d_mfma.hip", "launch_deconv<32, 16, 8>", "tr", 32, 16),
    ("deconv3d_mfma.hip", "launch_deconv<16, 16, 8>", "tr", 16, 16),
]
# named by the dispatchers, reachable only behind a launcher that refuses 2 GiB volumes: no row (conv_seam_cases' docstring)
UNREACHED_LINES = [("deconv3d_mfma.hip", "launch_deconv<16, 8, 8>", "tr", 16, 8), ("deconv3d_mfma.hip", "launch_deconv<64, 8, 8>", "tr", 64, 8)]


def test_the_table_covers_the_code():
    assert len({r.launcher for r in T.ROWS}) == len(T.ROWS)
    assert {line[1] for line in LAUNCH_LINES} == set(T.ROW_OF)
    for file, launcher, kind, cin, group in LAUNCH_LINES:
        r = T.ROW_OF[launcher]
        assert (r.file, r.kind, r.cin) == (file, kind, cin), launcher
        assert all(c % group == 0 for c in r.couts), launcher
    for file, launcher, kind, cin, cout in UNREACHED_LINES:
        assert launcher not in T.ROW_OF
        assert T.select(kind, cin, cout, "plain", 3, 9, 17) not in (launcher, None)


def test_every_case_is_selected_by_the_conditions_of_its_row():
    assert len(set(map(T.case_id, T.CASES))) == len(T.CASES)
    for c in T.CASES:
        r = T.ROW_OF[c.launcher]
        for form in r.forms:
            got = T.select(c.kind, c.cin, c.cout, form, *c.shape)
            assert got == c.launcher, (T.case_id(c), form, got)
    # the two kernels of 32 -> 8 and the plain-only kernels: the forms of a row are the ones that reach it
    assert T.select("s1", 32, 8, "fused", 5, 9, 17) != "launch_c8<false>" and T.select("s1", 32, 8, "plain", 5, 9, 17) != "launch_s1<32, 8, 8>"
    for launcher in ("conv3d_in1_kernel<8>", "conv3d_in1_kernel<4>", "conv3d_k8_kernel<32>"):
        r = T.ROW_OF[launcher]
        assert all(T.select("s1", r.cin, r.couts[0], form, *r.shapes[0]) is None for form in ("affine", "fused", "skip"))
    assert all(T.select("s1", cin, 1, form, 5, 9, 33) is None for cin in (4, 8, 16) for form in ("affine", "fused"))


def test_the_shapes_put_a_seam_on_every_tiled_axis():
    for r in T.ROWS:
        ext = [T.out_shape("s2", s) if r.kind == "s2" else s for s in r.shapes]
        for axis, t in enumerate(r.tile):
            if not t:
                assert all(e[axis] == 5 for e in ext), r.launcher
                continue
            vals = {e[axis] for e in ext}
            if axis == 0:
                assert vals == {3, 5}, r.launcher
            else:
                assert any(v > t for v in vals), r.launcher                          # a seam
                assert any(v > 2 * t for v in vals), r.launcher                      # an interior tile
        if r.kind == "s2":
            for axis in range(3):
                assert {s[axis] % 2 for s in r.shapes} == {0, 1}, r.launcher         # both values of pad_before


def test_the_refused_list_is_refused_by_the_selection_rules():
    assert len(set(T.REFUSED)) == len(T.REFUSED)
    for cin, cout, kind, form, shape in T.REFUSED:
        assert T.select(kind, cin, cout, form, *shape) is None, (cin, cout, kind, form)


def test_a_failure_names_tile_and_position():
    exp = np.ones((5, 9, 17, 4))
    got = exp.astype(np.float32)
    assert T.describe_failures("s1", (0, 8, 16), got, exp) is None
    got[2, 8, 16, 3] = np.nan                                # the one-voxel corner tile
    got[1, 7, 15, 0] = 1.001
    msg = T.describe_failures("s1", (0, 8, 16), got, exp)
    assert "2 of 765 voxels" in msg
    assert "d=2, h=8 (tile 1, pos 0 of 8), w=16 (tile 1, pos 0 of 16): channel 3" in msg
    assert "d=1, h=7 (tile 0, pos 7 of 8), w=15 (tile 0, pos 15 of 16): channel 0" in msg
    tr = T.describe_failures("tr", (2, 4, 4), np.zeros((6, 10, 10, 1), np.float32) + np.float32(1e-3) * (np.arange(10) == 9)[:, None],
                             np.zeros((6, 10, 10, 1)))
    assert "w=9 (tile 1, pos 0 of 4+1/2)" in tr and "d=0 (tile 0, pos 0 of 2+0/2)" in tr


# ---- the three margins ---------------------------------------------------------------------------------------------------------
def _axis_slice(axis, sl):
    return tuple(sl if a == axis else slice(None) for a in range(3))


def seam_margin(case, form):
    r = T.ROW_OF[case.launcher]
    inp = T.inputs_of(case)
    xin, e = T.staged_input(form, inp.arrays), inp.expect[form]
    bound = T.out_bound(e)
    worst = np.inf
    tiled = T.out_shape("s2", case.shape) if case.kind == "s2" else case.shape
    for axis, t in enumerate(r.tile):
        for s in range(t, tiled[axis], t) if t else ():
            if case.kind == "s1":
                probes = [(slice(s, None), s - 1), (slice(0, s), s)]
            elif case.kind == "s2":
                c = 2 * s - T.pad_before(case.shape[axis])
                probes = [(slice(c, None), s - 1), (slice(0, c + 1), s)]
            else:
                probes = [(slice(0, s), 2 * s)]
            for part, o in probes:
                only = np.zeros_like(xin)
                only[_axis_slice(axis, part)] = xin[_axis_slice(axis, part)]
                d = T.conv64(case.kind, only, inp.arrays["w"])
                at = _axis_slice(axis, o)
                worst = min(worst, float((np.abs(d[at]) / bound[at]).max()))
    return worst


def halo_faces(kind, shape):
    """(axis, output index) of the faces whose voxels have taps outside the volume."""
    no = T.out_shape(kind, shape)
    faces = []
    for axis in range(3):
        if kind == "s1" or kind == "tr" or shape[axis] % 2:
            faces.append((axis, 0))
        if kind != "tr":
            faces.append((axis, no[axis] - 1))
    return faces


def padding_margin(case, form):
    inp = T.inputs_of(case)
    e = inp.expect[form]
    h = np.maximum(inp.arrays["sh"].astype(np.float64), 0)
    e_off = {"s1": 1, "s2": 2, "tr": 1}[case.kind]           # the volume's offset inside the padded one (even for stride 2)
    big = np.empty(tuple(n + 2 * e_off for n in case.shape) + (case.cin,))
    big[...] = h
    big[e_off:-e_off, e_off:-e_off, e_off:-e_off] = 0
    o_off = {"s1": 1, "s2": 1, "tr": 2}[case.kind]
    d = T.conv64(case.kind, big, inp.arrays["w"])[tuple(slice(o_off, o_off + n) for n in e.shape[:3])]
    assert d.shape == e.shape
    ratio = np.abs(d) / T.out_bound(e)
    faces = halo_faces(case.kind, case.shape)
    silent = [(a, i) for a in range(3) for i in (0, e.shape[a] - 1) if (a, i) not in faces]
    assert all(not d[_axis_slice(a, i)][(slice(1, -1),) * 2].any() for a, i in silent)       # (face interiors: no taps outside)
    return min(float(ratio[_axis_slice(a, i)].max()) for a, i in faces)


def stray_margin(case, form):
    r = T.ROW_OF[case.launcher]
    inp = T.inputs_of(case)
    xin, e = T.staged_input(form, inp.arrays), inp.expect[form]
    bound = T.sum_bound(T.sums_of(e))
    if case.kind == "s2":
        ext = None
    else:                                                    # the zero-padded convolution one position past every high face
        more = np.zeros(tuple(n + 1 for n in case.shape) + (case.cin,))
        more[:-1, :-1, :-1] = xin
        ext = T.conv64(case.kind, more, inp.arrays["w"])
    per_voxel = []
    for axis in range(3):
        n = e.shape[axis]
        if ext is None:
            v = e[_axis_slice(axis, n - 1)]
        else:                                                # position n of this axis, inside the volume on the other two
            rows, cols = (m for a, m in enumerate(e.shape[:3]) if a != axis)
            v = np.take(ext, n, axis=axis)[:rows, :cols]
        v = v.reshape(-1, e.shape[-1])
        per_voxel.append(np.maximum(np.abs(v) / bound[0], v ** 2 / bound[1]).max(axis=1))
    return float(np.median(np.concatenate(per_voxel)))


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.launcher.replace(" ", ""))
def test_a_seam_defect_is_a_hundred_times_the_bound(row):
    seam, pad, stray = {}, {}, {}
    for c in (c for c in T.CASES if c.launcher == row.launcher):
        for form in row.forms:
            aff, _, sums = T.form_has(form)
            key = (T.case_id(c), form)
            m = seam_margin(c, form)
            if np.isfinite(m):
                seam[key] = m
            if aff:
                pad[key] = padding_margin(c, form)
            if sums:
                stray[key] = stray_margin(c, form)
    low = lambda d: min(d.values()) if d else float("nan")
    print("margins %-42s seam %9.0f  padding %9.0f  stray %9.0f   (%d cases)"
          % (row.launcher, low(seam), low(pad), low(stray), len({k[0] for k in seam})))
    assert seam, "no case of the row has a seam"
    for name, d in (("seam", seam), ("padding", pad), ("stray lane", stray)):
        short = {k: v for k, v in d.items() if not v >= MARGIN}
        assert not short, "%s margin below %g: %s" % (name, MARGIN, short)
