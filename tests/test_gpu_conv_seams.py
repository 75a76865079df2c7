"""Every 3-D convolution launcher at the seams of its own tiling, against the float64 oracle, inside the poisoned, guarded arena.

The cases, their shapes and inputs are tests/conv_seam_cases.py (one row per launcher instantiation behind mvs_conv3d_f32 /
mvs_deconv3d_f32; the table is that module's docstring); tests/test_conv_seam_cases_host.py shows from the reference alone that at
every case a wrong seam, a halo staged as relu(shift) or a lane past the volume in the BatchNorm sums is at least 100 times the
bounds used here.  Per case and form of the row:

  1. conv impl `mfma` -- the entry returns the launcher's code and never falls back to the shape-generic kernel -- must succeed;
     its output is held to the oracle at test_gpu_parity's bounds for these layers (rtol 1e-4, atol 2e-5; the two BatchNorm sums
     rtol 1e-4, atol 1e-3) and mvs_bn_finalize_f32 of the sums as in test_gpu_arena.check_conv_case;
  2. `auto` gives the same output bit for bit and the same sums up to the order of the float64 atomics
     (test_gpu_halo_planes.sums_equal): `auto` did not fall back;
  3. `scalar` meets the same oracle bounds at the same shape: a failure reads as "kernel" or as "oracle".
A failure names the voxels by tile index and position in the tile on every tiled axis.  The REFUSED combinations answer
MVS_E_SHAPE under `mfma` and leave the output's poison in place, and meet the oracle bounds under `auto`.

Whole-network shapes for what only prepared weights reach (os_block<.., PREP = true>, the filled launches of 3dconv3_0 / 3_1 / 4_0
with 3dconv2_1's blocks behind them, the fused 3dconv1_1 + 2_0 launch, the Winograd pair): RegNetUS0 through the entries
`prepared`, `plain` and `batch` at three volumes, held as test_gpu_parity.test_regnet_auto_mode_on_small_odd_volumes holds its
own (rel-L1 < 2e-5, rtol 1e-3, atol 2e-4).  Extents per level and how each kernel's tiles split them:

    volume        level  extents       8x32 pair / output conv   8x16 (1_1 + 2_0, 6_0)   2x4x8 (2_1)       2x8x8 (5_0)     2x4x4 (3_0, 3_1, 4_0)
    (40,24,72)    1      (40,24,72)    H 8|8|8  W 32|32|8
                  1/2    (20,12,36)                              H 8|4  W 16|16|4
                  1/4    (10,6,18)                                                       D 2x5 H 4|2 W 8|8|2  D 2x5 H 6 W 8|8|2
                  1/8    (5,3,9)                                                                                          D 2|2|1 H 3 W 4|4|1
    (24,72,40)    1      (24,72,40)    H 8x9  W 32|8
                  1/2    (12,36,20)                              H 8x4|4  W 16|4
                  1/4    (6,18,10)                                                       D 2x3 H 4x4|2 W 8|2  D 2x3 H 8|8|2 W 8|2
                  1/8    (3,9,5)                                                                                          D 2|1 H 4|4|1 W 4|1
    (72,40,24)    1      (72,40,24)    H 8x5  W 24
                  1/2    (36,20,12)                              H 8|8|4  W 12
                  1/4    (18,10,6)                                                       D 2x9 H 4|4|2 W 6    D 2x9 H 8|2 W 6
                  1/8    (9,5,3)                                                                                          D 2x4|1 H 4|1 W 3
Between them every tiled axis of every one of these kernels sees two full tiles or blocks and a remainder at its own level (depth
at 1/4 is even for every volume the network takes: blocks of 2 planes never leave one there).  At (40,24,72) the route is pinned
as test_gpu_parity.test_regnet_routes_are_the_recorded_ones pins its own: 1_0, 2_0 and 2_1 report no launch of their own.
"""
import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L

from tests import conv_seam_cases as T
from tests import test_gpu_parity as P
from tests.device_arena import PATTERNS, Arena
from tests.test_gpu_arena import check_regnet
from tests.test_gpu_halo_planes import sums_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"
BN_EPSILON = 1e-5
F32, F64 = torch.float32, torch.float64
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


class Operands:
    """One case's operands, read-only inside an arena sized for them and for `runs` outputs."""

    def __init__(self, pattern, kind, cin, cout, shape, arrays, runs):
        self.kind, self.cin, self.cout, self.shape = kind, cin, cout, shape
        self.oshape = T.out_shape(kind, shape) + (cout,)
        nbytes = sum(v.nbytes for v in arrays.values()) + runs * (4 * int(np.prod(self.oshape)) + 16 * cout)
        self.a = Arena(nbytes + (len(arrays) + 4 * runs + 4) * (2 * 64 * 1024 + 512) + (1 << 20), pattern, DEV)
        self.t = {k: self.a.take(v.shape, F32, data=np.ascontiguousarray(v), readonly=True, name=k) for k, v in arrays.items()}

    def run(self, form, impl, tag):
        """-> (return code, output tensor, float64 sums tensor or None) of the entry point under conv impl `impl`."""
        lib, t, a = L.load(), self.t, self.a
        aff, skip, sums = T.form_has(form)
        y = a.take(self.oshape, F32, name="y_%s" % tag)
        stats = None
        if sums:
            stats = a.take((2, self.cout), F64, name="stats_%s" % tag)
            L.check(lib.mvs_zero_f64(L.ptr(stats), stats.numel(), L.stream_ptr()), "mvs_zero_f64")
        xs, xb = (t["sc"], t["sh"]) if aff else (None, None)
        x2, x2s, x2b = (t["x2"], t["sc2"], t["sh2"]) if skip else (None, None, None)
        D, H, W = self.shape
        head = (L.ptr(t["x"]), L.ptr(xs), L.ptr(xb), L.ptr(x2), L.ptr(x2s), L.ptr(x2b), L.ptr(t["w"]), D, H, W, self.cin, self.cout)
        L.set_conv_impl(impl)
        try:
            if self.kind == "tr":
                rc = lib.mvs_deconv3d_f32(*head, L.ptr(y), L.ptr(stats), L.stream_ptr())
            else:
                rc = lib.mvs_conv3d_f32(*head, 2 if self.kind == "s2" else 1, L.ptr(y), L.ptr(stats), L.stream_ptr())
            torch.cuda.synchronize()
        finally:
            L.set_conv_impl("auto")
        return rc, y, stats

    def finalize(self, stats, count, tag):
        scale, shift = self.a.take((self.cout,), F32, name="scale_%s" % tag), self.a.take((self.cout,), F32, name="shift_%s" % tag)
        L.check(L.load().mvs_bn_finalize_f32(L.ptr(stats), self.cout, float(count), L.ptr(self.t["gamma"]), L.ptr(self.t["beta"]),
                                             BN_EPSILON, L.ptr(scale), L.ptr(shift), L.stream_ptr()), "mvs_bn_finalize_f32")
        return n(scale), n(shift)


def hold(kind, tile, what, y, stats, exp):
    """The oracle bounds: outputs voxel by voxel (a failure names tiles and positions), then the two sums."""
    msg = T.describe_failures(kind, tile, y, exp)
    assert msg is None, "%s\n%s" % (what, msg)
    if stats is not None:
        s = T.sums_of(exp)
        np.testing.assert_allclose(stats[0], s[0], rtol=T.SUM_RTOL, atol=T.SUM_ATOL, err_msg=what + ": sums")
        np.testing.assert_allclose(stats[1], s[1], rtol=T.SUM_RTOL, atol=T.SUM_ATOL, err_msg=what + ": sums of squares")


@both_patterns
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_conv3d_seams(case, pattern):
    row = T.ROW_OF[case.launcher]
    inp = T.inputs_of(case)
    ops = Operands(pattern, case.kind, case.cin, case.cout, case.shape, inp.arrays, 3 * len(row.forms))
    for form in row.forms:
        exp = inp.expect[form]
        what = "%s %s" % (T.case_id(case), form)
        rc, y, stats = ops.run(form, "mfma", form + "_mfma")
        assert rc == 0, "%s: conv impl mfma answered %d: %s did not take the shape" % (what, rc, case.launcher)
        y_m, st_m = n(y), (n(stats) if stats is not None else None)
        hold(case.kind, row.tile, what + " mfma", y_m, st_m, exp)
        if stats is not None:
            scale, shift = ops.finalize(stats, exp.size // case.cout, form)
            np.testing.assert_allclose(np.maximum(exp * scale + shift, 0), inp.bn[form], rtol=1e-4, atol=1e-5, err_msg=what)

        rc, y, stats = ops.run(form, "auto", form + "_auto")
        assert rc == 0, what
        y_a = n(y)
        if not np.array_equal(y_a, y_m):
            raise AssertionError("%s: auto differs from mfma (a fall-back to the shape-generic kernel?)\n%s"
                                 % (what, T.describe_failures(case.kind, row.tile, y_a, y_m.astype(np.float64), 0, 0)))
        if stats is not None:
            sums_equal(n(stats), st_m, y_m)

        rc, y, stats = ops.run(form, "scalar", form + "_scalar")
        assert rc == 0, what
        hold(case.kind, row.tile, what + " scalar", n(y), n(stats) if stats is not None else None, exp)
    ops.a.check()


@both_patterns
@pytest.mark.parametrize("refused", T.REFUSED, ids=lambda r: "%dto%d-%s-%s" % r[:4])
def test_conv3d_refused_shapes(refused, pattern):
    cin, cout, kind, form, shape = refused
    inp = T.case_inputs(kind, cin, cout, shape)
    ops = Operands(pattern, kind, cin, cout, shape, inp.arrays, 2)
    what = "%d -> %d %s %s %s" % (cin, cout, kind, form, shape)
    rc, y, stats = ops.run(form, "mfma", "mfma")
    assert rc == T.MVS_E_SHAPE, "%s: conv impl mfma answered %d" % (what, rc)
    assert ops.a.is_pattern(y), what + ": a refused call wrote to its output"
    rc, y, stats = ops.run(form, "auto", "auto")
    assert rc == 0, what
    hold(kind, (0, 0, 0), what + " auto", n(y), n(stats) if stats is not None else None, inp.expect[form])
    ops.a.check()


# ---- whole-network shapes for the kernels that only prepared weights reach -------------------------------------------------------
SEAM_VOLUMES = [(40, 24, 72), (24, 72, 40), (72, 40, 24)]


@both_patterns
@pytest.mark.parametrize("entry", ["prepared", "plain", "batch"])
@pytest.mark.parametrize("shape", SEAM_VOLUMES, ids=lambda s: "x".join(map(str, s)))
def test_regnet_seam_volumes(shape, entry, pattern):
    check_regnet("normal", shape, entry, pattern)


def test_regnet_seam_volume_takes_the_prepared_route():
    """The filled launches and the fused 3dconv1_1 + 2_0 launch really ran at (40,24,72)."""
    P.test_regnet_routes_are_the_recorded_ones("prepared", "auto", {}, SEAM_VOLUMES[0], {"1_0", "2_0", "2_1"})
