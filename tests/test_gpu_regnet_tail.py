"""The regulariser's tail: the BatchNorm fold done once per consumer workgroup, the partial-row counts picked with it, and
3dconv6_2 over forced chunk lengths.

Library hooks: MVS_HOOK_OUT_PLANES, MVS_HOOK_BN_SLOTS, MVS_HOOK_PAIR_SLOTS.  The routes are held to the float64 oracle at the
bound the older tests of the same entry point use (tests/test_gpu_parity.py).
"""
import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from mvsnet_amd import synthetic as S
from mvsnet_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


# ---- 3dconv6_2 through the single-layer entry -------------------------------------------------------------------------
OUT_SHAPES = [(16, 16, 48), (9, 10, 40), (5, 8, 32)]
_out_cases = {}


def out_case(shape):
    """Inputs and the float64 expectation of one shape, computed once: Cin = 8 -> 1, both inputs with a finalised affine."""
    if shape not in _out_cases:
        D, H, W = shape
        rs = np.random.RandomState(D * 1000 + H * 10 + W)
        x = rs.standard_normal((D, H, W, 8)).astype(np.float32)
        x2 = rs.standard_normal((D, H, W, 8)).astype(np.float32)
        wgt = (rs.standard_normal((3, 3, 3, 8, 1)) / np.sqrt(27 * 8)).astype(np.float32)
        sc = (1 + 0.3 * rs.standard_normal(8)).astype(np.float32); sh = (0.2 * rs.standard_normal(8)).astype(np.float32)
        sc2 = (1 + 0.3 * rs.standard_normal(8)).astype(np.float32); sh2 = (0.2 * rs.standard_normal(8)).astype(np.float32)
        xin = np.maximum(x * sc + sh, 0).astype(np.float64) + np.maximum(x2 * sc2 + sh2, 0)
        exp = O.conv3d_same(xin, wgt, 1, np.float64)
        exp.setflags(write=False)
        _out_cases[shape] = (x, x2, wgt, sc, sh, sc2, sh2, exp)
    return _out_cases[shape]


@pytest.mark.parametrize("planes", [16, 5, 3, 1])
@pytest.mark.parametrize("shape", OUT_SHAPES)
def test_out_conv_plane_chunks_match_oracle(shape, planes):
    """Planes per workgroup 16 / 5 / 3 / 1 over depths 16 / 9 / 5: one chunk and several, forwards and backwards marches,
    marches of three planes, H and W that are no multiples of the 8 x 32 tile."""
    from mvsnet_amd.model import conv3d
    x, x2, wgt, sc, sh, sc2, sh2, exp = out_case(shape)
    with L.test_hooks(out_planes=planes):
        got = n(conv3d(t(x), t(wgt), 1, (t(sc), t(sh)), t(x2), (t(sc2), t(sh2))))
    assert got.shape == exp.shape
    print("out conv %s planes %d: max |got - oracle| = %.3g" % (shape, planes, np.abs(got - exp).max()))
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=2e-5)


# ---- the whole regulariser: default partial rows against one row ------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16, 32), (24, 24, 48), (8, 8, 8)])
def test_regnet_default_rows_against_one_row_and_oracle(shape):
    """mvs_regnet_us0_prepared_f32 with the built-in row counts, with every layer's sums in ONE row (hooks bn_slots = 1,
    pair_slots = 1) and in eight: each against the float64 oracle at the bound of test_regnet_matches_oracle.  The runs add the same
    float64 terms in another order, so they may differ in last bits; two results inside the oracle's bound could be twice the
    bound apart, they are held to once the bound."""
    from mvsnet_amd.model import RegNetWeights, regnet_us0
    D, H, W = shape
    params = S.make_regnet_params("normal", seed=31, random_affine=True)
    rs = np.random.RandomState(32 + D)
    cost = np.abs(rs.standard_normal((D, H, W, 32))).astype(np.float32)
    wts = RegNetWeights(params, DEV)
    exp = O.regnet_us0(cost, params, np.float64)
    dflt = n(regnet_us0(t(cost), wts))
    with L.test_hooks(bn_slots=1, pair_slots=1):
        one = n(regnet_us0(t(cost), wts))
    with L.test_hooks(bn_slots=8, pair_slots=8):
        eight = n(regnet_us0(t(cost), wts))
    print("regnet %s: max |default - one row| = %.3g, |eight rows - one row| = %.3g, |default - oracle| = %.3g"
          % (shape, np.abs(dflt - one).max(), np.abs(eight - one).max(), np.abs(dflt - exp).max()))
    for got in (dflt, one, eight):
        np.testing.assert_allclose(got, exp, rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(dflt, one, rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(eight, one, rtol=1e-3, atol=2e-4)
