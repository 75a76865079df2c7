"""BatchNorm (batch statistics) + ReLU backward -- bn_bwd_reduce_kernel and bn_bwd_apply_kernel of backward.hip behind
backward.bn_relu_bwd -- at the seams of its launches, element by element against the closed form in numpy float64.

Both kernels give a lane one channel quad and walk n4 = voxels x C / 4 quads in workgroups of 256 with a grid-stride loop; `reduce`
caps its grid at 1024 workgroups, `apply` at 4096; every workgroup of `reduce` adds its float64 sums into slot blockIdx.x % 32 and
`apply` folds the 32 slots.  Cases: C in {4, 8, 16, 32, 64} (C / 4 = 1 .. 16 quads per voxel), with and without a second gradient,
at
  one        1 voxel: a single workgroup with 1 .. 16 live lanes (batch variance 0);
  below      256 - C / 4 quads: one partial workgroup (255 quads at C = 4);
  above      256 + C / 4 quads: a count that is no multiple of 256, the second workgroup almost empty (257 quads at C = 4);
  wrap       35 x 256 + 3 C / 4 quads: 36 workgroups, slots 0 .. 3 are added into twice, the last workgroup is partial;
and, one volume per grid cap,
  reduce cap C = 32, 32773 voxels: 1024 x 256 + 40 quads -- `reduce` takes a second trip of its loop in its first workgroup;
  apply cap  C = 64, 16 x 64 x 66 voxels: 1081344 quads > 4096 x 256 -- `apply` takes a second trip too (17 MB per tensor).

The reference is the closed form, not autograd (no autograd at the large sizes): z = y scale + shift with the batch moments,
gz = (g1 + g2) [z > 0], g_beta = sum gz, g_gamma = sum gz xhat, g_y = gamma inv_std (gz - g_beta / n - xhat g_gamma / n).  The
ReLU's sign: a float32 z may differ in sign from the float64 one where |z| is tiny, so the INPUT is moved -- y is shifted by 0.01
wherever the float64 |z| < 1e-4, again until no such element is left (the moments move with it) -- and nothing is masked in the
comparison: every element of g_y is held.  beta keeps 0.05 <= |beta| so that the 1-voxel case (z = beta) is clear of it as well.

Bounds: g_y by tensor_distance (tests/_helpers.py), g_gamma and g_beta per channel by the same measure over the C channels, each
within 3 x the FLOOR: the largest distance, over all cases of this file, of a float32 numpy restatement of the closed form
(float32 moments, mask, sums by numpy's pairwise float32 sum, g_y) from float64.  Where the reference is exactly zero (1 voxel: g_y
and g_gamma vanish identically) the result must be exactly zero.  Measured on an MI355X:

                 float32 floor   bound      device, worst case of  one     below    above    wrap     reduce cap  apply cap
    g_y          1.56e-07        4.68e-07                          0       1.2e-07  1.6e-07  1.6e-07  1.4e-07     1.3e-07
    g_gamma      6.46e-06        1.94e-05                          0       1.4e-07  1.3e-07  9.4e-08  5.6e-08     6.6e-08
    g_beta       5.29e-06        1.59e-05                          4.8e-08 5.3e-08  5.0e-08  4.9e-08  4.0e-08     4.3e-08

(The two sums' floors come from the cap volumes, where numpy's float32 pairwise sum over 3e4 .. 7e4 terms is a hundred times
coarser than the kernels' float64 slots; a workgroup's sums lost or added twice would move a channel by 1 / 36 and more.)
C = 12 (3 quads per voxel do not divide the workgroup) is refused by both entries and C = 128 by `apply` (its folded sums have 64
channels of LDS; `reduce` alone takes 128): MVS_E_SHAPE, outputs untouched.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 3.0
EPS = 1e-5
MVS_E_SHAPE = -2

SMALL = {"one": lambda cq: 1, "below": lambda cq: 256 // cq - 1, "above": lambda cq: 256 // cq + 1,
         "wrap": lambda cq: (35 * 256) // cq + 3}
CASES = [(C, two, name, SMALL[name](C // 4)) for C in (4, 8, 16, 32, 64) for two in (False, True) for name in SMALL]
CASES += [(32, two, "reduce-cap", 1024 * 256 // 8 + 5) for two in (False, True)]
CASES += [(64, two, "apply-cap", 16 * 64 * 66) for two in (False, True)]
IDS = ["C%d-%s-%s-%d" % (C, "g1g2" if two else "g1", name, vox) for C, two, name, vox in CASES]


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    from mvsnet_amd import _lib as L
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def moments(y):
    """-> float64 stats (2, C) as the forward kernels emit them, mean, 1 / sqrt(biased variance + eps)."""
    y64 = y.astype(np.float64)
    stats = np.stack([y64.sum(0), (y64 ** 2).sum(0)])
    mu = stats[0] / y.shape[0]
    var = np.maximum(stats[1] / y.shape[0] - mu * mu, 0.0)
    return stats, mu, 1.0 / np.sqrt(var + EPS)


def inputs(C, two, vox):
    """-> y (vox, C), gamma, beta, g1, g2 or None: float32, seeded per case, y moved off the ReLU's edge (the docstring)."""
    rs = np.random.RandomState(C * 7 + two + vox % 1000)
    y = (rs.standard_normal((vox, C)) * 1.5 + 0.3).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32)
    beta = (rs.uniform(0.05, 0.3, C) * rs.choice([-1.0, 1.0], C)).astype(np.float32)
    g1 = rs.standard_normal((vox, C)).astype(np.float32)
    g2 = rs.standard_normal((vox, C)).astype(np.float32) if two else None
    for _ in range(8):
        _, mu, inv = moments(y)
        near = np.abs((y.astype(np.float64) - mu) * inv * gamma + beta) < 1e-4
        if not near.any():
            break
        y[near] += np.float32(0.01)
    else:
        raise AssertionError("elements stay within 1e-4 of the ReLU's edge")
    return y, gamma, beta, g1, g2


def closed_form(y, gamma, beta, g1, g2, dtype):
    """(g_y, g_gamma, g_beta) of BatchNorm + ReLU with every operation in `dtype`; the moments and gamma inv_std come from the float64
    sums and are rounded once, as on the device."""
    n = dtype(y.shape[0])
    _, mu64, inv64 = moments(y)
    k64 = gamma.astype(np.float64) * inv64
    scale, shift = k64.astype(dtype), (beta - mu64 * k64).astype(dtype)
    mu, inv, k0 = mu64.astype(dtype), inv64.astype(dtype), k64.astype(dtype)
    yy = y.astype(dtype)
    g = g1.astype(dtype) if g2 is None else g1.astype(dtype) + g2.astype(dtype)
    gz = np.where(yy * scale + shift > 0, g, dtype(0))
    xhat = (yy - mu) * inv
    s1, s2 = gz.sum(0, dtype=dtype), (gz * xhat).sum(0, dtype=dtype)
    g_y = k0 * (gz - s1 / n - xhat * (s2 / n))
    assert g_y.dtype == dtype and s1.dtype == dtype
    return g_y.astype(np.float64), s2.astype(np.float64), s1.astype(np.float64)


def distance(got, ref):
    """tensor_distance, or the largest |got| where the reference is identically zero."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    return float(np.abs(got - ref).max() / top) if top > 0 else float(np.abs(got).max())


@functools.lru_cache(maxsize=None)
def floor_of(C, two, vox):
    """The float32 restatement's three distances from float64 and whether each reference is identically zero."""
    args = inputs(C, two, vox)
    ref = closed_form(*args, np.float64)
    f32 = closed_form(*args, np.float32)
    return tuple(distance(a, b) for a, b in zip(f32, ref)), tuple(not np.any(r) for r in ref)


@pytest.fixture(scope="module")
def bounds():
    floor = [0.0, 0.0, 0.0]
    for C, two, _name, vox in CASES:
        d, zero = floor_of(C, two, vox)
        for k in range(3):
            if zero[k]:
                assert d[k] == 0.0
            else:
                floor[k] = max(floor[k], d[k])
    print("\nBatchNorm backward: float32 floors g_y %.3e g_gamma %.3e g_beta %.3e" % tuple(floor))
    return [MARGIN * f for f in floor]


@pytest.mark.parametrize("C,two,name,vox", CASES, ids=IDS)
def test_bn_relu_backward_matches_the_closed_form(C, two, name, vox, bounds):
    from mvsnet_amd import backward as B
    from mvsnet_amd import model as M
    y, gamma, beta, g1, g2 = inputs(C, two, vox)
    ref = closed_form(y, gamma, beta, g1, g2, np.float64)
    t = lambda a: torch.as_tensor(a).to(DEV) if a is not None else None
    stats = t(moments(y)[0])
    aff = M.bn_finalize(stats, vox, t(gamma), t(beta))
    got = B.bn_relu_bwd(t(y), stats, aff, t(gamma), t(g1), t(g2))
    torch.cuda.synchronize()
    got = [g.cpu().numpy() for g in got]
    assert got[0].shape == (vox, C) and got[1].shape == got[2].shape == (C,)
    dist = [distance(g, r) for g, r in zip(got, ref)]
    print("\n%s: n4 %d, workgroups %d | g_y %.3e (bound %.3e) g_gamma %.3e (%.3e) g_beta %.3e (%.3e)"
          % (name, vox * C // 4, -(-vox * C // 4 // 256), dist[0], bounds[0], dist[1], bounds[1], dist[2], bounds[2]))
    for k, what in enumerate(("g_y", "g_gamma", "g_beta")):
        if not np.any(ref[k]):
            assert dist[k] == 0.0, (what, dist[k])
        else:
            assert dist[k] <= bounds[k], (what, dist[k], bounds[k])


@pytest.mark.parametrize("C,entries", [(12, ("reduce", "apply")), (128, ("apply",))])
def test_refused_channel_counts_answer_shape_errors_and_write_nothing(C, entries):
    from mvsnet_amd import _lib as L
    lib = L.load()
    vox = 40
    rs = np.random.RandomState(C)
    mk = lambda *s: torch.as_tensor(rs.standard_normal(s).astype(np.float32)).to(DEV)
    y, g1, scale, shift, gamma = mk(vox, C), mk(vox, C), mk(C), mk(C), mk(C)
    stats = torch.stack([y.double().sum(0), (y.double() ** 2).sum(0)]).contiguous()
    sums = torch.full((lib.mvs_bn_bwd_sum_slots(), 2, C), 3.5, device=DEV, dtype=torch.float64)
    g_y = torch.full((vox, C), 7.25, device=DEV)
    g_gamma, g_beta = torch.full((C,), 7.25, device=DEV), torch.full((C,), 7.25, device=DEV)
    if "reduce" in entries:
        rc = lib.mvs_bn_bwd_reduce_f32(L.ptr(y), L.ptr(stats), float(vox), EPS, L.ptr(scale), L.ptr(shift), L.ptr(g1), None, vox, C,
                                       L.ptr(sums), L.stream_ptr())
        assert rc == MVS_E_SHAPE
    rc = lib.mvs_bn_bwd_apply_f32(L.ptr(y), L.ptr(stats), float(vox), EPS, L.ptr(scale), L.ptr(shift), L.ptr(gamma), L.ptr(g1), None,
                                  L.ptr(sums), vox, C, L.ptr(g_y), L.ptr(g_gamma), L.ptr(g_beta), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == MVS_E_SHAPE
    assert bool((sums == 3.5).all()) and bool((g_y == 7.25).all()) and bool((g_gamma == 7.25).all()) and bool((g_beta == 7.25).all())
