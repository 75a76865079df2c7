"""Every plane count mvs_softargmin_prob_f32 branches on, and its backward, against the float64 oracle.

softargmin.hip takes the LDS tile kernel (32 pixels x 16 plane groups per block, the D x 32 column tile in dynamic LDS) while
D * 32 * 4 <= 60 KB, that is D <= 480, and the plain kernel (64 pixels x 4 plane groups) above.  What each D reaches:

    1, 2, 15      fewer planes than the tile kernel has plane groups (idle groups carry -inf / 0 into the combine)
    16, 17        one plane per group; the first group with two
    63, 64, 65    the four-loads-per-trip loop needs D > 48 + g: it runs for groups 0..14 / all 16 / all, and at 65 group 0 has a tail plane
    129           two trips and a tail
    479, 480      the largest tiles; 480 asks for 61 440 B of dynamic LDS beside 4 096 B of static LDS: exactly 64 KB
    481, 500      the plain kernel
3 x 40 = 120 pixels: the last block of either kernel (32 / 64 pixels) is ragged.  Both kernels are right on either side of 480 (an
MI355X launches the tile kernel with more than 64 KB of LDS as well), so WHERE the launcher switches is pinned by the order of
the kernels' float32 sums: test_softargmin_takes_the_tile_kernel_up_to_480_planes_and_the_plain_kernel_above.

Inputs: reg = 2 N(0,1), one near-one-hot pixel.  A regressed depth whose plane index lies within the depth bound of an integer
may take the neighbouring buckets of the probability map on the device; the seed of every case is therefore the first one whose
float64 index stays INDEX_MARGIN away from every integer at every pixel but the one-hot one (a property of the reference alone;
the margin is asserted to cover the movement the depth bound allows).  The one-hot pixel sits on an integer index by construction:
there the device's float32 arithmetic is the float32 oracle's, operation for operation, and the float32 oracle chooses the
float64 oracle's buckets (asserted per case).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import mvsnet_oracle as O
from mvsnet_amd import _lib as L

from tests.device_arena import PATTERNS, Arena

pytestmark = pytest.mark.gpu

DEV = "cuda"
PLANE_COUNTS = [1, 2, 15, 16, 17, 63, 64, 65, 129, 479, 480, 481, 500]
BACKWARD_PLANE_COUNTS = [1, 2, 17, 65, 481]
H, W = 3, 40
START, INTERVAL = 425.0, 2.65
HOT = (1, 4)                                 # the near-one-hot pixel
INDEX_MARGIN = 0.01


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


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


def plane_index(depth, D, inverse):
    """Float64 plane index of a depth, as probability_map computes it (counted from the far end for inverse depth)."""
    if D == 1:
        return np.zeros_like(depth)
    if inverse:
        end = START + (D - 1.0) * INTERVAL
        return (1.0 / depth - 1.0 / end) / ((1.0 / START - 1.0 / end) / (D - 1.0))
    return (depth - START) / INTERVAL


def oracle(reg, D, inverse, dtype):
    with np.errstate(all="ignore"):          # D = 1 with inverse depth: the reference's index is 0 / 0, every bucket clamps to plane 0
        return O.softargmin_and_prob(reg, D, START, INTERVAL, inverse, dtype)


@functools.lru_cache(maxsize=None)
def forward_case(D, inverse, hot=True):
    """-> reg (D,H,W) float32, float64 depth and prob, float32-oracle depth and prob, seed.  Read-only."""
    for seed in range(1000):
        rs = np.random.RandomState(10000 * D + 100 * int(inverse) + seed)
        noise = (2.0 * rs.standard_normal((D, H, W))).astype(np.float32)
        # the one-hot plane: the first from plane 7 on at which the float32 oracle takes the float64 oracle's buckets (the index
        # is an integer there up to the last bit of either precision)
        for k in range(min(7, D - 1), min(15, D)) if hot else (None,):
            reg = noise.copy()
            if hot:
                reg[k, HOT[0], HOT[1]] = -60.0
            ed, ep = oracle(reg, D, inverse, np.float64)
            idx = plane_index(ed, D, inverse)
            away = np.abs(idx - np.round(idx))
            if hot:
                away[HOT] = 1.0
            if D > 2 and away.min() <= INDEX_MARGIN:         # (1 or 2 planes: the clamps leave one choice of buckets)
                break                                        # another seed
            d32, p32 = oracle(reg, D, inverse, np.float32)
            if (np.abs(p32 - ep) <= 1e-5).all():
                for a in (reg, ed, ep, d32, p32):
                    a.setflags(write=False)
                return reg, ed, ep, d32, p32, seed
    raise AssertionError("no seed keeps the plane indices away from the integers")


def depth_bound(D, inverse):
    """-> (E, bound): E = the float32 oracle's largest relative depth error against float64; the kernel is held to max(2e-6, 4 E) --
    2e-6 is the bound of test_softargmin_prob_matches_oracle at D = 48, the factor 4 the one the sweep tests allow a device over the
    float32 reference (tests/sweep_reference.py).  Neither comes from the kernel.  Measured: E = 3.4e-7 at D = 17, 1.1e-6 at 480,
    1.6e-6 at 500 (inverse), so the bound is 2e-6 up to D = 17 and 4.3e-6 .. 6.5e-6 from 479 on; the kernels stay below 4.7e-7
    everywhere (table in test_softargmin_prob_at_every_plane_count)."""
    _reg, ed, _ep, d32, _p32, _seed = forward_case(D, inverse)
    E = float((np.abs(d32.astype(np.float64) - ed) / ed).max())
    return E, max(2e-6, 4.0 * E)


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["linear", "inverse"])
@pytest.mark.parametrize("D", PLANE_COUNTS)
def test_softargmin_prob_at_every_plane_count(D, inverse):
    """Depth within max(2e-6, 4 E) of the float64 oracle, relative (depth_bound); at most 5e-3 of the pixels -- of 120, none -- with
    a probability off by more than 1e-5.  Measured on an MI355X, largest relative depth error, linear / inverse sampling:

        D      E (float32 oracle)     kernel                  D      E (float32 oracle)     kernel
        1      0       / 7.2e-8       0      / 7.2e-8         65     5.5e-7 / 6.0e-7        2.8e-7 / 3.4e-7
        2      1.3e-7  / 1.5e-7       1.5e-7 / 1.5e-7         129    7.0e-7 / 6.9e-7        2.5e-7 / 3.2e-7
        15     2.4e-7  / 3.0e-7       2.5e-7 / 3.1e-7         479    1.1e-6 / 1.3e-6        3.3e-7 / 4.2e-7
        16     2.6e-7  / 2.4e-7       2.3e-7 / 2.7e-7         480    1.1e-6 / 1.3e-6        4.2e-7 / 2.6e-7
        17     3.4e-7  / 2.7e-7       3.1e-7 / 2.8e-7         481    1.2e-6 / 1.3e-6        3.6e-7 / 4.6e-7
        63     6.2e-7  / 4.5e-7       3.8e-7 / 3.0e-7         500    1.2e-6 / 1.6e-6        3.3e-7 / 4.2e-7
        64     4.5e-7  / 5.4e-7       3.1e-7 / 3.1e-7

    The oracle's error grows with D (one running sum over all planes); the kernels' does not (16 or 4 partial sums).  No pixel's
    probability was off by more than 2.4e-7."""
    from mvsnet_amd.model import softargmin_prob
    reg, ed, ep, d32, p32, seed = forward_case(D, inverse)
    E, bound = depth_bound(D, inverse)
    # preconditions, from the reference alone
    assert (~(np.abs(p32 - ep) <= 1e-5)).sum() == 0, "the float32 oracle itself takes other buckets"
    if D > 2:
        idx = plane_index(ed, D, inverse)
        moved = max(float(np.abs(plane_index(ed * (1.0 + s * bound), D, inverse) - idx).max()) for s in (-1.0, 1.0))
        assert moved < INDEX_MARGIN, "the depth bound lets an index move further than the margin"
        assert abs(idx[HOT] - round(float(idx[HOT]))) < 1e-9
    depth, prob = softargmin_prob(t(reg), START, INTERVAL, inverse)
    depth, prob = n(depth), n(prob)
    err = float((np.abs(depth - ed) / ed).max())
    share = float((~(np.abs(prob - ep) <= 1e-5)).mean())
    print("soft-argmin D=%d %s seed %d: E %.3g, bound %.3g, kernel %.3g; prob pixels off by more than 1e-5: %.3g, worst %.3g"
          % (D, "inverse" if inverse else "linear", seed, E, bound, err, share, float(np.abs(prob - ep).max())))
    assert depth.shape == (H, W) and np.isfinite(depth).all() and np.isfinite(prob).all()
    assert err <= bound
    assert share <= 5e-3


# ---- known answers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 481])
def test_softargmin_known_answers_on_both_kernels(D):
    """test_softargmin_kats_on_device (D = 8) on the tile kernel's unrolled loop and on the plain kernel: a one-hot column at plane k
    gives exactly start + k * interval and the buckets' sum 3 at either end (the outer neighbour clamps onto the plane itself),
    2 inside; an all-zero volume gives the mid depth and 4 / D."""
    from mvsnet_amd.model import softargmin_prob
    start, interval = 100.0, 2.0                 # every plane depth is an exact float32
    for k, expect in ((0, 3.0), (D // 2, 2.0), (D - 1, 3.0)):
        reg = np.zeros((D, 1, 70), np.float32); reg[k] = -1000.0
        depth, prob = softargmin_prob(t(reg), start, interval)
        assert np.all(n(depth) == start + interval * k), k
        assert np.all(n(prob) == expect), k
    depth, prob = softargmin_prob(t(np.zeros((D, 1, 70), np.float32)), start, interval)
    np.testing.assert_allclose(n(depth), start + interval * (D - 1) / 2.0, rtol=1e-6)
    np.testing.assert_allclose(n(prob), 4.0 / D, rtol=1e-6)


# ---- which kernel ran -------------------------------------------------------------------------------------------------------------
def summed_depth(alive, z, groups, pairwise):
    """The kernels' float32 depth of columns whose planes weigh exactly 1 (alive) or 0: group g adds its planes g, g + groups, ...
    in order, the groups' sums are combined in order (tile kernel) or as (0 + 1) + (2 + 3) (plain kernel), then sz / se."""
    f = np.float32
    part_z = np.zeros((groups, alive.shape[1]), f); part_e = np.zeros_like(part_z)
    for d in range(alive.shape[0]):
        g = d % groups
        part_e[g] = part_e[g] + alive[d]
        part_z[g] = part_z[g] + alive[d] * z[d]
    if pairwise:
        se = (part_e[0] + part_e[1]) + (part_e[2] + part_e[3]); sz = (part_z[0] + part_z[1]) + (part_z[2] + part_z[3])
    else:
        se = np.zeros(alive.shape[1], f); sz = np.zeros_like(se)
        for g in range(groups):
            se = se + part_e[g]; sz = sz + part_z[g]
    assert se.dtype == sz.dtype == f
    return sz / se


@pytest.mark.parametrize("D", [479, 480, 481, 500])
def test_softargmin_takes_the_tile_kernel_up_to_480_planes_and_the_plain_kernel_above(D):
    """Both kernels give right answers on either side of D = 480, so the parity tests cannot see where the launcher switches; the
    order of their float32 sums can.  Every plane of a column weighs exactly 1 (reg = 0: exp(0)) or 0 (reg = 1000: exp underflows)
    and the plane depths 2^20 + d / 8 are exact float32, so the only rounding is in the running sums of depths (about 5e8, ulp 32)
    and in the final division -- and the tile kernel adds planes g, g + 16, .. per group and combines 16 sums in order, the plain
    kernel g, g + 4, .. and (0 + 1) + (2 + 3) (softargmin.hip).  Restated in numpy float32, the two orders differ on most columns;
    the device must give the bits of the kernel the launcher documents for D: tile up to 480 planes (61 440 B of dynamic LDS
    beside 4 096 B of static: 64 KB), plain above."""
    from mvsnet_amd.model import softargmin_prob
    start, interval, P = float(2 ** 20), 0.125, 70
    rs = np.random.RandomState(D)
    alive = (rs.uniform(size=(D, P)) < 0.7).astype(np.float32)
    alive[0] = 1.0                                # the column's maximum of -reg is 0
    alive[:, :6] = 1.0                            # six columns with every plane alive
    z = (start + interval * np.arange(D)).astype(np.float32)
    assert np.array_equal(z.astype(np.float64), start + interval * np.arange(D))
    tile, plain = summed_depth(alive, z, 16, False), summed_depth(alive, z, 4, True)
    differ = tile != plain
    assert differ.mean() > 0.25, "the two orders must be told apart"
    exact = (alive.astype(np.float64) * z[:, None]).sum(0) / alive.sum(0)
    assert np.abs(tile - exact).max() <= 1e-6 * start and np.abs(plain - exact).max() <= 1e-6 * start
    reg = np.where(alive > 0, 0.0, 1000.0).astype(np.float32).reshape(D, 1, P)
    depth, _prob = softargmin_prob(t(reg), start, interval)
    depth = n(depth)[0]
    want, other = (tile, plain) if D <= 480 else (plain, tile)
    print("soft-argmin route D=%d: %d of %d columns tell the kernels apart; device equals tile order on %d, plain order on %d"
          % (D, int(differ.sum()), P, int((depth == tile).sum()), int((depth == plain).sum())))
    assert np.array_equal(depth, want), "D = %d ran the %s kernel's order of sums" % (
        D, ("plain" if D <= 480 else "tile") if np.array_equal(depth, other) else "neither")


# ---- backward --------------------------------------------------------------------------------------------------------------------
def autograd(reg, g, gp, D, inverse, dtype):
    """d/d reg of sum(depth * g) [+ sum(prob * gp)] with the bucket indices as constants of the FLOAT64 forward."""
    z = torch.from_numpy(O.depth_values(D, START, INTERVAL, inverse, np.float64)).to(dtype)
    x = torch.tensor(np.asarray(reg, np.float64)).to(dtype).requires_grad_(True)
    P = torch.softmax(-x, dim=0)
    depth = (P * z[:, None, None]).sum(0)
    loss = (depth * torch.tensor(g, dtype=dtype)).sum()
    if gp is not None:
        z64 = z.double()
        d64 = (torch.softmax(-x.detach().double(), dim=0) * z64[:, None, None]).sum(0).numpy()
        idx = torch.from_numpy(plane_index(d64, D, inverse))
        if inverse:
            l0 = (D - idx.ceil().long() - 1).clamp(0, D - 1); r0 = (D - idx.floor().long() - 1).clamp(0, D - 1)
        else:
            l0 = idx.floor().long().clamp(0, D - 1); r0 = idx.ceil().long().clamp(0, D - 1)
        l1 = (l0 - 1).clamp(0, D - 1); r1 = (r0 + 1).clamp(0, D - 1)
        pick = lambda i: torch.gather(P, 0, i[None])[0]
        loss = loss + ((pick(l0) + pick(r0) + pick(l1) + pick(r1)) * torch.tensor(gp, dtype=dtype)).sum()
    loss.backward()
    return x.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def backward_case(D, inverse, with_prob):
    reg = forward_case(D, inverse, hot=False)[0]
    rs = np.random.RandomState(77 + D)
    g = rs.randn(H, W).astype(np.float32)
    gp = rs.randn(H, W).astype(np.float32) if with_prob else None
    e64 = autograd(reg, g, gp, D, inverse, torch.float64)
    e32 = autograd(reg, g, gp, D, inverse, torch.float32)
    return reg, g, gp, e64, rel_l1(e32, e64)


@pytest.mark.parametrize("with_prob", [False, True], ids=["depth", "depth+prob"])
@pytest.mark.parametrize("inverse", [False, True], ids=["linear", "inverse"])
@pytest.mark.parametrize("D", BACKWARD_PLANE_COUNTS)
def test_softargmin_backward_at_other_plane_counts(D, inverse, with_prob):
    """B.softargmin_bwd against float64 autograd at the bounds of test_softargmin_backward_matches_autograd (rel-L1 < 1e-5 for the
    depth gradient alone, < 1e-4 with a gradient for the probability map), relaxed only to 4 E_b where the float32 autograd's own
    distance E_b from float64 asks for it.  forward_case without the one-hot pixel: every plane index is INDEX_MARGIN from an
    integer, both sides choose the same buckets.  One plane: the gradient is exactly zero.

    Measured on an MI355X (E_b, then the kernel; depth gradient alone, linear / inverse; with g_prob the figures are the same to
    two digits):  D = 2: 2.4e-5 / 2.9e-5, kernel 2.5e-5 / 2.9e-5 (two planes: the gradient is a difference of two nearly equal
    products, and the bound becomes 4 E_b = 9.8e-5 / 1.2e-4);  17: 3.9e-6 / 3.3e-6, kernel 3.8e-6 / 4.3e-6 (bound 1.6e-5 / 1.3e-5);
    65: 1.6e-6 / 1.8e-6, kernel 1.7e-6 / 2.0e-6;  481: 1.4e-6 / 1.1e-6, kernel 1.6e-6 / 1.2e-6 (bound 1e-5 at both)."""
    from mvsnet_amd import backward as B
    reg, g, gp, e64, Eb = backward_case(D, inverse, with_prob)
    bound = max(1e-4 if with_prob else 1e-5, 4.0 * Eb)
    got = n(B.softargmin_bwd(t(reg), t(g), START, INTERVAL, inverse_depth=inverse, g_prob=None if gp is None else t(gp)))
    got = got.astype(np.float64)
    err = rel_l1(got, e64)
    print("soft-argmin backward D=%d %s %s: E_b %.3g, bound %.3g, kernel %.3g" % (
        D, "inverse" if inverse else "linear", "depth+prob" if with_prob else "depth", Eb, bound, err))
    assert got.shape == (D, H, W) and np.isfinite(got).all()
    if D == 1:
        assert not e64.any() and not got.any()
    else:
        assert err < bound


# ---- arena -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])
@pytest.mark.parametrize("D", [480, 481])
def test_softargmin_in_the_arena_on_either_side_of_the_switch(D, pattern):
    """The largest tile and the first plain launch with reg, depth and prob inside the poisoned, guarded arena: a read past plane
    D - 1 or past pixel 119 picks up poison, a store past either output lands in a guard."""
    lib = L.load()
    reg, ed, ep, _d32, _p32, _seed = forward_case(D, False)
    _E, bound = depth_bound(D, False)
    a = Arena(1 << 20, pattern, DEV)
    x = a.take(reg.shape, torch.float32, data=reg, readonly=True, name="reg")
    depth = a.take((H, W), torch.float32, name="depth")
    prob = a.take((H, W), torch.float32, name="prob")
    L.check(lib.mvs_softargmin_prob_f32(L.ptr(x), D, H, W, START, INTERVAL, 0, L.ptr(depth), L.ptr(prob), L.stream_ptr()),
            "mvs_softargmin_prob_f32")
    depth, prob = n(depth), n(prob)
    a.check()
    assert not (np.abs(depth - ed) / ed > bound).any() and np.isfinite(depth).all()
    assert (~(np.abs(prob - ep) <= 1e-5)).mean() <= 5e-3
