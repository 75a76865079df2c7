"""The six kernels of csrc/gru_train.hip behind mvs_gru_train_cell_fwd_f32 / _bwd_f32, element by element against the float64
reference with the kernels' own interface (tests/gru_train_reference.py), inside the poisoned, guarded arena, through the C ABI.

The tile is TH x 16 with TH = 16 / NS rows and NS output-channel groups (F = 16: 4 x 16, 4 groups; F = 8: 8 x 16, 2; F <= 4:
16 x 16, 1).  Per F the seam shape (2 TH + 1, 33) -- two full tiles and a one-pixel remainder on both axes -- at D = 3 and 4 (both
parities of the dh / dz_u ping-pong buffers end a sweep), (1, 17) and (17, 1) at D = 2 and (5, 7) at D = 1: there H*W*F is no
multiple of 256 and the elementwise launches end in a partial block.  Per case and arena pattern:

  forward      g, c, rh and every plane of h[1..D] element by element; stats folded over its slots against the float64 sums; h[0]
               bit-identical afterwards; a second call gives the same bits and the same sums up to the order of the float64 atomics;
  backward     with dh_in = dh_out = null and a zeroed scratch: gpx element by element, part folded over its slots;
               with a random dh_in, dh_out given and scratch left POISONED: gpx, part and dh_out;
  chunked      (the D = 4 seam shapes) forward as planes [0,1), [1,3), [3,4) through one (D+1)-plane h buffer, backward the same
               chunks descending with one call's dh_out as the next call's dh_in and ONE poisoned scratch for all calls, as
               gru_train.RecurrentCells runs the cells: every buffer against the float64 reference of the whole chain and against
               the unchunked device result, both at the same bounds.  (Not bit-identical by construction: unchunked, a plane's
               blend and its backward run inside the staging / epilogue of the neighbouring plane's gate kernel, at a chunk's
               end in gt_blend_kernel / gt_bwd_blend_kernel -- the same expressions in another kernel, which the compiler may
               contract differently, and per-channel sums partitioned differently.)

Operands are read-only regions; the caller's part of the contract is zeroing stats, part and (dh_in null) scratch; everything else
starts as poison; the forward's g, c, h and stats are frozen before the backward takes them as const; arena.check() ends each case.
The flipped / transposed kernels come from gru_train.flip_t, the slot counts from mvs_gru_train_slots.

Bounds: atol + rtol |expected| per element, gru_train_reference.BOUNDS = MARGIN x the float32 floor below.  The floor is the
reference's float32 mode against its float64 mode on the CPU (tests/test_gru_train_reference_host.py measures it, fits it and
holds BOUNDS to it); `atol, rtol` per output, worst over the cases of the class -- the element-by-element outputs share one floor
per F, the sums (stats, part) have one per shape class because theirs grows with the number of terms:

    F  class   g                  c                  rh                 h                  stats              gpx                part               dh_out
    16 seam    1.2e-06, 4.5e-07   7e-07, 3.8e-07     2.5e-07, 2.3e-07   4.3e-07, 2e-08     0.00012, 1.2e-07   4e-07, 1.2e-06     2.7e-06, 7.7e-07   6.5e-07, 1.9e-07
    16 narrow  1.2e-06, 4.5e-07   7e-07, 3.8e-07     2.5e-07, 2.3e-07   4.3e-07, 2e-08     6e-06, 1.1e-07     4e-07, 1.2e-06     7.3e-07, 2.5e-07   6.5e-07, 1.9e-07
    8  seam    9e-07, 1.7e-07     4e-07, 4e-08       2.1e-07, 1.3e-07   3.3e-07, 5.8e-09   0.00022, 9e-08     2.3e-07, 1.5e-06   3.8e-06, 4.8e-07   5e-07, 3e-07
    8  narrow  9e-07, 1.7e-07     4e-07, 4e-08       2.1e-07, 1.3e-07   3.3e-07, 5.8e-09   7.3e-06, 9.3e-08   2.3e-07, 1.5e-06   7e-07, 3.8e-07     5e-07, 3e-07
    4  seam    7e-07, 1.4e-07     4.3e-07, 2.5e-08   1.6e-07, 7.7e-08   3e-07, 6.8e-08     0.0005, 2.3e-08    2.3e-07, 2.1e-06   4.2e-06, 1.5e-07   7.5e-07, 1.8e-07
    4  narrow  7e-07, 1.4e-07     4.3e-07, 2.5e-08   1.6e-07, 7.7e-08   3e-07, 6.8e-08     9.5e-07, 7.5e-08   2.3e-07, 2.1e-06   1.3e-06, 6.7e-07   7.5e-07, 1.8e-07
    2  seam    5.2e-07, 5.3e-08   3.3e-07, 7.5e-08   1.3e-07, 8.3e-08   1.9e-07, 1.9e-07   0.00025, 2.3e-08   2.2e-07, 8e-07     1.9e-06, 5.5e-07   4.8e-07, 2.5e-07
    2  narrow  5.2e-07, 5.3e-08   3.3e-07, 7.5e-08   1.3e-07, 8.3e-08   1.9e-07, 1.9e-07   1.5e-06, 6e-08     2.2e-07, 8e-07     4.5e-07, 5.8e-07   4.8e-07, 2.5e-07
    1  seam    2.8e-07, 9.3e-08   2.8e-07, 6.8e-08   1e-07, 2.8e-07     2.2e-07, 5.5e-08   1.7e-05, 1.2e-07   2.8e-07, 3.5e-06   3.2e-06, 4e-07     4.8e-07, 2e-07
    1  narrow  2.8e-07, 9.3e-08   2.8e-07, 6.8e-08   1e-07, 2.8e-07     2.2e-07, 5.5e-08   7.3e-07, 9.8e-08   2.8e-07, 3.5e-06   2.2e-07, 1.5e-06   4.8e-07, 2e-07

MARGIN = 4: what tests/test_gpu_value_conditioning.py grants over its float32 floor (max |got - e64| <= 4 E; that file's margin is
4, not 8, so 4 it is here).  It covers the device's other summation order and the 1-ulp hardware exp / reciprocal of the gates.
Every test prints the largest error of each output in bounds (pytest -s).  No element is left out of any comparison.

As measured on an MI355X, largest error over all cases in bounds: forward g 0.45, c 0.94, rh 0.49, h 0.43, stats 0.52; backward
gpx 0.77, part 0.42, dh_out 0.42; chunked against the whole sweep on the device: forward below 0.005, backward 0.19.

What it adds to test_gpu_backward's whole-tensor test, tried once with the kernel broken in a scratch copy: (a) gt_gates_kernel
staging the halo column left of the seam w = 16 as zero -- 70 of the 110 tests here fail and name plane >= 1, tile (*, 1), column 0
of the tile at 2e5 bounds; (b) gt_bwd_gates_kernel staging ONE halo pixel (tile (0, 1), row 0) as zero -- 40 fail, the first
element named sits in tile (0, 1), row 1 col 0 at 4e4 bounds.  The whole-tensor test fails under both as well wherever its shape has
a seam at w = 16 -- under (b) at rel-L1 1.8e-4 ... 5.4e-4 against its limit of 1e-4, two to five times where this file stands
four orders of magnitude out -- and says neither where nor in which buffer; the wavefront test (device against device) passes (b).
"""
import numpy as np
import pytest
import torch

from mvsnet_amd import _lib as L
from mvsnet_amd import gru_train as G

from tests import gru_train_reference as R
from tests.device_arena import PATTERNS, Arena

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
CHUNKS = ((0, 1), (1, 3), (3, 4))
both_patterns = pytest.mark.parametrize("pattern", PATTERNS, ids=["nan", "huge"])


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def n(x):
    torch.cuda.synchronize()
    return x.detach().cpu().numpy()


def slots():
    sf, sb = L.C.c_int(), L.C.c_int()
    L.load().mvs_gru_train_slots(L.C.byref(sf), L.C.byref(sb))
    assert sf.value >= 1 and sb.value >= 1
    return sf.value, sb.value


class Operands:
    """One case's operands, read-only inside an arena with room for every buffer the case's calls write."""

    def __init__(self, case, pattern):
        self.case = c = case
        self.sf, self.sb = slots()
        arrays = dict(R.case_inputs(c))
        arrays["wgh_t"] = G.flip_t(torch.tensor(arrays["wgh"])).numpy()        # the layouts gru_train.py itself hands over
        arrays["woh_t"] = G.flip_t(torch.tensor(arrays["woh"])).numpy()
        assert arrays["wgh_t"].shape == (3, 3, 2 * c.F, c.F) and arrays["woh_t"].shape == (3, 3, c.F, c.F)
        plane = c.H * c.W * c.F
        fwd = 4 * plane * (5 * c.D + 1) + 8 * c.D * self.sf * 6
        bwd = 4 * plane * (3 * c.D + 7) + 8 * c.D * 3 * self.sb * 2 * c.F
        regions = len(arrays) + 3 * 5 + 4 * 4 + 8
        nbytes = sum(v.nbytes for v in arrays.values()) + 3 * fwd + 4 * bwd
        self.a = Arena(nbytes + regions * (2 * 64 * 1024 + 512) + (1 << 20), pattern, DEV)
        self.t = {k: self.a.take(v.shape, F32, data=np.ascontiguousarray(v), readonly=True, name=k) for k, v in arrays.items()}

    def forward_buffers(self, tag):
        c, a = self.case, self.a
        D, H, W, Fn = c.D, c.H, c.W, c.F
        b = dict(g=a.take((D, H, W, 2 * Fn), F32, name="g_" + tag), c=a.take((D, H, W, Fn), F32, name="c_" + tag),
                 rh=a.take((D, H, W, Fn), F32, name="rh_" + tag), h=a.take((D + 1, H, W, Fn), F32, name="h_" + tag),
                 stats=a.take((D, self.sf, 6), F64, name="stats_" + tag))
        b["h"][0].copy_(self.t["h0"])                       # the caller's: the state entering plane 0 ...
        b["stats"].zero_()                                  # ... and zeroed moments
        return b

    def forward(self, b, lo=0, hi=None):
        c, t = self.case, self.t
        hi = c.D if hi is None else hi
        L.check(L.load().mvs_gru_train_cell_fwd_f32(
            L.ptr(t["px"][lo:hi]), L.ptr(t["wgh"]), L.ptr(t["woh"]), L.ptr(t["ln"]), hi - lo, c.H, c.W, c.F, L.ptr(b["g"][lo:hi]),
            L.ptr(b["c"][lo:hi]), L.ptr(b["rh"][lo:hi]), L.ptr(b["h"][lo:hi + 1]), L.ptr(b["stats"][lo:hi]), L.stream_ptr()),
            "mvs_gru_train_cell_fwd_f32")

    def backward_buffers(self, tag, zero_scratch):
        c, a = self.case, self.a
        D, H, W, Fn = c.D, c.H, c.W, c.F
        b = dict(gpx=a.take((D, H, W, 3 * Fn), F32, name="gpx_" + tag), part=a.take((D, 3, self.sb, 2, Fn), F64, name="part_" + tag),
                 scratch=a.take((6, H, W, Fn), F32, name="scratch_" + tag))
        b["part"].zero_()
        if zero_scratch:
            b["scratch"].zero_()
        return b

    def backward(self, f, b, dh_in, dh_out, lo=0, hi=None):
        c, t = self.case, self.t
        hi = c.D if hi is None else hi
        L.check(L.load().mvs_gru_train_cell_bwd_f32(
            L.ptr(t["gh"][lo:hi]), L.ptr(f["g"][lo:hi]), L.ptr(f["c"][lo:hi]), L.ptr(f["h"][lo:hi]), L.ptr(f["stats"][lo:hi]),
            L.ptr(t["wgh_t"]), L.ptr(t["woh_t"]), L.ptr(t["ln"]), hi - lo, c.H, c.W, c.F, L.ptr(b["gpx"][lo:hi]),
            L.ptr(b["part"][lo:hi]), L.ptr(b["scratch"]), L.ptr(dh_in), L.ptr(dh_out), L.stream_ptr()),
            "mvs_gru_train_cell_bwd_f32")


def fold(name, x):
    """A device buffer as the reference lays it out: stats and part summed over their slots, h without its plane 0."""
    x = n(x).astype(np.float64)
    return x.sum(1) if name == "stats" else (x.sum(2) if name == "part" else x)


def hold(case, what, got, exp, names):
    """Prints the largest error of every output in bounds, then asserts each output element by element."""
    msgs = []
    for k in names:
        ratio = np.abs(got[k] - exp[k]) / R.bound(case, k, exp[k])
        print("%s %s %-6s %.2f bounds" % (R.case_id(case), what, k, float(np.where(np.isfinite(ratio), ratio, np.inf).max())))
        m = R.describe_failures(case, k, got[k], exp[k])
        if m is not None:
            msgs.append(m)
    assert not msgs, "%s\n%s" % (what, "\n".join(msgs))


def same_sums(got, ref, terms):
    """float64 sums of the same float32 partials added in another order (test_gpu_halo_planes.sums_equal): sums to 1e-12 of the
    sum of the terms' magnitudes, sums of squares to 1e-12 of themselves."""
    np.testing.assert_allclose(got[:, 0::2], ref[:, 0::2], rtol=1e-12, atol=1e-12 * terms)
    np.testing.assert_allclose(got[:, 1::2], ref[:, 1::2], rtol=1e-12, atol=0)


FWD = ("g", "c", "rh", "h", "stats")


def forward_outputs(b):
    return {k: fold(k, b[k]) for k in FWD}


def run_forward(ops, tag):
    b = ops.forward_buffers(tag)
    ops.forward(b)
    return b


@both_patterns
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_forward_every_element_and_the_same_bits_twice(case, pattern):
    ops = Operands(case, pattern)
    e = R.expect(case, False)
    b1 = run_forward(ops, "1")
    got = forward_outputs(b1)
    hold(case, "forward", got, e, FWD)
    assert np.array_equal(n(b1["h"][0]).view(np.uint32), R.case_inputs(case)["h0"].view(np.uint32)), "h[0] changed"
    b2 = run_forward(ops, "2")
    for k in ("g", "c", "rh", "h"):
        assert torch.equal(b1[k].view(torch.int32), b2[k].view(torch.int32)), "%s differs between two calls" % k
    terms = float(np.abs(e["g"]).sum(axis=(1, 2, 3)).max() + np.abs(e["c"]).sum(axis=(1, 2, 3)).max())
    same_sums(fold("stats", b2["stats"]), got["stats"], terms)
    ops.a.check()


@both_patterns
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_backward_every_element_without_and_with_a_state_gradient_from_above(case, pattern):
    ops = Operands(case, pattern)
    f = run_forward(ops, "f")
    for k in ("g", "c", "h", "stats"):
        ops.a.freeze(f[k])                                  # const operands of the backward from here on
    b = ops.backward_buffers("null", zero_scratch=True)
    ops.backward(f, b, None, None)
    hold(case, "backward, dh_in null", {k: fold(k, b[k]) for k in ("gpx", "part")}, R.expect(case, False), ("gpx", "part"))
    b = ops.backward_buffers("carry", zero_scratch=False)   # dh_in given: nothing of scratch may be read before it is written
    dh_out = ops.a.take((case.H, case.W, case.F), F32, name="dh_out")
    ops.backward(f, b, ops.t["dh_in"], dh_out)
    b["dh_out"] = dh_out
    hold(case, "backward, dh_in given", {k: fold(k, b[k]) for k in ("gpx", "part", "dh_out")}, R.expect(case, True),
         ("gpx", "part", "dh_out"))
    ops.a.check()


@both_patterns
@pytest.mark.parametrize("case", [c for c in R.SEAM_CASES if c.D == 4], ids=R.case_id)
def test_chunked_sweep_is_the_whole_chain(case, pattern):
    assert CHUNKS[0][0] == 0 and CHUNKS[-1][1] == case.D and all(a[1] == b[0] for a, b in zip(CHUNKS, CHUNKS[1:]))
    ops = Operands(case, pattern)
    e = R.expect(case, True)
    whole = run_forward(ops, "whole")
    f = ops.forward_buffers("chunked")
    for lo, hi in CHUNKS:                                   # ascending, h carried through the (D+1)-plane buffer
        ops.forward(f, lo, hi)
    got = forward_outputs(f)
    hold(case, "chunked forward", got, e, FWD)
    hold(case, "chunked forward against the whole sweep on the device", got, forward_outputs(whole), FWD)
    for buf in (whole, f):
        for k in ("g", "c", "h", "stats"):
            ops.a.freeze(buf[k])
    names = ("gpx", "part", "dh_out")
    bw = ops.backward_buffers("whole", zero_scratch=False)
    bw["dh_out"] = ops.a.take((case.H, case.W, case.F), F32, name="dh_out_whole")
    ops.backward(whole, bw, ops.t["dh_in"], bw["dh_out"])
    bc = ops.backward_buffers("chunked", zero_scratch=False)
    carry = ops.a.take((len(CHUNKS) + 1, case.H, case.W, case.F), F32, name="carry")
    carry[len(CHUNKS)].copy_(ops.t["dh_in"])                # what arrives at the last plane from beyond the sweep
    for j in reversed(range(len(CHUNKS))):                  # descending, dh_out of one call is dh_in of the next
        ops.backward(f, bc, carry[j + 1], carry[j], *CHUNKS[j])
    bc["dh_out"] = carry[0]
    got = {k: fold(k, bc[k]) for k in names}
    hold(case, "chunked backward", got, e, names)
    hold(case, "chunked backward against the whole sweep on the device", got, {k: fold(k, bw[k]) for k in names}, names)
    ops.a.check()
