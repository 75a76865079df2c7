"""Every weight-gradient kernel behind mvs_conv3d_wgrad_f32 at the seams of its tiling and depth chunking: the cases of
tests/wgrad_seam_cases.py (its docstring has the table, the shapes and why; tests/test_wgrad_seam_cases_host.py shows that a seam
defect is at least 100 bounds in some tap at them) against float64 autograd.

Per case:
  * the workspace query answers tiles x chunks x 27 x CB x CS x 4 bytes with the chunk count derived on the host from the plan
    formulas -- a change to a plan fails here instead of silently moving the seam the shapes were chosen for;
  * the project's whole-tensor relative L1 < 2e-5;
  * the relative L1 of each of the 27 (CB, CS) tap slabs -- a defect confined to one tap or to one chunk boundary does not
    average out -- within 3 x the float32 CPU floor: the largest per-tap distance from float64 that float32 torch-CPU autograd of
    the same expression shows over the whole table (3 x: the margin of tests/test_gpu_towers_backward.py for a different float32
    summation order).  Measured: floor 2.29e-06 on the MI355X's host, bound 6.86e-06 (1.31e-06 / 3.94e-06 on another host: the
    float32 CPU convolution's summation order is the host's; wgrad_c1_kernel at 87 x 9 x 33, eight numbers per tap, sets it,
    the MFMA rows stay at 5.2e-07).  The device's largest per-tap distance: 4.25e-07 (run<8, 1, 1, 8>), 2.3e-07 .. 3.7e-07 per
    row otherwise; its largest whole-tensor distance 2.96e-07;
  * a second launch gives the same bits.

Stride 2 with an odd D, H or W is refused: the workspace query answers 0, the entry MVS_E_SHAPE with a pre-filled dw untouched,
and backward.conv3d_wgrad raises.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import wgrad_seam_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 3.0


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    from mvsnet_amd import _lib as L
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


@pytest.fixture(scope="module")
def tap_bound():
    """3 x the largest per-tap distance of float32 CPU autograd from the float64 reference over the table."""
    floor = 0.0
    for c in T.CASES:
        big, small = T.case_arrays(c)
        floor = max(floor, float(T.per_tap(T.wgrad_autograd(c.kind, big, small, c.stride, torch.float32), T.reference(c)).max()))
    print("\nweight-gradient seams: float32 CPU per-tap floor %.3e, bound %.3e" % (floor, MARGIN * floor))
    return MARGIN * floor


def t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV)


@pytest.mark.parametrize("c", T.CASES, ids=list(map(T.case_id, T.CASES)))
def test_weight_gradient_matches_float64_at_the_seam(c, tap_bound):
    from mvsnet_amd import _lib as L
    from mvsnet_amd import backward as B
    row = T.ROW_OF[c.name]
    big, small = T.case_arrays(c)
    D, H, W = big.shape[:3]
    need = L.load().mvs_conv3d_wgrad_workspace_bytes(D, H, W, c.cb, c.cs, c.stride)
    assert need == T.workspace_bytes(row, c.cs, c.shape), (need, T.plan(row, c.shape))
    bt, st = t(big), t(small)
    dw = B.conv3d_wgrad(bt, st, c.stride)
    again = B.conv3d_wgrad(bt, st, c.stride)
    torch.cuda.synchronize()
    got = dw.cpu().numpy().astype(np.float64)
    ref = T.reference(c)
    assert got.shape == ref.shape == (3, 3, 3, c.cb, c.cs)
    whole, taps = T.rel_l1(got, ref), T.per_tap(got, ref)
    print("\n%s: whole %.3e, worst tap %d at %.3e (bound %.3e), chunks %s"
          % (T.case_id(c), whole, int(taps.argmax()), taps.max(), tap_bound, T.chunk_planes(row, c.shape)))
    assert whole < T.WHOLE_BOUND
    assert taps.max() <= tap_bound, (int(taps.argmax()), taps.max(), tap_bound)
    assert torch.equal(dw, again), "a second launch gave other bits"


@pytest.mark.parametrize("odd", [(5, 8, 16), (6, 9, 16), (6, 8, 17), (5, 9, 17)])
@pytest.mark.parametrize("cb,cs", [(32, 16), (8, 16), (64, 24)])
def test_stride_two_refuses_odd_sizes_and_writes_nothing(cb, cs, odd):
    from mvsnet_amd import _lib as L
    from mvsnet_amd import backward as B
    lib = L.load()
    D, H, W = odd
    even = tuple(n + n % 2 for n in odd)
    assert lib.mvs_conv3d_wgrad_workspace_bytes(*even, cb, cs, 2) > 0           # the same channels are taken at even sizes
    assert lib.mvs_conv3d_wgrad_workspace_bytes(D, H, W, cb, cs, 2) == 0
    rs = np.random.RandomState(0)
    big = t(rs.standard_normal((D, H, W, cb)))
    small = t(rs.standard_normal(tuple((n + 1) // 2 for n in odd) + (cs,)))
    ws = torch.zeros(lib.mvs_conv3d_wgrad_workspace_bytes(*even, cb, cs, 2), device=DEV, dtype=torch.uint8)
    dw = torch.full((3, 3, 3, cb, cs), 7.25, device=DEV, dtype=torch.float32)
    rc = lib.mvs_conv3d_wgrad_f32(L.ptr(big), L.ptr(small), D, H, W, cb, cs, 2, C.c_void_p(ws.data_ptr()), ws.numel(), L.ptr(dw),
                                  L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == T.MVS_E_SHAPE
    assert bool((dw == 7.25).all()) and bool((ws == 0).all())
    with pytest.raises(L.MvsnetHipError):
        B.conv3d_wgrad(big, small, 2)
