"""The cost-volume backward kernels (backward.hip: the two-pass gather behind method="gather", which training uses, and the
float-atomic scatter) against float64 autograd of oracle.torch_grad.cost_volume under the camera families of
tests/camera_families.py: roll, zoom in both directions, wide baselines, tilt, seeded random cameras, and minification beyond 8,
where the gather's candidate window used to be cut at 8 pixels and the entry returned success with part of the gradient missing
(zoom0.125 and zoom0.1 fail on that form: tests/test_cost_backward_window_host.py counts what it dropped).

Per case -- 3 views, 24 x 32 pixels, 8 planes, C = 32 and 16; wide25 also at 50 planes, which ends the 48-plane chunks of pass 1
and the 24-plane chunks of pass 2 in a chunk of 2 -- and per method:
  * the project's relative L1 < 1e-4, over the whole gradient and per view;
  * per view, tensor_distance (max |got - ref64| / max |ref64|, tests/_helpers.py) within 3 x the largest per-view distance
    that float32 torch-CPU autograd of the SAME expression shows on the SAME case.  An elementwise bound is legitimate here: a
    float32 sample point that lands on the other side of a pixel boundary changes the cell, but the bilinear weight of the
    corner that moves is zero at the boundary, so the gradient is continuous in the sample point;
  * gather: a second launch gives the same bits;
  * gather and scatter agree with each other within that same bound.

Measured on an MI355X (per family over C = 32 and 16: the smaller float32 CPU floor, then the largest per-view distance of each
method, the largest distance between the methods and the largest relative L1; the bound is 3 x the case's own floor):

    family        floor      gather     scatter    between    rel L1
    roll30        5.81e-06   4.03e-06   4.48e-06   2.28e-06   2.99e-06
    roll90        3.84e-06   4.57e-06   4.67e-06   1.68e-06   2.69e-06
    roll180       3.82e-06   2.59e-06   2.79e-06   1.56e-06   2.51e-06
    zoom0.5       4.55e-06   3.10e-06   3.04e-06   1.04e-06   2.54e-06
    zoom0.25      3.18e-06   2.43e-06   2.52e-06   7.14e-07   2.25e-06
    zoom2         5.48e-06   7.53e-06   7.06e-06   4.86e-06   3.30e-06
    zoom4         9.01e-06   7.51e-06   7.63e-06   5.70e-06   6.26e-06
    wide25        4.33e-06   4.79e-06   5.28e-06   1.59e-06   3.04e-06
    wide45        4.38e-06   3.96e-06   3.96e-06   1.40e-06   2.82e-06
    tilt20        5.01e-06   4.55e-06   4.57e-06   2.11e-06   3.08e-06
    random0       3.20e-06   2.95e-06   3.03e-06   1.70e-06   2.53e-06
    random1       3.00e-06   3.07e-06   3.06e-06   1.35e-06   2.26e-06
    random2       3.52e-06   3.00e-06   3.08e-06   2.72e-06   2.97e-06
    random3       3.77e-06   2.96e-06   5.74e-06   4.23e-06   3.38e-06
    zoom0.125     2.20e-06   2.29e-06   1.83e-06   2.03e-06   2.16e-06
    zoom0.1       2.61e-06   1.95e-06   2.01e-06   1.03e-06   2.30e-06
    wide25, D 50  3.77e-06   3.54e-06   3.46e-06   1.68e-06   2.82e-06

The largest share of its bound any case used was 0.43.  With the window cut at 8 pixels the gather's source-view distances were
1.4e-02 .. 1.7e-02 at zoom0.125 and 8.5e-02 .. 1.1e-01 at zoom0.1 (relative L1 7.9e-03 and 1.5e-01) while the scatter kernel stayed
at 1.8e-06: those four cases failed all three criteria.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import torch_grad as TG
from mvsnet_amd import synthetic as S
from tests import camera_families as CF
from tests._helpers import tensor_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, H, W = 3, 24, 32
MARGIN = 3.0
REL_L1 = 1e-4


CASES = [(name, C, 8) for name in CF.FAMILIES for C in (32, 16)] + [("wide25", 32, 50), ("wide25", 16, 50)]


@pytest.fixture(scope="module", autouse=True)
def _lib(lib_built):
    from mvsnet_amd import _lib as L
    L.load()
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield


def rel_l1(a, b):
    return float(np.abs(a - b).sum() / max(np.abs(b).sum(), 1e-30))


def autograd(feats, t8, g, dtype):
    f = torch.tensor(feats, dtype=dtype).requires_grad_(True)
    cost = TG.cost_volume(f, torch.tensor(t8, dtype=dtype)).permute(1, 2, 3, 0)            # (D, H, W, C)
    (cost * torch.tensor(g, dtype=dtype)).sum().backward()
    return f.grad.numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def problem(name, C, D):
    """-> feats, t8, g1, g2 (float32), the float64 gradient (N, H, W, C) and the float32 CPU floor: the largest per-view
    tensor_distance of float32 autograd from it.  Read-only, computed once per case."""
    t8 = CF.family_transforms(name, N, H, W, D)
    feats = S.make_features(N, H, W, C, seed=5)
    rs = np.random.RandomState(3)
    g1 = rs.randn(D, H, W, C).astype(np.float32)
    g2 = rs.randn(D, H, W, C).astype(np.float32)
    g = g1.astype(np.float64) + g2
    ref = autograd(feats, t8, g, torch.float64)
    f32 = autograd(feats, t8, g, torch.float32)
    floor = max(tensor_distance(f32[v], ref[v]) for v in range(N))
    for a in (feats, t8, g1, g2, ref):
        a.setflags(write=False)
    return feats, t8, g1, g2, ref, floor


@pytest.mark.parametrize("name,C,D", CASES, ids=["%s-C%d-D%d" % c for c in CASES])
def test_cost_volume_backward_matches_float64_under_the_camera_family(name, C, D):
    from mvsnet_amd import backward as B
    feats, t8, g1, g2, ref, floor = problem(name, C, D)
    bound = MARGIN * floor
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)              # (a copy: the cached arrays are read-only)
    ft, tt, g1t, g2t = t(feats), t(t8), t(g1), t(g2)
    got = {}
    for method in ("gather", "scatter"):
        g_ref, g_src = B.cost_volume_bwd(ft[0], ft[1:], tt, g1t, g2t, method=method)
        if method == "gather":
            r2, s2 = B.cost_volume_bwd(ft[0], ft[1:], tt, g1t, g2t, method=method)
            torch.cuda.synchronize()
            assert torch.equal(r2, g_ref) and torch.equal(s2, g_src), "gather is not bit-reproducible"
        torch.cuda.synchronize()
        got[method] = np.concatenate([g_ref.cpu().numpy()[None], g_src.cpu().numpy()], 0).astype(np.float64)
    dist = {m: [tensor_distance(got[m][v], ref[v]) for v in range(N)] for m in got}
    l1 = {m: [rel_l1(got[m], ref)] + [rel_l1(got[m][v], ref[v]) for v in range(N)] for m in got}
    scale = [np.abs(ref[v]).max() for v in range(N)]
    between = [float(np.abs(got["gather"][v] - got["scatter"][v]).max() / scale[v]) for v in range(N)]
    print("\n%s C=%d D=%d: float32 CPU floor %.3e bound %.3e | gather dist %s l1 %.2e | scatter dist %s l1 %.2e | between %s"
          % (name, C, D, floor, bound, " ".join("%.2e" % d for d in dist["gather"]), max(l1["gather"]),
             " ".join("%.2e" % d for d in dist["scatter"]), max(l1["scatter"]), " ".join("%.2e" % d for d in between)))
    for m in ("gather", "scatter"):
        assert max(l1[m]) < REL_L1, (m, l1[m])
        assert max(dist[m]) <= bound, (m, dist[m], bound)
    assert max(between) <= bound, (between, bound)
