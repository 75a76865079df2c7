"""Times the point-cloud evaluation (csrc/pointcloud.hip through mvsnet_amd.evaluate) on seeded synthetic clouds and prints
one JSON line: milliseconds of EvaluationPlan.enqueue() (both grid builds, both queries, both statistics; device events,
median of --reps after --warmup), and for dtu_like per direction the query alone (mvs_nn_query_f32 over the built grid),
the grid builds (the direction's time minus its query), the statistics, and the candidate points compared per query.
scipy's cKDTree (build + both queries, workers=16) is timed for scale when scipy imports: HOST time, not device time.

  dtu_like  mm units, scene about 500 mm: a 300 mm square plane and a sphere of radius 75 mm; GT 2.5 M points on the
            surfaces (about 0.25 mm apart), prediction 4 M surface points + N(0, 0.3 mm) noise + 3 % uniform outliers in
            the 500 mm box; max_dist 20, tau 0.5 / 1 / 2
  large     the same scene at 10 M x 10 M points

    python tools/bench_pointcloud_eval.py [--reps 10] [--warmup 2] [--configs dtu_like,large] [--no-ckdtree]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = {"dtu_like": dict(n_gt=2_500_000, n_pred=4_000_000), "large": dict(n_gt=10_000_000, n_pred=10_000_000)}
MAX_DIST, THRESHOLDS = 20.0, (0.5, 1.0, 2.0)


def surface(n, rs):
    """n points on a 300 mm square (z = 0) and a sphere of radius 75 mm above it, about equal density."""
    a_plane, a_sphere = 300.0 ** 2, 4 * np.pi * 75.0 ** 2
    npl = int(n * a_plane / (a_plane + a_sphere))
    plane = np.stack([rs.uniform(-150, 150, npl), rs.uniform(-150, 150, npl), np.zeros(npl)], 1)
    v = rs.standard_normal((n - npl, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([plane, v * 75.0 + [0.0, 0.0, 90.0]])


def clouds(n_gt, n_pred, seed=0):
    rs = np.random.RandomState(seed)
    gt = surface(n_gt, rs).astype(np.float32)
    n_out = int(0.03 * n_pred)
    pred = surface(n_pred - n_out, rs) + rs.normal(0, 0.3, (n_pred - n_out, 3))
    pred = np.concatenate([pred, rs.uniform(-250, 250, (n_out, 3)) + [0.0, 0.0, 90.0]]).astype(np.float32)
    return pred[rs.permutation(len(pred))], gt


def device_ms(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def per_direction(plan, pl, ws, reps, warmup):
    """(direction ms, query-only ms, statistics ms, candidates per query: mean / p99 / max)."""
    import torch
    from mvsnet_amd import _lib
    lib = _lib.load()
    g = pl.grid
    visited = torch.empty(pl.query.shape[0], dtype=torch.int32, device=pl.dist.device)

    def query(v=None):
        _lib.check(lib.mvs_nn_query_f32(pl.query.shape[0], pl.target.shape[0], *g["origin"], g["cell"], *g["dims"], plan.max_dist,
                                        _lib.ptr(pl.dist), _lib.ptr(pl.index), _lib.ptr(v), _lib.ptr(pl.workspace),
                                        pl.workspace.numel(), _lib.stream_ptr()), "mvs_nn_query_f32")

    def stats():
        _lib.check(lib.mvs_dist_stats_f32(_lib.ptr(pl.dist), pl.dist.numel(), plan.max_dist, plan._thr, len(plan.thresholds),
                                          _lib.ptr(plan.stats[0]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "mvs_dist_stats_f32")
    total = device_ms(pl._enqueue, reps, warmup)[0]
    q = device_ms(query, reps, warmup)[0]
    st = device_ms(stats, reps, warmup)[0]
    query(visited)
    v = visited.cpu().numpy()
    return total, q, st, (float(v.mean()), float(np.percentile(v, 99)), int(v.max()))


def ckdtree_ms(pred, gt):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    t = time.perf_counter()
    tp, tg = cKDTree(pred), cKDTree(gt)
    tg.query(pred, k=1, distance_upper_bound=MAX_DIST, workers=16)
    tp.query(gt, k=1, distance_upper_bound=MAX_DIST, workers=16)
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="dtu_like,large")
    ap.add_argument("--no-ckdtree", action="store_true", help="skip the host cKDTree timing (profiling runs)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud_eval needs a GPU")
    torch.cuda.set_device(0)
    from mvsnet_amd import evaluate as E
    out = {"metric": "pointcloud_eval_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "max_dist": MAX_DIST,
           "thresholds": list(THRESHOLDS), "results": []}
    for name in a.configs.split(","):
        pred, gt = clouds(**CONFIGS[name])
        plan = E.EvaluationPlan(pred, gt, max_dist=MAX_DIST, thresholds=THRESHOLDS)
        med, lo, hi = device_ms(plan.enqueue, a.reps, a.warmup)
        m = plan.result()
        r = {"config": name, "pred_points": len(pred), "gt_points": len(gt), "ms": round(med, 3), "ms_min": round(lo, 3),
             "ms_max": round(hi, 3), "accuracy": m["accuracy"], "completeness": m["completeness"], "fscore": m["fscore"],
             "grid_pred_to_gt": m["grid_pred_to_gt"], "grid_gt_to_pred": m["grid_gt_to_pred"]}
        if name == "dtu_like":
            for key, pl, ws in (("pred_to_gt", plan.acc, plan.stats_ws[0]), ("gt_to_pred", plan.comp, plan.stats_ws[1])):
                total, q, st, (vm, v99, vmax) = per_direction(plan, pl, ws, a.reps, a.warmup)
                r[key] = {"build_ms": round(total - q, 3), "query_ms": round(q, 3), "stats_ms": round(st, 3),
                          "candidates_per_query": round(vm, 1), "candidates_p99": v99, "candidates_max": vmax}
        if not a.no_ckdtree:
            ms = ckdtree_ms(pred, gt)
            if ms is not None:
                r["ckdtree_host_ms_workers16"] = round(ms, 1)
                r["speedup_vs_ckdtree"] = round(ms / med, 1)
        out["results"].append(r)
        del plan
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
