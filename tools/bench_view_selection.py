"""Times the view selection (csrc/view_selection.hip through mvsnet_amd.select_views) on bench_pointcloud_eval's seeded
dtu_like clouds (ground truth 2.5 M points, prediction 4 M) into 49 and 144 cameras of 640 x 512 on bench_render's arc,
with frustum and z-buffer visibility, and writes one JSON line to profiles/view_selection_bench.json (and prints it).  Per
configuration (device events, median of --reps after --warmup):

  visibility_ms         the mask: mvs_view_visibility_f32, in z-buffer mode behind the render of the depth maps
  scores_ms             mvs_view_scores_f32 with the plan's processing order
  scores_input_order_ms the same call with order=None
  depth_ranges_ms       the two histogram passes and torch's scans between them
  torch_scores_ms       the pair matrices from torch alone, in the same process and from the same mask: per view c_v - p and
                        its squared norm once, then a loop over the pairs of element-wise tensor operations in the
                        statement's order and a gather from the weight table (median of --torch_reps)
  same_integers         checked once per configuration: the torch form gives the fused call's score_sum and shared

    python tools/bench_view_selection.py [--reps 10] [--warmup 2] [--torch_reps 2] [--views 49,144] [--skip_torch]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from bench_pointcloud_eval import CONFIGS, clouds, device_ms  # noqa: E402
from bench_render import arc_cameras  # noqa: E402

H, W = 512, 640


def torch_scores(pts, mask, centres, table, V):
    """The module docstring's pair score in torch ops alone -> (score_sum, shared) (V,V) int64, upper triangles."""
    import torch
    vis = [((mask[:, p // 64] >> (p % 64)) & 1).bool() for p in range(V)]
    D = [centres[v][None] - pts for v in range(V)]
    nn = [(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] for d in D]
    score = torch.zeros((V, V), dtype=torch.int64, device=pts.device)
    shared = torch.zeros_like(score)
    for a in range(V):
        for b in range(a + 1, V):
            both = vis[a] & vis[b]
            dot = (D[a][:, 0] * D[b][:, 0] + D[a][:, 1] * D[b][:, 1]) + D[a][:, 2] * D[b][:, 2]
            x = (1.0 - (dot * dot) / (nn[a] * nn[b]))
            f = torch.floor(torch.sqrt(torch.where(x < 0, 0.0, x)) * 8192.0)
            ok = both & (dot > 0) & torch.isfinite(f)
            k = torch.where(ok, f, 0.0).long().clamp(max=8191)
            score[a, b] = torch.where(ok, table[k], 0).sum()
            shared[a, b] = both.sum()
    return score, shared


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch_reps", type=int, default=2)
    ap.add_argument("--views", default="49,144")
    ap.add_argument("--n_gt", type=int, default=CONFIGS["dtu_like"]["n_gt"])
    ap.add_argument("--n_pred", type=int, default=CONFIGS["dtu_like"]["n_pred"])
    ap.add_argument("--skip_torch", action="store_true", help="time the fused calls alone (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_selection_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_view_selection needs a GPU")
    torch.cuda.set_device(0)
    from mvsnet_amd import select_views as S
    dev = torch.device("cuda", 0)
    pred, gt = clouds(a.n_gt, a.n_pred)
    out = {"metric": "view_selection_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "height": H, "width": W,
           "results": []}
    for name, cloud in (("gt", gt), ("pred", pred)):
        pts = torch.as_tensor(cloud).to(dev)
        for V in (int(v) for v in a.views.split(",")):
            cams = arc_cameras(V, H, W)
            for mode in ("frustum", "zbuffer"):
                plan = S.ViewSelectionPlan(pts, cams=cams, size=(H, W), visibility=mode)
                r = plan.run()
                per_point = sum(((r["mask"][:, w] >> b) & 1) for w in range(plan.MW) for b in range(64) if 64 * w + b < V)
                pairs = int((per_point * (per_point - 1) // 2).sum())
                row = {"cloud": name, "points": int(pts.shape[0]), "views": V, "visibility": mode,
                       "views_per_point": round(float(per_point.double().mean()), 2), "pair_evaluations": pairs}
                for key, fn in (("visibility_ms", plan.enqueue_visibility), ("scores_ms", plan.enqueue_scores),
                                ("scores_input_order_ms", lambda: plan.enqueue_scores(order=None)),
                                ("depth_ranges_ms", plan.enqueue_depth_ranges)):
                    med, lo, hi = device_ms(fn, a.reps, a.warmup)
                    row.update({key: round(med, 3), key + "_min": round(lo, 3), key + "_max": round(hi, 3)})
                row["pair_evaluations_per_ns"] = round(pairs / (row["scores_ms"] * 1e6), 2)
                if not a.skip_torch:
                    table = plan.table.long() & 0xFFFF
                    centres = plan.centres.view(V, 3)
                    plan.enqueue_scores()
                    ts, tn = torch_scores(pts, plan.mask, centres, table, V)
                    row["same_integers"] = bool(torch.equal(ts, plan.score_sum) and torch.equal(tn, plan.shared))
                    del ts, tn
                    med, lo, hi = device_ms(lambda: torch_scores(pts, plan.mask, centres, table, V), a.torch_reps, 0)
                    row.update({"torch_scores_ms": round(med, 1), "torch_scores_ms_min": round(lo, 1),
                                "torch_scores_ms_max": round(hi, 1), "speedup": round(med / row["scores_ms"], 1)})
                out["results"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del plan, r, per_point
                torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
