"""Times the rendering of a point cloud into per-view depth maps (mvs_render_points_f32 through mvsnet_amd.render) on
bench_pointcloud_eval's seeded dtu_like clouds and prints one JSON line.  Per cloud (ground truth 2.5 M points, prediction
4 M), image size (640 x 512, 160 x 128) and splat radius (0, 1), into 49 cameras on an arc:

  fused_ms              the fused call with the plan's processing order (device events, median of --reps after --warmup)
  fused_input_order_ms  the same call with order=None
  torch_ms              the same maps from torch alone, in the same process: the projection of every point into every view
                        as (V, n) float32 tensors in the statement's operation order, int64 keys, one
                        scatter_reduce_(..., "amin") per covered offset, then the split into depth and index
  same_bytes            checked once per configuration: the torch form gives the fused call's bytes
  order_ms              what the plan paid once for its order (voxel keys + stable sort; host clock around a synchronise)

The cameras stand 600 mm from (0, 0, 40) on a 60 degree arc over the scene and look at that point; the focal length puts
the 300 mm square on about two thirds of the image width.

    python tools/bench_render.py [--reps 10] [--warmup 2] [--views 49] [--n_gt N --n_pred N] [--skip_torch]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from bench_pointcloud_eval import CONFIGS, clouds, device_ms  # noqa: E402

SIZES = ((512, 640), (128, 160))
SPLATS = (0, 1)


def arc_cameras(V, H, W, distance=600.0, span_deg=60.0, target=(0.0, 0.0, 40.0)):
    """(V,2,4,4): cameras on an arc in the x-z plane above the scene, looking at `target`; f = W * distance / 450."""
    target = np.asarray(target)
    f = W * distance / 450.0
    cams = np.zeros((V, 2, 4, 4))
    for i in range(V):
        th = np.radians((i - (V - 1) / 2.0) * span_deg / max(V - 1, 1))
        C = target + distance * np.array([np.sin(th), 0.0, np.cos(th)])
        z = (target - C) / np.linalg.norm(target - C)
        x = np.cross(np.array([0.0, 1.0, 0.0]), z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        cams[i, 0, :3, :3], cams[i, 0, :3, 3], cams[i, 0, 3, 3] = R, -R @ C, 1.0
        cams[i, 1, :3, :3] = [[f, 0, W / 2.0 + 0.1371], [0, f, H / 2.0 - 0.0613], [0, 0, 1.0]]
    return cams


def torch_render(pts, P, H, W, splat):
    """The module docstring's semantics in torch ops alone -> (depth (V,H,W) float32, index (V,H,W) int32)."""
    import torch
    V, n = P.shape[0], pts.shape[0]
    X, Y, Z = pts[:, 0][None], pts[:, 1][None], pts[:, 2][None]
    row = lambda r: ((P[:, r, 0:1] * X + P[:, r, 1:2] * Y) + P[:, r, 2:3] * Z) + P[:, r, 3:4]
    u, v, w = row(0), row(1), row(2)
    fx, fy = torch.floor(u / w + 0.5), torch.floor(v / w + 0.5)
    cand = torch.isfinite(w) & (w > 0) & torch.isfinite(fx) & torch.isfinite(fy)
    key = (w.view(torch.int32).long() << 32) | torch.arange(n, device=pts.device)[None]
    base = (torch.arange(V, device=pts.device) * (H * W))[:, None]
    empty = torch.iinfo(torch.int64).max
    buf = torch.full((V * H * W,), empty, dtype=torch.int64, device=pts.device)
    for dy in range(-splat, splat + 1):
        for dx in range(-splat, splat + 1):
            px, py = fx + float(dx), fy + float(dy)
            ok = cand & (px >= 0) & (px <= float(W - 1)) & (py >= 0) & (py <= float(H - 1))
            pix = (base + torch.where(ok, py, 0.0).long() * W + torch.where(ok, px, 0.0).long())[ok]
            buf.scatter_reduce_(0, pix, key[ok], "amin")
    hit = buf != empty
    depth = torch.where(hit, (buf >> 32).int(), 0).view(torch.float32).reshape(V, H, W)
    index = torch.where(hit, (buf & 0xFFFFFFFF).int(), -1).reshape(V, H, W)
    return depth, index


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--n_gt", type=int, default=CONFIGS["dtu_like"]["n_gt"])
    ap.add_argument("--n_pred", type=int, default=CONFIGS["dtu_like"]["n_pred"])
    ap.add_argument("--skip_torch", action="store_true", help="time the fused call alone (profiling runs)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_render needs a GPU")
    torch.cuda.set_device(0)
    from mvsnet_amd import render as Rn
    dev = torch.device("cuda", 0)
    pred, gt = clouds(a.n_gt, a.n_pred)
    out = {"metric": "render_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "views": a.views, "results": []}
    for name, cloud in (("gt", gt), ("pred", pred)):
        pts = torch.as_tensor(cloud).to(dev)
        for H, W in SIZES:
            cams = arc_cameras(a.views, H, W)
            P = torch.as_tensor(Rn.projection_tables(cams).reshape(a.views, 3, 4)).to(dev)
            for splat in SPLATS:
                torch.cuda.synchronize()
                t = time.perf_counter()
                plan = Rn.RenderPlan(pts, cams, H, W, splat=splat)
                torch.cuda.synchronize()
                plan_ms = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                plan._processing_order()
                torch.cuda.synchronize()
                order_ms = (time.perf_counter() - t) * 1e3
                med, lo, hi = device_ms(plan.enqueue, a.reps, a.warmup)
                med_in, lo_in, hi_in = device_ms(lambda: plan.enqueue(order=None), a.reps, a.warmup)
                depth, index = plan.run()
                row = {"cloud": name, "points": int(pts.shape[0]), "height": H, "width": W, "splat": splat,
                       "projections": int(pts.shape[0]) * a.views, "covered_pixels": int((index >= 0).sum()),
                       "pixels": a.views * H * W, "fused_ms": round(med, 3), "fused_ms_min": round(lo, 3),
                       "fused_ms_max": round(hi, 3), "fused_input_order_ms": round(med_in, 3),
                       "fused_input_order_ms_min": round(lo_in, 3), "fused_input_order_ms_max": round(hi_in, 3),
                       "order_worth": round(med_in / med, 2), "order_ms": round(order_ms, 1), "plan_ms": round(plan_ms, 1)}
                if not a.skip_torch:
                    td, ti = torch_render(pts, P, H, W, splat)
                    row["same_bytes"] = bool(torch.equal(td.view(torch.int32), depth.view(torch.int32)) and torch.equal(ti, index))
                    del td, ti
                    bmed, blo, bhi = device_ms(lambda: torch_render(pts, P, H, W, splat), a.reps, a.warmup)
                    row.update({"torch_ms": round(bmed, 3), "torch_ms_min": round(blo, 3), "torch_ms_max": round(bhi, 3),
                                "speedup": round(bmed / med, 2)})
                out["results"].append(row)
                del plan, depth, index
                torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
