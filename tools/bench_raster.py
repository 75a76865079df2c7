"""Times the rasterisation of a triangle mesh into per-view depth maps (mvs_raster_mesh_f32 through mvsnet_amd.render_mesh)
and writes profiles/raster_bench.json (the same JSON is printed as one line).  The mesh is a seeded closed surface, a sphere
of radius 120 mm with bumps of a few millimetres, of about 2 M and about 5 M faces; the cameras are bench_render's 49 on an
arc, 600 mm away, at 160 x 128 and 1152 x 864.  Per mesh and image size:

  mesh_ms         the fused call with the plan's processing order and the default large path (device events; the median
                  over --blocks blocks of the median of --reps calls, after --warmup calls; min and max of the block medians)
  splat0_ms       render.py's splat-0 call on as many points (the face centroids) from the same cameras in the same
                  process: the yardstick for the per-primitive loop
  ground_ms       the same mesh plus a ground plane of two triangles that fills the image behind it, default large path
  ground_few_ms, ground_few_lane_ms   the ground-plane mesh into the first --lane_views views with the default large path and
                  with large_pixels = 2^30: no pair is queued, a lane walks the whole plane (--lane_reps calls, no warm-up)
  same_bytes      the two give the same depth and index bytes
  sweep           ground_ms over large_pixels x queue_capacity (the module's defaults are chosen from it)

    python tools/bench_raster.py [--reps 5] [--blocks 3] [--warmup 2] [--views 49] [--faces 2000000 5000000] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from bench_pointcloud_eval import device_ms  # noqa: E402
from bench_render import arc_cameras  # noqa: E402

SIZES = ((128, 160), (864, 1152))
SWEEP_LARGE = (16, 64, 256, 1024, 4096)
SWEEP_QUEUE = (1 << 10, 1 << 16, 1 << 20)


def bumpy_sphere(n_faces, radius=120.0, centre=(0.0, 0.0, 140.0), seed=0):
    """A closed, outward-wound sphere of about n_faces triangles (stacks = slices), the radius modulated by a few smooth
    bumps -> (vertices (M,3) float32, faces (F,3) int32)."""
    n = max(4, int(round(np.sqrt(n_faces / 2.0))))
    rs = np.random.RandomState(seed)
    th = np.pi * np.arange(1, n)[:, None] / n
    ph = 2 * np.pi * np.arange(n)[None, :] / n
    r = radius * (1.0 + sum(0.01 * np.sin(k * th + rs.uniform(0, 6)) * np.cos(k * ph) for k in (3, 7, 12)))
    body = np.stack([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th) + 0 * ph], -1).reshape(-1, 3)
    verts = np.concatenate([[[0, 0, radius]], body, [[0, 0, -radius]]]) + np.asarray(centre)
    ring = lambda i, j: 1 + (i - 1) * n + j % n
    j = np.arange(n)
    i = np.arange(1, n - 1)[:, None]
    south = len(verts) - 1
    faces = [np.stack([0 * j, ring(1, j), ring(1, j + 1)], 1), np.stack([south + 0 * j, ring(n - 1, j + 1), ring(n - 1, j)], 1),
             np.stack([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], -1).reshape(-1, 3),
             np.stack([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)], -1).reshape(-1, 3)]
    return verts.astype(np.float32), np.concatenate(faces).astype(np.int32)


def with_ground(verts, faces, half=400.0):
    """The mesh plus two triangles: the square |x|, |y| <= half of the plane z = 0, behind the sphere from every camera."""
    m = len(verts)
    quad = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float32)
    return np.concatenate([verts, quad]), np.concatenate([faces, np.array([[m, m + 1, m + 2], [m, m + 2, m + 3]], np.int32)])


def blocks_ms(fn, reps, warmup, blocks):
    """Median over `blocks` blocks of the median of `reps` calls -> (ms, min, max of the block medians)."""
    meds = [device_ms(fn, reps, warmup if b == 0 else 0)[0] for b in range(blocks)]
    return round(float(np.median(meds)), 3), round(min(meds), 3), round(max(meds), 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lane_reps", type=int, default=1, help="calls of the lane-only ground-plane case, not warmed up (each can take seconds)")
    ap.add_argument("--lane_views", type=int, default=4, help="views of the lane-only comparison")
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--faces", type=int, nargs="+", default=[2000000, 5000000])
    ap.add_argument("--sweep_faces", type=int, default=2000000, help="the sweep runs on the mesh of this size only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_raster needs a GPU")
    torch.cuda.set_device(0)
    from mvsnet_amd import render as Rn
    from mvsnet_amd import render_mesh as RM
    dev = torch.device("cuda", 0)
    out = {"metric": "raster_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "blocks": a.blocks, "views": a.views,
           "default_large_pixels": RM.LARGE_PIXELS, "default_queue_capacity": RM.QUEUE_CAPACITY, "results": []}
    for n_faces in a.faces:
        verts, faces = bumpy_sphere(n_faces)
        gverts, gfaces = with_ground(verts, faces)
        tv, tf = torch.as_tensor(verts).to(dev), torch.as_tensor(faces).to(dev)
        centroids = tv[tf.long()].mean(1).contiguous()
        for H, W in SIZES:
            cams = arc_cameras(a.views, H, W)
            plan = RM.RasterPlan(tv, tf, cams, H, W)
            row = {"faces": int(len(faces)), "vertices": int(len(verts)), "height": H, "width": W,
                   "pairs": int(len(faces)) * a.views, "pixels": a.views * H * W}
            row["mesh_ms"], row["mesh_ms_min"], row["mesh_ms_max"] = blocks_ms(plan.enqueue, a.reps, a.warmup, a.blocks)
            row["mesh_input_order_ms"] = blocks_ms(lambda: plan.enqueue(order=None), a.reps, a.warmup, a.blocks)[0]
            row["covered_pixels"] = int((plan.run()[1] >= 0).sum())
            del plan
            splat = Rn.RenderPlan(centroids, cams, H, W, splat=0)
            row["splat0_ms"], row["splat0_ms_min"], row["splat0_ms_max"] = blocks_ms(splat.enqueue, a.reps, a.warmup, a.blocks)
            row["mesh_over_splat0"] = round(row["mesh_ms"] / row["splat0_ms"], 2)
            del splat
            ground = RM.RasterPlan(gverts, gfaces, cams, H, W, queue_capacity=max(SWEEP_QUEUE))
            run = lambda **kw: (lambda: ground.enqueue(queue_capacity=RM.QUEUE_CAPACITY, **kw))
            row["ground_ms"], row["ground_ms_min"], row["ground_ms_max"] = blocks_ms(run(), a.reps, a.warmup, a.blocks)
            ground.run(queue_capacity=RM.QUEUE_CAPACITY)
            row["ground_queued_pairs"] = int(ground.workspace[:8].cpu().numpy().view(np.uint64)[0])
            # lane-only against the large path on the first --lane_views views: a lane takes the views of a call four at a
            # time, each a serial walk over the whole plane, so all 49 at 1152 x 864 would be a kernel of a minute
            few = RM.RasterPlan(gverts, gfaces, cams[:a.lane_views], H, W)
            row["lane_views"] = a.lane_views
            row["ground_few_ms"] = blocks_ms(few.enqueue, a.reps, a.warmup, a.blocks)[0]
            want = [x.clone() for x in few.run()]
            row["ground_few_lane_ms"] = round(device_ms(lambda: few.enqueue(large_pixels=1 << 30), a.lane_reps, 0)[0], 3)
            row["same_bytes"] = bool(torch.equal(few.depth.view(torch.int32), want[0].view(torch.int32)) and torch.equal(few.index, want[1]))
            row["large_path_speedup"] = round(row["ground_few_lane_ms"] / row["ground_few_ms"], 2)
            del few
            if n_faces == a.sweep_faces:
                row["sweep"] = [{"large_pixels": lp, "queue_capacity": qc,
                                 "ground_ms": blocks_ms(lambda: ground.enqueue(large_pixels=lp, queue_capacity=qc), a.reps, 1, a.blocks)[0]}
                                for lp in SWEEP_LARGE for qc in SWEEP_QUEUE]
            out["results"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del ground, want
            torch.cuda.empty_cache()
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
