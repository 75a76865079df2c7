"""Times the vertex normals and the colouring from the images (csrc/mesh_colour.hip through mvsnet_amd.mesh_colour) and prints one
JSON line (also written to --out, default profiles/mesh_colour_bench.json).  Mesh: bench_mesh_smooth.py's grid of 1000 x 1000
quads over a noisy height field (2 M faces), numbered as an extraction numbers its vertices, and again with the vertex numbers
shuffled, as a foreign mesh may come.  Views: 49 cameras on a 7 x 7 grid above it, at 1600 x 1200 and at 640 x 512, with seeded
random uint8 images on the device.  Per row, with bench_tsdf.py's protocol (device events, median of --reps after --warmup, _min
and _max kept), apart from each other: the normals (keys, torch's sort, normals; the sort alone beside it), the rasteriser's
depth maps of the 49 views in one call, the accumulation of the 49 views in one call on those maps, the finish; and the whole
colour_device call on device tensors as wall time (chunks of 8 views, with its plans and its read-back).  The bytes the
accumulation needs are counted from the shapes and the visits it made (seen.sum()), and given over its time as GB/s beside the
6 300 GB/s a streaming pass reaches on this part.  The yardstick is the same computation written with torch
operations on the same device: index_add_ of the face normals in float64, and per view element-wise tensor operations with
gathers for the depth and the four taps; each row says in how many values the two differ.

    python tools/bench_mesh_colour.py [--reps 7] [--warmup 2] [--rows grid1000@1200x1600,...] [--no-torch] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_mesh_smooth import make_mesh  # noqa: E402
from bench_tsdf import time_events, time_wall  # noqa: E402

ROWS = ["grid1000@1200x1600", "grid1000@512x640", "grid1000_shuffled@1200x1600", "grid1000_shuffled@512x640"]
VIEWS_PER_AXIS = 7
STREAM_GBPS = 6300.0


def look_down(eye, target, f, H, W):
    """cam (2,4,4) at `eye` looking at `target`, image x along world x as far as the direction allows."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, -1.0, 0.0], z)
    x /= np.linalg.norm(x)
    cam = np.zeros((2, 4, 4))
    cam[0] = np.eye(4)
    cam[0, :3, :3] = np.stack([x, np.cross(z, x), z])
    cam[0, :3, 3] = -cam[0, :3, :3] @ eye
    cam[1, :3, :3] = [[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]]
    return cam


def make_cams(n, H, W):
    """49 cameras 1.4 n above the n x n height field (its faces wind towards +z), each looking at a point a third of the way
    from the middle to the spot below it."""
    at = np.linspace(0.1 * n, 0.9 * n, VIEWS_PER_AXIS)
    mid = 0.5 * n
    return np.stack([look_down((ex, ey, 1.4 * n), (mid + 0.3 * (ex - mid), mid + 0.3 * (ey - mid), 0.0), 1.1 * W, H, W) for ey in at for ex in at])


def accumulate_bytes(M, visits):
    """What the accumulation has to move: per vertex its position, its normal, the row of four sums in and out and the count in
    and out; per visit a depth and four taps of three bytes."""
    return M * (12 + 12 + 32 + 32 + 4 + 4) + visits * (4 + 12)


# ------------------------------------------------------------------------------------------------ the torch statement

def torch_normals(tv, tf):
    import torch
    f = tf.long()
    p = tv.double()
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    n = torch.cross(b - a, c - a, dim=1)
    s = torch.zeros_like(p)
    for k in range(3):
        s.index_add_(0, f[:, k], n)
    length = s.norm(dim=1, keepdim=True)
    return torch.where((length > 0) & torch.isfinite(length), s / length, torch.zeros_like(s)).float()


def torch_accumulate(tv, tn, proj, centres, depth, images, ratio, min_cos, power, acc, seen):
    import torch
    V, H, W = depth.shape
    x, y, z = tv[:, 0], tv[:, 1], tv[:, 2]
    live = torch.isfinite(tv).all(1) & (tn != 0).any(1)
    nd, pd = tn.double(), tv.double()
    for v in range(V):
        P = proj[12 * v:12 * v + 12]
        u, t, w = [((P[4 * r] * x + P[4 * r + 1] * y) + P[4 * r + 2] * z) + P[4 * r + 3] for r in range(3)]
        sx, sy = u / w, t / w
        px, py = torch.floor(sx + 0.5), torch.floor(sy + 0.5)
        inside = live & torch.isfinite(w) & (w > 0) & torch.isfinite(sx) & torch.isfinite(sy) & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
        at = torch.where(inside, py * W + px, torch.zeros_like(px)).long()
        zb = depth[v].reshape(-1)[at]
        d = centres[v].double()[None, :] - pd
        q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        c = ((nd[:, 0] * d[:, 0] + nd[:, 1] * d[:, 1]) + nd[:, 2] * d[:, 2]) / torch.sqrt(q)
        sees = inside & (zb > 0) & (w <= zb * ratio) & (q > 0) & (c >= min_cos)
        g = torch.ones_like(c)
        for k in range(power):
            g = c if k == 0 else g * c
        x0, y0 = torch.floor(sx), torch.floor(sy)
        fx, fy = sx - x0, sy - y0
        clamp = lambda a, top: torch.where(sees, a.clamp(0, top), torch.zeros_like(a)).long()
        xa, xb, ya, yb = clamp(x0, W - 1), clamp(x0 + 1, W - 1), clamp(y0, H - 1), clamp(y0 + 1, H - 1)
        im = images[v].reshape(-1, 3)
        tap = lambda yy, xx: im[yy * W + xx].float()
        top = (1 - fx)[:, None] * tap(ya, xa) + fx[:, None] * tap(ya, xb)
        bot = (1 - fx)[:, None] * tap(yb, xa) + fx[:, None] * tap(yb, xb)
        s = (1 - fy)[:, None] * top + fy[:, None] * bot
        zero = torch.zeros_like(g)
        acc[:, :3] += torch.where(sees[:, None], g[:, None] * s.double(), zero[:, None])
        acc[:, 3] += torch.where(sees, g, zero)
        seen += sees.int()


# ------------------------------------------------------------------------------------------------ one row

def run_row(name, a):
    import torch
    from mvsnet_amd import _lib, mesh_colour
    from mvsnet_amd.render import projection_tables
    from mvsnet_amd.render_mesh import RasterPlan
    mesh_name, size = name.split("@")
    H, W = (int(s) for s in size.split("x"))
    v, f = make_mesh(mesh_name)
    n = int(mesh_name[4:].split("_")[0])
    cams = make_cams(n, H, W)
    V, M, F = len(cams), len(v), len(f)
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream_ptr
    tv, tf = torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev)
    images = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    min_cos, power, rel, min_depth, chunk = mesh_colour.check_options()
    ratio = mesh_colour.occlusion_ratio(rel)
    row = {"row": name, "vertices": M, "faces": F, "views": V, "height": H, "width": W, "view_chunk": chunk}

    def put(key, t):
        row.update({key: round(t[0], 4), key + "_min": round(t[1], 4), key + "_max": round(t[2], 4)})

    ws = mesh_colour._Workspace(M, F, dev)
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    put("normals_ms", time_events(lambda: mesh_colour.normals_device(tv, tf, dev, ws), a.reps, a.warmup))
    _lib.check(lib.mvs_mesh_normals_keys_i64(p(tv), M, p(tf), F, p(keys), p(ws.t), ws.bytes, st()), "keys")
    put("normals_sort_ms", time_events(lambda: torch.sort(keys), a.reps, a.warmup))
    normals = mesh_colour.normals_device(tv, tf, dev, ws)[0]
    plan = RasterPlan(tv, tf, cams, H, W, device=dev)
    put("raster_ms", time_events(lambda: plan.enqueue(index=False), a.reps, a.warmup))
    depth = plan.run(index=False)[0]
    proj = torch.as_tensor(projection_tables(cams)).to(dev)
    centres = torch.as_tensor(mesh_colour.camera_centres(cams)).to(dev)
    acc, seen = torch.zeros((M, 4), dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)
    out = torch.empty((M, 3), dtype=torch.uint8, device=dev)

    def accumulate():
        _lib.check(lib.mvs_mesh_colour_accumulate_f32(p(tv), p(normals), M, p(proj), p(centres), V, H, W, p(depth), p(images), min_depth,
                                                      ratio, min_cos, power, p(acc), p(seen), st()), "accumulate")

    def finish():
        _lib.check(lib.mvs_mesh_colour_finish_u8(None, p(acc), p(seen), M, p(out), p(ws.t), ws.bytes, st()), "finish")

    put("accumulate_ms", time_events(accumulate, a.reps, a.warmup))
    put("finish_ms", time_events(finish, a.reps, a.warmup))
    acc.zero_()
    seen.zero_()
    accumulate()
    finish()
    visits = int(seen.sum())
    row["visits"], row["unseen_vertices"] = visits, int((seen == 0).sum())
    row["accumulate_bytes"] = accumulate_bytes(M, visits)
    row["accumulate_GBps"] = round(row["accumulate_bytes"] / row["accumulate_ms"] / 1e6, 1)
    row["accumulate_share_of_streaming"] = round(row["accumulate_GBps"] / STREAM_GBPS, 4)
    stages = row["normals_ms"] + row["raster_ms"] + row["accumulate_ms"] + row["finish_ms"]
    row["raster_share_of_stages"] = round(row["raster_ms"] / stages, 4)
    views = [images[k] for k in range(V)]
    whole = mesh_colour.colour_device(tv, None, tf, dev, cams, views)
    row["chunked_same_bytes"] = bool(torch.equal(whole[1], out))
    put("colour_device_ms", time_wall(lambda: mesh_colour.colour_device(tv, None, tf, dev, cams, views), a.reps, a.warmup))
    if a.torch:
        tn = torch_normals(tv, tf)
        row["torch_normals_differing"] = int((tn != normals).sum())
        row["torch_normals_max_abs_difference"] = float((tn - normals).abs().max())
        put("torch_normals_ms", time_events(lambda: torch_normals(tv, tf), a.reps, a.warmup))
        tacc, tseen = torch.zeros_like(acc), torch.zeros_like(seen)
        go = lambda: torch_accumulate(tv, normals, proj, centres, depth, images, ratio, min_cos, power, tacc, tseen)
        go()
        row["torch_acc_differing"], row["torch_seen_differing"] = int((tacc != acc).sum()), int((tseen != seen).sum())
        put("torch_accumulate_ms", time_events(go, max(1, a.reps // 2), 1))
    del plan, depth, images, views, whole
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no-torch", dest="torch", action="store_false", help="leave the torch yardstick out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_colour_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_colour needs a GPU")
    torch.cuda.set_device(0)
    out = {"metric": "mesh_colour_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "stream_GBps": STREAM_GBPS, "results": []}
    for name in a.rows.split(","):
        out["results"].append(run_row(name, a))
        print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
