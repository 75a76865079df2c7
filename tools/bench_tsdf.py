"""Times the TSDF fusion and the surface-nets extraction (csrc/tsdf.hip through mvsnet_amd.mesh) on bench_fusion.py's
sphere-and-plane scenes -- 48 and 144 views at 160 x 128, 135 at 288 x 216 -- into volumes of 256 and 512 nodes along the
longest axis, and prints one JSON line (also written to --out): milliseconds per integration of all views (device events
around mvs_tsdf_integrate_f32 on device-resident maps, median of --reps after --warmup) and per extraction (count, torch's
two scans, the read-back of the totals and write; wall time), each against a torch statement of the same integers and floats
in the same process: a loop over the views of element-wise tensor operations and a gather for the integration; slices,
cumsum, nonzero and gathers for the extraction.  Every row says in how many values the two differ (0: the same bytes).

    python tools/bench_tsdf.py [--reps 5] [--warmup 1] [--torch_reps 2] [--resolutions 256,512] [--out profiles/tsdf_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import fusion_reference as FR  # noqa: E402

CONFIGS = [(48, 128, 160), (144, 128, 160), (135, 216, 288)]
BOX = ((-2.0, -1.5, 3.0), (2.0, 1.5, 6.0))        # the sphere, the plane behind it and the truncation band in front of both
TRUNC_VOXELS = 4.0


def scene(V, H, W):
    return FR.make_scene("sphere", V=V, H=H, W=W, f=0.8 * W, arc_step_deg=70.0 / V, low_prob_fraction=0.05, seed=11)


def time_events(call, reps, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def time_wall(call, reps, warmup):
    import torch
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return float(np.median(times)), float(min(times)), float(max(times))


# ------------------------------------------------------------------------------------------------ the torch statement

def torch_integrate(vol, df, proj_host, H, W):
    """mesh.py's integration without colour: views in ascending order, every operation one rounded float32 tensor operation."""
    import torch
    nx, ny, nz = vol.dims
    dev = vol.dev
    o = [float(v) for v in vol.origin]
    ar = lambda n: torch.arange(n, device=dev, dtype=torch.float32)
    X = (o[0] + vol.voxel * ar(nx)).reshape(1, 1, nx)
    Y = (o[1] + vol.voxel * ar(ny)).reshape(1, ny, 1)
    Z = (o[2] + vol.voxel * ar(nz)).reshape(nz, 1, 1)
    s, c = torch.zeros((nz, ny, nx), device=dev), torch.zeros((nz, ny, nx), dtype=torch.int32, device=dev)
    P = proj_host.reshape(-1, 3, 4)
    # a tensor, not a number: torch turns a division by a number into a multiplication by its reciprocal
    trunc = torch.full((), vol.trunc, device=dev)
    for v in range(P.shape[0]):
        u, vv, w = [((float(P[v, r, 0]) * X + float(P[v, r, 1]) * Y) + float(P[v, r, 2]) * Z) + float(P[v, r, 3]) for r in range(3)]
        fx, fy = torch.floor(u / w + 0.5), torch.floor(vv / w + 0.5)
        cand = torch.isfinite(w) & (w > 0) & torch.isfinite(fx) & torch.isfinite(fy)
        cand &= (fx >= 0) & (fx <= float(W - 1)) & (fy >= 0) & (fy <= float(H - 1))
        zero = torch.zeros((), device=dev)
        at = torch.where(cand, fy * float(W) + fx, zero).long()                # exact in float32 below 2^24 pixels per view
        d = torch.where(cand, df[v].reshape(-1)[at], zero)
        sdf = d - w
        ok = cand & (d > 0) & ~(sdf < -trunc)
        s = torch.where(ok, s + torch.clamp(sdf / trunc, max=1.0), s)
        c += ok
    return s, c


def torch_extract(vol, min_count=1):
    """mesh.py's surface nets from the volume's sums -> (vertices, faces) device tensors."""
    import torch
    nx, ny, nz = vol.dims
    dev = vol.dev
    n = (nx - 1, ny - 1, nz - 1)
    obs = vol.count >= min_count
    f = torch.where(obs, vol.sum / vol.count.float(), torch.zeros((), device=dev))
    ins = obs & (f < 0)
    corner = lambda a, off: a[off[2]:off[2] + n[2], off[1]:off[1] + n[1], off[0]:off[0] + n[0]]
    offs = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    valid = torch.ones((n[2], n[1], n[0]), dtype=torch.bool, device=dev)
    nin = torch.zeros((n[2], n[1], n[0]), dtype=torch.int32, device=dev)
    for off in offs:
        valid &= corner(obs, off)
        nin += corner(ins, off)
    active = valid & (nin > 0) & (nin < 8)
    cid = torch.cumsum(active.reshape(-1), 0, dtype=torch.int32).reshape(active.shape) - 1
    kk, jj, ii = torch.nonzero(active, as_tuple=True)
    acc = [torch.zeros(len(ii), device=dev) for _ in range(3)]
    m = torch.zeros(len(ii), dtype=torch.int32, device=dev)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for off_c, off_b in ((0, 0), (0, 1), (1, 0), (1, 1)):
            lo, hi = [0, 0, 0], [0, 0, 0]
            lo[b] = hi[b] = off_b
            lo[c] = hi[c] = off_c
            hi[a] = 1
            at = lambda arr, off: arr[kk + off[2], jj + off[1], ii + off[0]]
            fa, fb = at(f, lo), at(f, hi)
            cross = at(ins, lo) != at(ins, hi)
            acc[a] = torch.where(cross, acc[a] + fa / (fa - fb), acc[a])
            acc[b] = torch.where(cross, acc[b] + float(off_b), acc[b])
            acc[c] = torch.where(cross, acc[c] + float(off_c), acc[c])
            m += cross
    md = m.float()
    o = [float(v) for v in vol.origin]
    verts = torch.stack([o[ax] + vol.voxel * (idx.float() + acc[ax] / md) for ax, idx in enumerate((ii, jj, kk))], 1)

    vpad = torch.zeros((nz + 1, ny + 1, nx + 1), dtype=torch.bool, device=dev)
    vpad[1:nz, 1:ny, 1:nx] = valid
    cpad = torch.full((nz + 1, ny + 1, nx + 1), -1, dtype=torch.int32, device=dev)
    cpad[1:nz, 1:ny, 1:nx] = cid
    shifted = lambda pad, sh: pad[1 - sh[2]:1 - sh[2] + nz, 1 - sh[1]:1 - sh[1] + ny, 1 - sh[0]:1 - sh[0] + nx]
    e = lambda *axes: tuple(1 if ax in axes else 0 for ax in range(3))
    cond = torch.zeros((nz, ny, nx, 3), dtype=torch.bool, device=dev)
    shifts = {}
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        shifts[a] = (e(b, c), e(c), e(), e(b))
        dim = 2 - a                                                            # tensor dimension of axis a
        nxt = lambda t: torch.cat([t.narrow(dim, 1, t.shape[dim] - 1), torch.zeros_like(t.narrow(dim, 0, 1))], dim)
        ok = obs & nxt(obs) & (ins != nxt(ins))
        for sh in shifts[a]:
            ok = ok & shifted(vpad, sh)
        cond[..., a] = ok
    fk, fj, fi, fa = torch.nonzero(cond, as_tuple=True)
    faces = torch.zeros((len(fk), 2, 3), dtype=torch.int32, device=dev)
    inq = ins[fk, fj, fi]
    for a in range(3):
        sel = fa == a
        k_, j_, i_ = fk[sel], fj[sel], fi[sel]
        c0, c1, c2, c3 = (cpad[k_ + 1 - sh[2], j_ + 1 - sh[1], i_ + 1 - sh[0]] for sh in shifts[a])
        q = inq[sel][:, None]
        faces[sel, 0] = torch.where(q, torch.stack([c0, c1, c2], 1), torch.stack([c0, c2, c1], 1))
        faces[sel, 1] = torch.where(q, torch.stack([c0, c2, c3], 1), torch.stack([c0, c3, c2], 1))
    return verts, faces.reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ cases

def run_case(s, V, H, W, resolution, a):
    import torch
    from mvsnet_amd import _lib, mesh
    from mvsnet_amd.render import projection_tables
    origin, voxel, dims = mesh.choose_volume(BOX[0], BOX[1], resolution=resolution)
    vol = mesh.TsdfVolume(origin, voxel, dims, TRUNC_VOXELS * voxel)
    lib = _lib.load()
    d, p = torch.as_tensor(s["depths"]).cuda(), torch.as_tensor(s["probs"]).cuda()
    proj_host = projection_tables(s["cams"])
    proj = torch.as_tensor(proj_host).cuda()
    ws = torch.empty(lib.mvs_tsdf_integrate_workspace_bytes(V, H, W), dtype=torch.uint8, device="cuda")
    o = (ctypes.c_float * 3)(*[float(v) for v in vol.origin])
    nx, ny, nz = dims

    def integrate():
        _lib.check(lib.mvs_tsdf_integrate_f32(_lib.ptr(d), _lib.ptr(p), V, H, W, _lib.ptr(proj), None, 0, 0, o, vol.voxel, nx, ny, nz,
                                              vol.trunc, 0.8, 0, _lib.ptr(vol.sum), _lib.ptr(vol.count), None, None, _lib.ptr(ws),
                                              ws.numel(), _lib.stream_ptr()), "mvs_tsdf_integrate_f32")

    row = {"views": V, "H": H, "W": W, "resolution": resolution, "dims": list(dims), "nodes": nx * ny * nz}
    med, lo, hi = time_events(integrate, a.reps, a.warmup)
    row.update({"integrate_ms": round(med, 3), "integrate_ms_min": round(lo, 3), "integrate_ms_max": round(hi, 3),
                "ns_per_node_view": round(med * 1e6 / (float(nx) * ny * nz * V), 5)})
    vol.sum.zero_(), vol.count.zero_()
    integrate()
    row["observed_nodes"] = int((vol.count > 0).sum())
    if a.torch_reps > 0:
        df = torch.where((d > 0) & torch.isfinite(d) & (p >= 0.8), d, torch.zeros((), device="cuda"))
        out = []
        med, lo, hi = time_events(lambda: out.__setitem__(slice(None), [torch_integrate(vol, df, proj_host, H, W)]), a.torch_reps, 1)
        ts, tc = out[0]
        row.update({"integrate_ms_torch": round(med, 3), "integrate_torch_differs":
                    int((ts.view(torch.int32) != vol.sum.view(torch.int32)).sum()) + int((tc != vol.count).sum())})
        del out, ts, tc, df
    if a.extract:
        got = []
        med, lo, hi = time_wall(lambda: got.__setitem__(slice(None), [vol.extract()]), a.reps, a.warmup)
        v, c, f = got[0]
        row.update({"extract_ms": round(med, 3), "extract_ms_min": round(lo, 3), "extract_ms_max": round(hi, 3),
                    "vertices": int(len(v)), "faces": int(len(f))})
        if a.torch_reps > 0:
            out = []
            med, lo, hi = time_wall(lambda: out.__setitem__(slice(None), [torch_extract(vol)]), a.torch_reps, 1)
            tv, tf = out[0]
            tv, tf = tv.cpu().numpy(), tf.cpu().numpy()
            same_shape = tv.shape == v.shape and tf.shape == f.shape
            row.update({"extract_ms_torch": round(med, 3), "extract_torch_differs":
                        int((tv.view(np.uint32) != v.view(np.uint32)).sum()) + int((tf != f).sum()) if same_shape else -1})
            del out, tv, tf
    del vol
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch_reps", type=int, default=2, help="repetitions of the torch statement (0: leave it out)")
    ap.add_argument("--resolutions", default="256,512")
    ap.add_argument("--configs", default="0,1,2", help="which of the three view sets to run")
    ap.add_argument("--no-extract", dest="extract", action="store_false", help="time the integration only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs a GPU")
    torch.cuda.set_device(0)
    out = {"metric": "tsdf_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "torch_reps": a.torch_reps,
           "trunc_voxels": TRUNC_VOXELS, "box": BOX, "results": []}
    for k in (int(t) for t in a.configs.split(",")):
        V, H, W = CONFIGS[k]
        s = scene(V, H, W)
        for resolution in (int(t) for t in a.resolutions.split(",")):
            out["results"].append(run_case(s, V, H, W, resolution, a))
            print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
