"""Times the mesh simplification (csrc/mesh_simplify.hip through mvsnet_amd.mesh_simplify) and prints one JSON line (also
written to --out, default profiles/mesh_simplify_bench.json).  Meshes: bench_tsdf.py's own extractions at 256 and 512 nodes
(144 views of 160 x 128) with cells of 2 and 4 voxels aligned to the volume, and bench_raster.py's bumpy sphere at about 2 M
and 5 M faces, in input order and with the face order shuffled, with cells of 2 and 4 equatorial edges; the 512-node mesh and
the 2 M sphere also with one cell around everything (every sum lands on one cluster).  Per row, with bench_tsdf.py's protocol
(device events, median of --reps after --warmup, _min and _max kept): each of the five library calls on its own, torch's two
sorts and three scans between them, and the whole simplify_device call on device tensors as wall time (it holds the read-back).
The yardstick is the same statement written in torch on the same device (unique, index_add_, sorts), which must give the same
bytes: the row says whether it did.

    python tools/bench_mesh_simplify.py [--reps 5] [--warmup 1] [--rows tsdf256@2,tsdf512@4,sphere2m@one,...] [--no-torch] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import bench_raster  # noqa: E402
import bench_tsdf  # noqa: E402
from bench_tsdf import time_events, time_wall  # noqa: E402

TSDF_CONFIG = 1                                   # 144 views of 160 x 128
ROWS = ["tsdf256@2", "tsdf256@4", "tsdf512@2", "tsdf512@4", "tsdf512@one", "sphere2m@2", "sphere2m@4", "sphere2m@one",
        "sphere2m_shuffled@2", "sphere2m_shuffled@4", "sphere5m@2", "sphere5m@4", "sphere5m_shuffled@2", "sphere5m_shuffled@4"]
_MESHES = {}


def make_mesh(name):
    """-> (vertices, faces, origin (3,) float32, unit: the length a cell is a multiple of, extra row fields), cached."""
    if name in _MESHES:
        return _MESHES[name]
    if name.startswith("tsdf"):
        from mvsnet_amd import mesh
        resolution = int(name[4:])
        V, H, W = bench_tsdf.CONFIGS[TSDF_CONFIG]
        s = bench_tsdf.scene(V, H, W)
        origin, voxel, dims = mesh.choose_volume(bench_tsdf.BOX[0], bench_tsdf.BOX[1], resolution=resolution)
        vol = mesh.TsdfVolume(origin, voxel, dims, bench_tsdf.TRUNC_VOXELS * voxel)
        vol.integrate(s["depths"], s["probs"], s["cams"])
        v, _, f = vol.extract()
        out = (v, f, vol.origin, vol.voxel, {"resolution": resolution, "unit": "voxel"})
    elif name.startswith("sphere"):
        n = int(name[6]) * 1000000
        v, f = bench_raster.bumpy_sphere(n)
        if name.endswith("_shuffled"):
            f = f[np.random.RandomState(0).permutation(len(f))]
        edge = 2 * np.pi * 120.0 / max(4, int(round(np.sqrt(n / 2.0))))
        out = (v, f, v.min(0) - np.float32(1), edge, {"unit": "equatorial edge"})
    else:
        raise SystemExit("unknown mesh %r" % name)
    _MESHES.clear()                                                            # one mesh at a time stays in memory
    _MESHES[name] = out
    return out


def torch_simplify(v, f, cell, origin):
    """mesh_simplify.py's statement in torch, without colours -> (vertices, faces) on the device."""
    import torch
    M, cell = v.shape[0], float(np.float32(cell))
    o = torch.as_tensor(np.asarray(origin, np.float64), device=v.device)
    u = (v.double() - o) / torch.tensor(cell, dtype=torch.float64, device=v.device)    # a tensor: torch multiplies by the reciprocal of a number
    k = torch.floor(u)
    ok = torch.isfinite(v).all(1) & ((k >= 0) & (k <= 2 ** 21 - 1)).all(1)
    q = torch.where(ok[:, None], torch.floor((u - k) * 2.0 ** 20), torch.zeros_like(u)).long()
    kk = torch.where(ok[:, None], k, torch.zeros_like(k)).long()
    key = kk[:, 0] | (kk[:, 1] << 21) | (kk[:, 2] << 42)
    fl = f.long()
    inside = ((fl >= 0) & (fl < M)).all(1)
    valid = inside & ok[fl.clamp(0, max(M - 1, 0))].all(1)
    used = torch.zeros(M, dtype=torch.bool, device=v.device)
    used[fl[valid].reshape(-1)] = True
    ukeys, inverse = torch.unique(key[used], return_inverse=True)
    K = ukeys.numel()
    n = torch.bincount(inverse, minlength=K)
    S = torch.zeros((K, 3), dtype=torch.int64, device=v.device).index_add_(0, inverse, q[used])
    kc = torch.stack([ukeys & (2 ** 21 - 1), (ukeys >> 21) & (2 ** 21 - 1), ukeys >> 42], 1)
    b = kc.double() + S.double() / (n * 2 ** 20).double()[:, None]
    pos = (o + b * float(cell)).float()
    cluster = torch.full((M,), -1, dtype=torch.int64, device=v.device)
    cluster[used] = inverse
    index = torch.nonzero(valid).flatten()
    g = cluster[fl[index]]
    live = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 0] != g[:, 2])
    index, g = index[live], g[live]
    t = torch.sort(g, 1)[0]
    if K <= 2 ** 21:
        skey, order = torch.sort((t[:, 0] << 42) | (t[:, 1] << 21) | t[:, 2], stable=True)
        first = torch.ones_like(skey, dtype=torch.bool)
        first[1:] = skey[1:] != skey[:-1]
    else:
        lo, by_lo = torch.sort((t[:, 1] << 32) | t[:, 2], stable=True)
        hi, by_hi = torch.sort(t[by_lo, 0], stable=True)
        lo, order = lo[by_hi], by_lo[by_hi]
        first = torch.ones_like(hi, dtype=torch.bool)
        first[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    kept = g[torch.sort(order[first])[0]]
    vk = torch.zeros(K, dtype=torch.bool, device=v.device)
    vk[kept.reshape(-1)] = True
    new = torch.cumsum(vk, 0) - 1
    return pos[vk], new[kept].to(torch.int32)


class Steps:
    """simplify_device call by call on tensors that stay allocated, so that every library call can be timed on its own."""

    def __init__(self, tv, tf, cell, origin, dev):
        import torch
        from mvsnet_amd import _lib, mesh_simplify
        self.lib, self.L, self.torch = _lib.load(), _lib, torch
        self.tv, self.tf, self.M, self.F = tv, tf, int(tv.shape[0]), int(tf.shape[0])
        self.grid = [float(x) for x in origin] + [mesh_simplify.check_cell(cell)]
        M, F = self.M, self.F
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        self.wsb = self.lib.mvs_mesh_cluster_workspace_bytes(M, F)
        self.ws = new(self.wsb, torch.uint8)
        self.keys_, self.offsets = new(M, torch.int64), new((M, 3), torch.int32)
        self.head, self.vc, self.cv = new(M, torch.int32), new(M, torch.int32), new((M, 3), torch.float32)
        self.cf, self.lo = new((F, 3), torch.int32), new(F, torch.int64)
        self.fk, self.vk = new(F, torch.int32), new(M, torch.int32)
        self.two = M > mesh_simplify.CELLS
        self.hi = new(F, torch.int64) if self.two else None

    def keys(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_cluster_keys_f32(p(self.tv), self.M, p(self.tf), self.F, *self.grid, p(self.keys_), p(self.offsets),
                                                   p(self.ws), self.wsb, L.stream_ptr()), "keys")

    def sort_vertices(self):
        self.sk, self.order = self.torch.sort(self.keys_, stable=True)

    def heads(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_cluster_heads_i64(p(self.sk), self.M, p(self.head), L.stream_ptr()), "heads")

    def scan_heads(self):
        self.rank = self.torch.cumsum(self.head, 0, dtype=self.torch.int32)

    def sums(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_cluster_sums_f32(p(self.sk), p(self.order), p(self.rank), p(self.offsets), None, self.M, *self.grid,
                                                   p(self.vc), p(self.cv), None, p(self.ws), self.wsb, L.stream_ptr()), "sums")

    def faces(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_cluster_faces_i32(p(self.tf), self.M, self.F, p(self.vc), p(self.cf), p(self.lo), p(self.hi), p(self.ws),
                                                    self.wsb, L.stream_ptr()), "faces")

    def sort_faces(self):
        torch = self.torch
        if self.two:
            lo1, by_lo = torch.sort(self.lo, stable=True)
            self.shi, by_hi = torch.sort(self.hi[by_lo], stable=True)
            self.slo, self.forder = lo1[by_hi].contiguous(), by_lo[by_hi].contiguous()
        else:
            (self.slo, self.forder), self.shi = torch.sort(self.lo, stable=True), None

    def mark(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_cluster_mark_i32(p(self.cf), self.M, self.F, p(self.slo), p(self.shi), p(self.forder), p(self.fk),
                                                   p(self.vk), p(self.ws), self.wsb, L.stream_ptr()), "mark")

    def scan_keeps(self):
        self.frank = self.torch.cumsum(self.fk, 0, dtype=self.torch.int32)
        self.vrank = self.torch.cumsum(self.vk, 0, dtype=self.torch.int32)

    ORDER = ("keys", "sort_vertices", "heads", "scan_heads", "sums", "faces", "sort_faces", "mark", "scan_keeps")


def run_row(spec, a):
    import torch
    from mvsnet_amd import mesh_simplify
    name, mult = spec.split("@")
    v, f, origin, unit, extra = make_mesh(name)
    if mult == "one":
        cell, origin = float(np.float32(4 * np.ptp(v, 0).max())), v.min(0) - np.float32(1)
    else:
        cell = float(np.float32(float(mult) * unit))
    dev = torch.device("cuda", torch.cuda.current_device())
    tv, tf = torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev)
    row = dict({"row": spec, "mesh": name, "cell_in_units": mult, "cell": cell, "vertices": int(len(v)), "faces": int(len(f))}, **extra)

    def put(key, t):
        row.update({key: round(t[0], 4), key + "_min": round(t[1], 4), key + "_max": round(t[2], 4)})

    out = mesh_simplify.simplify_device(tv, None, tf, dev, cell, origin)
    row.update({k: out[3][k] for k in ("clusters", "vertices_out", "faces_out", "degenerate_faces", "duplicate_faces", "invalid_faces")})
    steps = Steps(tv, tf, cell, origin, dev)
    row["two_keys"] = steps.two
    for step in Steps.ORDER:                                                   # each step needs what the steps before it left
        getattr(steps, step)()
    for step in Steps.ORDER:
        put(step + "_ms", time_events(getattr(steps, step), a.reps, a.warmup))
    row["library_ms"] = round(sum(row[s + "_ms"] for s in ("keys", "heads", "sums", "faces", "mark")), 4)
    row["torch_between_ms"] = round(sum(row[s + "_ms"] for s in ("sort_vertices", "scan_heads", "sort_faces", "scan_keeps")), 4)
    put("simplify_ms", time_wall(lambda: mesh_simplify.simplify_device(tv, None, tf, dev, cell, origin), a.reps, a.warmup))
    del steps
    if a.torch:
        tov, tof = torch_simplify(tv, tf, cell, origin)
        row["torch_same_bytes"] = bool(tov.shape == out[0].shape and tof.shape == out[2].shape and
                                       tov.cpu().numpy().tobytes() == out[0].cpu().numpy().tobytes() and torch.equal(tof, out[2]))
        del tov, tof
        put("torch_statement_ms", time_wall(lambda: torch_simplify(tv, tf, cell, origin), a.reps, a.warmup))
    del tv, tf, out
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no-torch", dest="torch", action="store_false", help="leave the torch yardstick out")
    ap.add_argument("--variant", default="product", help="a name for the library build that is measured (MVS_LIB_PATH)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify needs a GPU")
    torch.cuda.set_device(0)
    out = {"metric": "mesh_simplify_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "variant": a.variant, "results": []}
    for spec in a.rows.split(","):
        out["results"].append(run_row(spec, a))
        print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
