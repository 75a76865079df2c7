"""Times the surface sampling (csrc/mesh_sample.hip through mvsnet_amd.mesh_sample) and prints one JSON line (also written to
--out, default profiles/mesh_sample_bench.json).  Meshes: bench_mesh_simplify.py's (bench_tsdf.py's extractions at 256 and 512
nodes, bench_raster.py's bumpy sphere at about 2 M and 5 M faces, ordered and with the face order shuffled) and the 512-node
mesh after a simplification in cells of 4 voxels (tsdf512s4); each at the spacings that give about 1 M, 10 M and 50 M samples.
Per row, with bench_tsdf.py's protocol (device events, median of --reps after --warmup, _min and _max kept): the quota call,
torch's scan, the write call with the positions alone and with every output, and the whole sample_device call as wall time (it
holds the read-back).  Two yardsticks, neither of them the code under test: the same statement written in torch on the same
device (repeat_interleave, gathers, float64 arithmetic), with whether it gave the same bytes; and the streaming floor of the
write call from its bytes (N x (12 + what was asked for) written, the faces and the vertices read once) over the rate of a
device-to-device copy measured in the same process.

    python tools/bench_mesh_sample.py [--reps 5] [--warmup 1] [--rows tsdf512,sphere2m_shuffled,...] [--targets 1,10,50]
                                      [--no-torch] [--variant NAME] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import bench_mesh_simplify  # noqa: E402
from bench_tsdf import time_events, time_wall  # noqa: E402

ROWS = ["tsdf256", "tsdf512", "tsdf512s4", "sphere2m", "sphere2m_shuffled", "sphere5m", "sphere5m_shuffled"]
TARGETS = [1, 10, 50]                              # millions of samples


def make_mesh(name, dev):
    """-> (vertices, faces) as device tensors."""
    import torch
    if name == "tsdf512s4":
        from mvsnet_amd import mesh_simplify
        v, f, origin, voxel, _ = bench_mesh_simplify.make_mesh("tsdf512")
        tv, _, tf, _ = mesh_simplify.simplify_device(torch.as_tensor(v).to(dev), None, torch.as_tensor(f).to(dev), dev,
                                                     float(np.float32(4 * voxel)), origin)
        return tv, tf
    v, f = bench_mesh_simplify.make_mesh(name)[:2]
    return torch.as_tensor(v).to(dev), torch.as_tensor(np.ascontiguousarray(f)).to(dev)


def _lsr(x, k):
    """Logical shift right of the 64 bits held in an int64 tensor."""
    return (x >> k) & ((1 << (64 - k)) - 1)


def _i64(c):
    return c - (1 << 64) if c >= 1 << 63 else c


def _mix(x):
    x = x + _i64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def torch_sample(v, f, density, seed=0, normals=False):
    """mesh_sample.py's statement in torch (int64 holds the hash's 64 bits; the products wrap) -> (xyz, normals or None)."""
    import torch
    M = v.shape[0]
    fl = f.long()
    inside = ((fl >= 0) & (fl < M)).all(1)
    tri = v[fl.clamp(0, max(M - 1, 0))].double()
    valid = inside & torch.isfinite(tri).all(2).all(1)
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    e1, e2 = b - a, c - a
    n = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    A2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    t = ((torch.sqrt(A2) * 0.5) * density) * 65536.0
    ok = valid & (A2 != 0) & (t < 2.0 ** 36)
    q = torch.where(ok, torch.floor(torch.where(ok, t, torch.zeros_like(t))), torch.zeros_like(t)).long()
    I = torch.cumsum(q, 0)
    per_face = (I >> 16) - ((I - q) >> 16)
    face = torch.repeat_interleave(torch.arange(f.shape[0], device=v.device), per_face)
    N = face.shape[0]
    g = torch.arange(N, device=v.device, dtype=torch.int64)
    h = _mix(_mix(torch.tensor([_i64(int(seed))], device=v.device, dtype=torch.int64)) ^ g)
    k1, k2 = _lsr(h, 40), _lsr(h, 16) & 0xFFFFFF
    fold = k1 + k2 >= 2 ** 24
    k1, k2 = torch.where(fold, 2 ** 24 - 1 - k1, k1), torch.where(fold, 2 ** 24 - 1 - k2, k2)
    u, w = ((2 * k1 + 1).double() * 2.0 ** -25)[:, None], ((2 * k2 + 1).double() * 2.0 ** -25)[:, None]
    a, b, c = a[face], b[face], c[face]
    xyz = ((a + u * (b - a)) + w * (c - a)).float()
    nrm = (n[face] / torch.sqrt(A2[face])[:, None]).float() if normals else None
    return xyz, nrm


class Steps:
    """sample_device call by call on tensors that stay allocated, so that every library call can be timed on its own."""

    def __init__(self, tv, tf, density, dev):
        import torch
        from mvsnet_amd import _lib
        self.lib, self.L, self.torch = _lib.load(), _lib, torch
        self.tv, self.tf, self.M, self.F, self.density = tv, tf, int(tv.shape[0]), int(tf.shape[0]), float(density)
        self.new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        self.wsb = self.lib.mvs_mesh_sample_workspace_bytes(self.M, self.F)
        self.ws, self.q = self.new(self.wsb, torch.uint8), self.new(self.F, torch.int64)

    def quota(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_sample_quota_f32(p(self.tv), self.M, p(self.tf), self.F, self.density, p(self.q), p(self.ws), self.wsb,
                                                   L.stream_ptr()), "quota")

    def scan(self):
        self.sums = self.torch.cumsum(self.q, 0, dtype=self.torch.int64)

    def allocate(self):
        torch = self.torch
        self.N = int(self.sums[-1]) >> 16
        self.xyz, self.nrm = self.new((self.N, 3), torch.float32), self.new((self.N, 3), torch.float32)
        self.face = self.new(self.N, torch.int32)

    def write(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_sample_write_f32(p(self.tv), None, self.M, p(self.tf), self.F, p(self.sums), self.N, 0, p(self.xyz), None,
                                                   None, None, L.stream_ptr()), "write")

    def write_all(self):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_sample_write_f32(p(self.tv), None, self.M, p(self.tf), self.F, p(self.sums), self.N, 0, p(self.xyz),
                                                   p(self.face), None, p(self.nrm), L.stream_ptr()), "write")


def copy_rate(dev, a):
    """Bytes per second of a device-to-device copy of 1 GiB (read plus written), by the same protocol."""
    import torch
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = time_events(lambda: dst.copy_(src), a.reps, a.warmup)
    return 2.0 * (1 << 30) / (ms[0] * 1e-3), ms


def run_row(name, tv, tf, target, rate, a):
    import torch
    from mvsnet_amd import mesh_sample
    dev = tv.device
    tri = tv[tf.long()].double()
    area = float(0.5 * torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1).sum())
    del tri
    spacing = float(np.sqrt(area / (target * 1e6)))
    density = mesh_sample.check_spacing(spacing)
    row = {"row": "%s@%dM" % (name, target), "mesh": name, "vertices": int(tv.shape[0]), "faces": int(tf.shape[0]), "spacing": spacing,
           "density": density}

    def put(key, t):
        row.update({key: round(t[0], 4), key + "_min": round(t[1], 4), key + "_max": round(t[2], 4)})

    out, stats = mesh_sample.sample_device(tv, None, tf, dev, density, normals=True, face_index=True)
    row.update(stats)
    steps = Steps(tv, tf, density, dev)
    steps.quota()
    steps.scan()
    steps.allocate()
    assert steps.N == stats["samples"]
    for step in ("quota", "scan", "write", "write_all"):
        put(step + "_ms", time_events(getattr(steps, step), a.reps, a.warmup))
    N, M, F = steps.N, steps.M, steps.F
    for key, per in (("write", 12), ("write_all", 12 + 4 + 12)):
        nbytes = N * per + F * (12 + 8) + M * 12                               # samples written; faces, their sums and the vertices read once
        row[key + "_bytes"] = nbytes
        row[key + "_floor_ms"] = round(nbytes / rate * 1e3, 4)
        row[key + "_floor_fraction"] = round(row[key + "_floor_ms"] / row[key + "_ms"], 4)
    del steps
    put("sample_device_ms", time_wall(lambda: mesh_sample.sample_device(tv, None, tf, dev, density), a.reps, a.warmup))
    if a.torch:
        txyz, tnrm = torch_sample(tv, tf, density, 0, True)
        row["torch_same_bytes"] = bool(txyz.shape == out["xyz"].shape and torch.equal(txyz.view(torch.int32), out["xyz"].view(torch.int32)) and
                                       torch.equal(tnrm.view(torch.int32), out["normals"].view(torch.int32)))
        del txyz, tnrm
        put("torch_statement_ms", time_wall(lambda: torch_sample(tv, tf, density), a.reps, a.warmup))
    del out
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--targets", default=",".join(str(t) for t in TARGETS), help="millions of samples per row")
    ap.add_argument("--no-torch", dest="torch", action="store_false", help="leave the torch yardstick out")
    ap.add_argument("--variant", default="product", help="a name for the library build that is measured (MVS_LIB_PATH)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sample_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_sample needs a GPU")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rate, copy_ms = copy_rate(dev, a)
    out = {"metric": "mesh_sample_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "variant": a.variant,
           "copy_bytes_per_s": rate, "copy_1gib_ms": [round(x, 4) for x in copy_ms], "results": []}
    torch.cuda.empty_cache()
    for name in a.rows.split(","):
        tv, tf = make_mesh(name, dev)
        for target in (int(t) for t in a.targets.split(",")):
            out["results"].append(run_row(name, tv, tf, target, rate, a))
            print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
        del tv, tf
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
