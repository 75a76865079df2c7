"""Times the Taubin smoothing (csrc/mesh_smooth.hip through mvsnet_amd.mesh_smooth) and prints one JSON line (also written to
--out, default profiles/mesh_smooth_bench.json).  Meshes: a surface-nets-like grid of quads over a noisy height field, two
triangles a quad, with 300 x 300 quads (180 000 faces) and 1000 x 1000 quads (2 M faces), in grid order as an extraction
numbers its vertices, and the large one also with the vertex numbers shuffled (every gather then misses its neighbours' lines).
Per row, with bench_tsdf.py's protocol (device events, median of --reps after --warmup, _min and _max kept): the adjacency build
(the three library calls with torch's sort and scan between them), one pass and ten Taubin iterations (twenty passes), both
with positions as rows of three floats and as rows padded to four, and the whole smooth_device call on device tensors as wall
time (it holds the read-back).  The yardstick is the same pass written in torch on the same device (index_add_ over the unique
directed edges in float64, which adds in no fixed order: the row gives its largest difference from the kernels' bytes) and
torch's build of its edge list (unique, bincount).

    python tools/bench_mesh_smooth.py [--reps 7] [--warmup 2] [--rows grid300,grid1000,grid1000_shuffled] [--no-torch] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_tsdf import time_events, time_wall  # noqa: E402

ROWS = ["grid300", "grid1000", "grid1000_shuffled"]
LAM, MU, ITERATIONS = 0.5, -0.53, 10


def make_mesh(name):
    """-> (vertices (M,3) float32, faces (F,3) int32): n x n quads with a voxel of 1 and noise of a third of a voxel."""
    n = int(name[4:].split("_")[0])
    rs = np.random.RandomState(0)
    y, x = np.meshgrid(np.arange(n + 1, dtype=np.float64), np.arange(n + 1, dtype=np.float64), indexing="ij")
    z = 20 * np.sin(x / 40) * np.cos(y / 55) + rs.randn(n + 1, n + 1) / 3
    v = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).astype(np.float32)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (j * (n + 1) + i).reshape(-1)
    f = np.stack([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)], 1).reshape(-1, 3)
    if name.endswith("_shuffled"):
        number = rs.permutation(len(v))
        v2 = np.empty_like(v)
        v2[number] = v
        v, f = v2, number[f]
    return v, f.astype(np.int32)


class Steps:
    """smooth_device call by call on tensors that stay allocated."""

    def __init__(self, tv, tf, dev):
        import torch
        from mvsnet_amd import _lib
        self.lib, self.L, self.torch = _lib.load(), _lib, torch
        self.tv, self.tf, self.M, self.F = tv, tf, int(tv.shape[0]), int(tf.shape[0])
        M, E = self.M, 6 * self.F
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        self.wsb = self.lib.mvs_mesh_smooth_workspace_bytes(M, self.F)
        self.ws = new(self.wsb, torch.uint8)
        self.keys, self.head, self.nb = new(E, torch.int64), new(E, torch.int32), new(E, torch.int32)
        self.rs, self.vc = new(M + 1, torch.int32), new(M, torch.uint8)
        self.x = {3: tv, 4: torch.cat([tv, torch.zeros((M, 1), dtype=torch.float32, device=dev)], 1).contiguous()}
        self.y = {row: [new((M, row), torch.float32) for _ in range(2)] for row in (3, 4)}

    def build(self):
        p, L, lib, torch = self.L.ptr, self.L, self.lib, self.torch
        L.check(lib.mvs_mesh_smooth_edges_i64(p(self.tv), self.M, p(self.tf), self.F, p(self.keys), p(self.ws), self.wsb, L.stream_ptr()), "edges")
        self.sk = torch.sort(self.keys)[0]
        L.check(lib.mvs_mesh_smooth_heads_i64(p(self.sk), self.F, p(self.head), p(self.ws), self.wsb, L.stream_ptr()), "heads")
        self.rank = torch.cumsum(self.head, 0, dtype=torch.int32)
        L.check(lib.mvs_mesh_smooth_rows_i32(p(self.sk), p(self.head), p(self.rank), self.M, self.F, 0, p(self.nb), p(self.rs), p(self.vc),
                                             p(self.ws), self.wsb, L.stream_ptr()), "rows")

    def sort_and_scan(self):
        self.torch.sort(self.keys)
        self.torch.cumsum(self.head, 0, dtype=self.torch.int32)

    def step(self, row, x, y, factor):
        p, L = self.L.ptr, self.L
        L.check(self.lib.mvs_mesh_smooth_step_f32(p(x), p(self.x[row]), p(self.rs), p(self.nb), p(self.vc), self.M, 6 * self.F, row, factor,
                                                  -1.0, p(y), L.stream_ptr()), "step")

    def one_pass(self, row):
        self.step(row, self.x[row], self.y[row][0], LAM)

    def iterations(self, row):
        x, k = self.x[row], 0
        for _ in range(ITERATIONS):
            for factor in (LAM, MU):
                y = self.y[row][k % 2]
                self.step(row, x, y, factor)
                x, k = y, k + 1
        return x


class TorchForm:
    """The same passes in torch: float64 sums by index_add_ over the unique directed edges, fixed vertices masked."""

    def __init__(self, tv, tf, vertex_class):
        self.tv, self.tf, self.moves = tv, tf, (vertex_class != 0)[:, None]
        self.build()

    def build(self):
        import torch
        f, M = self.tf.long(), self.tv.shape[0]
        s = torch.cat([f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2], f[:, 0]])
        t = torch.cat([f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 0], f[:, 2]])
        keys = torch.unique((s << 31) | t)
        self.src, self.dst = keys >> 31, keys & (2 ** 31 - 1)
        self.degree = torch.bincount(self.src, minlength=M).clamp(min=1).double()[:, None]

    def one_pass(self, x, factor=LAM):
        import torch
        xd = x.double()
        s = torch.zeros_like(xd).index_add_(0, self.src, xd[self.dst])
        y = (xd + float(np.float32(factor)) * (s / self.degree - xd)).float()
        return torch.where(self.moves, y, x)

    def iterations(self):
        x = self.tv
        for _ in range(ITERATIONS):
            x = self.one_pass(self.one_pass(x, LAM), MU)
        return x


def run_row(name, a):
    import torch
    from mvsnet_amd import mesh_smooth
    v, f = make_mesh(name)
    dev = torch.device("cuda", torch.cuda.current_device())
    tv, tf = torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev)
    row = {"row": name, "vertices": int(len(v)), "faces": int(len(f)), "iterations": ITERATIONS, "lam": LAM, "mu": MU}

    def put(key, t):
        row.update({key: round(t[0], 4), key + "_min": round(t[1], 4), key + "_max": round(t[2], 4)})

    out = mesh_smooth.smooth_device(tv, None, tf, dev, ITERATIONS, LAM, MU)
    row.update({k: out[3][k] for k in ("edges", "boundary_edges", "boundary_vertices", "fixed_vertices")})
    steps = Steps(tv, tf, dev)
    steps.build()
    put("build_ms", time_events(steps.build, a.reps, a.warmup))
    put("build_sort_and_scan_ms", time_events(steps.sort_and_scan, a.reps, a.warmup))
    for r in (3, 4):
        put("pass_rows%d_ms" % r, time_events(lambda: steps.one_pass(r), a.reps, a.warmup))
        put("iterations_rows%d_ms" % r, time_events(lambda: steps.iterations(r), a.reps, a.warmup))
    row["rows_same_bytes"] = bool(torch.equal(steps.iterations(3), steps.iterations(4)[:, :3]) and torch.equal(steps.iterations(3), out[0]))
    put("smooth_device_ms", time_wall(lambda: mesh_smooth.smooth_device(tv, None, tf, dev, ITERATIONS, LAM, MU), a.reps, a.warmup))
    if a.torch:
        form = TorchForm(tv, tf, steps.vc)
        row["torch_max_abs_difference"] = float((form.iterations() - out[0]).abs().max())
        put("torch_build_ms", time_events(form.build, a.reps, a.warmup))
        put("torch_pass_ms", time_events(lambda: form.one_pass(tv), a.reps, a.warmup))
        put("torch_iterations_ms", time_events(form.iterations, a.reps, a.warmup))
        del form
    del steps, tv, tf, out
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--no-torch", dest="torch", action="store_false", help="leave the torch yardstick out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_smooth needs a GPU")
    torch.cuda.set_device(0)
    out = {"metric": "mesh_smooth_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "results": []}
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
