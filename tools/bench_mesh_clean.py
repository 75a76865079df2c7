"""Times the mesh cleaning (csrc/mesh_components.hip through mvsnet_amd.mesh_clean) and prints one JSON line (also written to
--out, default profiles/mesh_clean_bench.json).  Meshes: bench_tsdf.py's own extractions at 256 and 512 nodes (144 views of
160 x 128), bench_raster.py's bumpy sphere at about 2 M and 5 M faces in input order and with the face order shuffled, and
2 M faces split into 100 000 components (strips of 20 triangles).  Per mesh, with bench_tsdf.py's protocol (device events,
median of --reps after --warmup, _min and _max kept): labelling (mvs_mesh_components_label_i32), measures
(mvs_mesh_components_measure_f32) and compaction (mark, torch's two scans, write, with the sizes known) on their own, and the
whole clean_mesh call on device tensors with min_faces = 8 as wall time (it holds the table's nonzero and the read-back).
Beside them: scipy's connected_components on the host for the same mesh, and the extraction time of the same mesh from
profiles/tsdf_bench.json where that file has the row.

    python tools/bench_mesh_clean.py [--reps 5] [--warmup 1] [--meshes tsdf256,tsdf512,sphere2m,...] [--no-scipy] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import bench_raster  # noqa: E402
import bench_tsdf  # noqa: E402
from bench_tsdf import time_events, time_wall  # noqa: E402

TSDF_CONFIG = 1                                   # 144 views of 160 x 128
MESHES = ["tsdf256", "tsdf512", "sphere2m", "sphere2m_shuffled", "sphere5m", "sphere5m_shuffled", "pieces2m"]


def pieces(n_components=100000, faces_each=20):
    """n_components strips of faces_each triangles, each on its own vertices, laid out on a square lattice."""
    i = np.arange(faces_each)
    strip = np.stack([i, i + 1, i + 2], 1)
    per = faces_each + 2
    faces = (strip[None] + per * np.arange(n_components)[:, None, None]).reshape(-1, 3).astype(np.int32)
    side = int(np.ceil(np.sqrt(n_components)))
    k = np.arange(n_components)
    base = np.stack([(k % side) * 20.0, (k // side) * 4.0, np.zeros(n_components)], 1)
    local = np.stack([np.arange(per) * 0.5, np.arange(per) % 2, np.zeros(per)], 1)
    return (base[:, None] + local[None]).reshape(-1, 3).astype(np.float32), faces


def make_mesh(name):
    """-> (vertices, faces, extra row fields) as numpy."""
    if name.startswith("tsdf"):
        from mvsnet_amd import mesh
        resolution = int(name[4:])
        V, H, W = bench_tsdf.CONFIGS[TSDF_CONFIG]
        s = bench_tsdf.scene(V, H, W)
        origin, voxel, dims = mesh.choose_volume(bench_tsdf.BOX[0], bench_tsdf.BOX[1], resolution=resolution)
        vol = mesh.TsdfVolume(origin, voxel, dims, bench_tsdf.TRUNC_VOXELS * voxel)
        vol.integrate(s["depths"], s["probs"], s["cams"])
        v, _, f = vol.extract()
        return v, f, {"views": V, "H": H, "W": W, "resolution": resolution}
    if name.startswith("sphere"):
        n = int(name[6]) * 1000000
        v, f = bench_raster.bumpy_sphere(n)
        if name.endswith("_shuffled"):
            f = f[np.random.RandomState(0).permutation(len(f))]
        return v, f, {}
    if name == "pieces2m":
        v, f = pieces()
        return v, f, {}
    raise SystemExit("unknown mesh %r (known: %s)" % (name, ", ".join(MESHES)))


def tsdf_extract_ms(path, extra):
    """The extraction time of the same mesh from bench_tsdf.py's file, or None."""
    try:
        rows = json.load(open(path))["results"]
    except (OSError, ValueError, KeyError):
        return None
    for r in rows:
        if all(r.get(k) == extra.get(k) for k in ("views", "H", "W", "resolution")) and "extract_ms" in r:
            return r["extract_ms"]
    return None


def scipy_ms(vertices, faces):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = time.perf_counter()
    ok = ((faces >= 0) & (faces < len(vertices))).all(1)
    g = faces[ok].astype(np.int64)
    a, b = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    n, _ = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(len(vertices),) * 2), directed=False)
    return (time.perf_counter() - t) * 1e3, int(n)


def run_mesh(name, a):
    import torch
    from mvsnet_amd import _lib, mesh_clean
    v, f, extra = make_mesh(name)
    dev = torch.device("cuda", torch.cuda.current_device())
    tv, tf = torch.as_tensor(v).to(dev), torch.as_tensor(f).to(dev)
    lib = _lib.load()
    row = dict({"mesh": name, "vertices": int(len(v)), "faces": int(len(f))}, **extra)
    comp = mesh_clean._Components(tv, tf, dev)

    def put(key, t):
        row.update({key: round(t[0], 4), key + "_min": round(t[1], 4), key + "_max": round(t[2], 4)})

    put("label_ms", time_events(comp.label, a.reps, a.warmup))
    put("measure_ms", time_events(comp.measure, a.reps, a.warmup))
    out = mesh_clean.clean_device(tv, None, tf, dev, min_faces=8)
    rep = out[3]
    row.update({k: rep[k] for k in ("components", "components_kept", "faces_out", "vertices_out", "unreferenced", "error_word")})
    M, F, M_out, F_out = len(v), len(f), rep["vertices_out"], rep["faces_out"]
    keep_label = (comp.counts >= 8).to(torch.int32)
    face_keep, vertex_keep = torch.empty(F, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    out_v, out_f = torch.empty((M_out, 3), device=dev), torch.empty((F_out, 3), dtype=torch.int32, device=dev)

    def compact():
        _lib.check(lib.mvs_mesh_compact_mark_i32(_lib.ptr(tf), M, F, _lib.ptr(comp.face_labels), _lib.ptr(keep_label),
                                                 _lib.ptr(face_keep), _lib.ptr(vertex_keep), _lib.stream_ptr()), "mark")
        fr, vr = torch.cumsum(face_keep, 0, dtype=torch.int32), torch.cumsum(vertex_keep, 0, dtype=torch.int32)
        _lib.check(lib.mvs_mesh_compact_write_f32(_lib.ptr(tv), None, M, _lib.ptr(tf), F, _lib.ptr(face_keep), _lib.ptr(fr),
                                                  _lib.ptr(vertex_keep), _lib.ptr(vr), M_out, F_out, _lib.ptr(out_v), None,
                                                  _lib.ptr(out_f), _lib.stream_ptr()), "write")

    put("compact_ms", time_events(compact, a.reps, a.warmup))
    assert out_v.cpu().numpy().tobytes() == out[0].cpu().numpy().tobytes() and torch.equal(out_f, out[2])
    put("clean_mesh_ms", time_wall(lambda: mesh_clean.clean_device(tv, None, tf, dev, min_faces=8), a.reps, a.warmup))
    if a.scipy:
        row["scipy_components_ms"], n = scipy_ms(v, f)
        row["scipy_components"] = n - rep["unreferenced"]                      # scipy counts isolated vertices as components
    if extra:
        row["tsdf_extract_ms"] = tsdf_extract_ms(a.tsdf_bench, extra)
    del comp, tv, tf, out
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--meshes", default=",".join(MESHES))
    ap.add_argument("--no-scipy", dest="scipy", action="store_false", help="leave the host yardstick out")
    ap.add_argument("--tsdf_bench", default=os.path.join(ROOT, "profiles", "tsdf_bench.json"))
    ap.add_argument("--variant", default="product", help="a name for the library build that is measured (MVS_LIB_PATH)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean needs a GPU")
    torch.cuda.set_device(0)
    out = {"metric": "mesh_clean_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "variant": a.variant, "results": []}
    for name in a.meshes.split(","):
        out["results"].append(run_mesh(name, a))
        print(json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
