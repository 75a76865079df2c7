"""Times the depth-map fusion (csrc/fusion.hip through mvsnet_amd.fusion) on analytic sphere-and-plane scenes and prints one
JSON line: milliseconds per fusion (device events around FusionPlan.enqueue, median of --reps after --warmup) with and
without de-duplication, for 48 and 144 views at 160 x 128 and 135 views at 288 x 216 (configuration 4's share per rank), and
the float64 numpy reference (tests/fusion_reference.py) at 48 views for scale.  With --normals every size also gets the
normal-map kernel alone (mvs_depth_normals_f32: "normal_map_ms") and the fusion with normals ("ms_normals", threshold off; it
contains the normal-map launch), next to the plain fusion ("ms").  --repeat R measures everything R times over (R result
rows per case, "repeat" 0..R-1): the spread between the rows is what a difference between two builds has to exceed.

    python tools/bench_fusion.py [--reps 10] [--warmup 2] [--no-reference] [--normals] [--repeat 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import fusion_reference as FR  # noqa: E402

CONFIGS = [(48, 128, 160), (144, 128, 160), (135, 216, 288)]


def scene(V, H, W):
    # cameras spread over about 70 degrees of arc whatever V is; focal length scales with the width
    return FR.make_scene("sphere", V=V, H=H, W=W, f=0.8 * W, arc_step_deg=70.0 / V, low_prob_fraction=0.05, seed=11)


def time_calls(call, reps, warmup):
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


def time_device(s, dedupe, reps, warmup, normals=False):
    from mvsnet_amd import fusion as F
    plan = F.FusionPlan(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=3, dedupe=dedupe, normals=normals)
    med, lo, hi = time_calls(plan.enqueue, reps, warmup)
    return med, lo, hi, int(plan.count.item())


def time_normal_map(s, reps, warmup):
    """mvs_depth_normals_f32 alone on device-resident maps (what estimate_normals launches)."""
    import torch
    from mvsnet_amd import _lib, fusion as F
    d, p = torch.as_tensor(s["depths"]).cuda(), torch.as_tensor(s["probs"]).cuda()
    tables = torch.as_tensor(F.camera_tables(s["cams"])).cuda()
    V, H, W = d.shape
    out = torch.empty((V, H, W, 3), dtype=torch.float32, device=d.device)
    lib = _lib.load()

    def call():
        _lib.check(lib.mvs_depth_normals_f32(_lib.ptr(d), _lib.ptr(p), V, H, W, _lib.ptr(tables), 0.8, 0.05, _lib.ptr(out),
                                             _lib.stream_ptr()), "mvs_depth_normals_f32")
    return time_calls(call, reps, warmup)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy reference (profiling runs)")
    ap.add_argument("--normals", action="store_true", help="also time the normal-map kernel alone and the fusion with normals")
    ap.add_argument("--repeat", type=int, default=1, help="measure everything this many times over")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion needs a GPU")
    torch.cuda.set_device(0)
    out = {"metric": "fusion_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "num_consistent": 3, "results": []}
    for V, H, W in CONFIGS:
        s = scene(V, H, W)
        for k in range(a.repeat):
            if a.normals:
                med, lo, hi = time_normal_map(s, a.reps, a.warmup)
                out["results"].append({"views": V, "H": H, "W": W, "repeat": k, "normal_map_ms": round(med, 4),
                                       "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                                       "ns_per_pixel": round(med * 1e6 / (V * H * W), 5)})
            for dedupe in (True, False):
                med, lo, hi, pts = time_device(s, dedupe, a.reps, a.warmup)
                pairs = V * (V - 1) * H * W
                row = {"views": V, "H": H, "W": W, "dedupe": dedupe, "repeat": k, "ms": round(med, 4), "ms_min": round(lo, 4),
                       "ms_max": round(hi, 4), "points": pts, "pairs": pairs, "ns_per_pair": round(med * 1e6 / pairs, 5)}
                if a.normals:
                    med, lo, hi, npts = time_device(s, dedupe, a.reps, a.warmup, normals=True)
                    row.update({"ms_normals": round(med, 4), "ms_normals_min": round(lo, 4), "ms_normals_max": round(hi, 4),
                                "points_normals": npts})
                out["results"].append(row)
    if not a.no_reference:
        s = scene(48, 128, 160)
        for dedupe in (True, False):
            t = time.perf_counter()
            ref = FR.reference_fusion(s["depths"], s["probs"], s["cams"], s["images"], num_consistent=3, dedupe=dedupe)
            out["results"].append({"views": 48, "H": 128, "W": 160, "dedupe": dedupe, "numpy_reference_ms":
                                   round((time.perf_counter() - t) * 1e3, 1), "points": int(len(ref["xyz"]))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
