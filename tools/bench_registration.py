"""Times the ICP registration (mvs_icp_step_f32 through mvsnet_amd.register) on bench_pointcloud_eval's seeded dtu_like
clouds and prints one JSON line:

  step_ms           one fused registration step over the target grid built once (device events, median of --reps after
                    --warmup), at the start transform (identity, the source displaced) and at the aligned transform
  baseline_step_ms  the same eighteen moments from what the library offered before the fused step, in the same process:
                    torch transform of the source, NearestPlan (target grid rebuilt, queries sorted, dist / index written),
                    torch gathers and float64 sums
  build_ms          the target grid alone (mvs_nn_target_build_f32), paid once per plan
  run               a three-stage register_point_clouds (host wall time: it includes the uploads, the downsampling, the
                    grid choice and one small copy per iteration) with each stage's iterations, and the error of the result

The source is the prediction displaced by the inverse of a 1 degree rotation about (1,2,3) plus a (2, -1.5, 1) mm shift.

    python tools/bench_registration.py [--reps 10] [--warmup 2] [--stages 4:8:30,2:4:30,0:2:30] [--n_gt N --n_pred N]
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


def displacement():
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    t = np.deg2rad(1.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    T[:3, 3] = [2.0, -1.5, 1.0]
    return T


def baseline(E, src, tgt, max_dist, cp, cq):
    """-> fn(T) that leaves the 18 moments in a device tensor, built from NearestPlan and torch alone."""
    import torch
    nn = E.NearestPlan(src.clone(), tgt, max_dist)       # its own query buffer: a plan keeps device tensors as they are
    cp_t, cq_t = torch.as_tensor(cp, device=src.device), torch.as_tensor(cq, device=src.device)
    out = {}

    def fn(T):
        p = src.double()
        moved = torch.stack([((p[:, 0] * T[i, 0] + p[:, 1] * T[i, 1]) + p[:, 2] * T[i, 2]) + T[i, 3] for i in range(3)], 1)
        nn.query.copy_(moved.float())
        nn._enqueue()
        w = (nn.index >= 0).double()
        q = tgt[nn.index.clamp(min=0).long()].double()
        a, b, r = p - cp_t, q - cq_t, moved - q
        out["moments"] = torch.cat([w.sum()[None], ((r * r).sum(1) * w).sum()[None], (a * w[:, None]).sum(0), (b * w[:, None]).sum(0),
                                    ((a * w[:, None])[:, :, None] * b[:, None, :]).sum(0).reshape(9), ((a * a).sum(1) * w).sum()[None]])
        return out["moments"]
    return fn


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stages", default="4:8:30,2:4:30,0:2:30")
    ap.add_argument("--max_corr_dist", type=float, default=2.0, help="correspondence distance of the timed single step")
    ap.add_argument("--n_gt", type=int, default=CONFIGS["dtu_like"]["n_gt"])
    ap.add_argument("--n_pred", type=int, default=CONFIGS["dtu_like"]["n_pred"])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_registration needs a GPU")
    torch.cuda.set_device(0)
    from mvsnet_amd import _lib
    from mvsnet_amd import evaluate as E
    from mvsnet_amd import register as Rg
    pred, gt = clouds(a.n_gt, a.n_pred)
    T0 = displacement()
    dev = torch.device("cuda", 0)
    src = E._transform(torch.as_tensor(pred).to(dev), np.linalg.inv(T0))
    tgt = torch.as_tensor(gt).to(dev)
    out = {"metric": "registration_ms", "device": torch.cuda.get_device_name(0), "reps": a.reps, "source_points": len(pred),
           "target_points": len(gt), "max_corr_dist": a.max_corr_dist}

    plan = Rg.RegistrationPlan(src, tgt, max_corr_dist=a.max_corr_dist)
    g, lib = plan.grid, _lib.load()
    out["grid"] = g
    out["build_ms"] = round(device_ms(lambda: _lib.check(lib.mvs_nn_target_build_f32(
        _lib.ptr(plan.target), plan.target.shape[0], *g["origin"], g["cell"], *g["dims"], _lib.ptr(plan.target_ws),
        plan.target_ws.numel(), _lib.stream_ptr()), "mvs_nn_target_build_f32"), a.reps, a.warmup)[0], 3)
    base = baseline(E, src, tgt, a.max_corr_dist, plan.cp, plan.cq)
    for name, T in (("start", np.eye(4)), ("aligned", T0)):
        med, lo, hi = device_ms(lambda: plan.step(T), a.reps, a.warmup)
        med_in, _, _ = device_ms(lambda: plan.step(T, order=None), a.reps, a.warmup)
        bmed, blo, bhi = device_ms(lambda: base(T), a.reps, a.warmup)
        fused, ref = plan.step(T).cpu().numpy(), base(T).cpu().numpy()
        out[name] = {"step_ms": round(med, 3), "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3),
                     "step_input_order_ms": round(med_in, 3), "baseline_step_ms": round(bmed, 3),
                     "baseline_step_ms_min": round(blo, 3), "baseline_step_ms_max": round(bhi, 3),
                     "speedup": round(bmed / med, 2), "fitness": float(fused[0]) / len(pred),
                     "moments_max_rel_diff": float(np.max(np.abs(fused - ref) / np.maximum(np.abs(ref), 1e-300)))}
    del plan, base
    torch.cuda.empty_cache()

    stages = Rg.parse_stages(a.stages)
    torch.cuda.synchronize()
    t = time.perf_counter()
    rep = Rg.register_point_clouds(src, tgt, stages=stages)
    torch.cuda.synchronize()
    E_ = np.array(rep["transform"]) @ np.linalg.inv(T0)
    K = (E_[:3, :3] - E_[:3, :3].T) / 2
    out["run"] = {"stages": a.stages, "wall_ms": round((time.perf_counter() - t) * 1e3, 1), "stopped": rep["stopped"],
                  "iterations": [s["iterations"] for s in rep["stages"]],
                  "points": [[s["source_points"], s["target_points"]] for s in rep["stages"]],
                  "fitness": rep["stages"][-1]["fitness"], "inlier_rmse": rep["stages"][-1]["inlier_rmse"],
                  "rotation_error_rad": float(np.sqrt(K[2, 1] ** 2 + K[0, 2] ** 2 + K[1, 0] ** 2)),
                  "translation_error": float(np.linalg.norm(E_[:3, 3]))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
