"""Point-to-point ICP registration of a source cloud to a target cloud on the MI355X: the refinement step of the
Tanks-and-Temples evaluation protocol, between the crop / downsampling and the distances of mvsnet_amd.evaluate.

    python -m mvsnet_amd.register --source P.ply --target G.ply --stages 4:8:30,2:4:30,0:2:30 [--init T.txt] [--with_scale]
        [--crop x0,y0,z0,x1,y1,z1] --out T.txt [--report R.json]

One registration step is one fused HIP pass (csrc/pointcloud.hip, mvs_icp_step_f32) over the target's grid, which is built
once (mvs_nn_target_build_f32); torch owns the device memory, the stable sort behind the processing order and the voxel
downsampling's key sort; the 3x3 solve is float64 numpy on the host.

Semantics (shared by the kernels, tests/registration_reference.py and the tests).  S is the source, G the target, each (n,3)
float32; T a 4x4 float64 matrix with last row 0 0 0 1 that maps S onto G.
  * One step at T.  For every source point p: p' = T p per coordinate T[i,0] x + T[i,1] y + T[i,2] z + T[i,3], left to right
    in float64 (no fused multiply-add), rounded to float32 once (evaluate._transform).  Its correspondence q is the nearest
    target point of p' under evaluate's rule: float32 d^2 from float32 differences, kept when d^2 <= max_corr_dist^2, exact
    ties to the smallest target index.  Over the points that have one, in float64, with a = p - cp (the UNtransformed
    source), b = q - cq and r = T p - q (T p unrounded):
        moments = [count, sum |r|^2, sum a (3), sum b (3), sum a b^T (9, row-major), sum |a|^2]
    cp and cq are the float64 means of the whole source and target, fixed for a plan: they only centre the sums.
    Because a is taken from p and not from p', the solve yields the absolute transform: no increment is composed.
  * Solve (solve_from_moments).  n = count, H = sum a b^T - (sum a)(sum b)^T / n = U diag(S) V^T, D = diag(1, 1, det(V U^T)),
    R = V D U^T, s = tr(diag(S) D) / (sum |a|^2 - |sum a|^2 / n) with_scale, else 1, t = (cq + sum b / n) - s R (cp + sum a / n).
    n < 3 is "too_few_correspondences"; S[1] <= 1e-12 S[0], or with_scale a source variance that is not positive, is
    "degenerate".
  * Loop (RegistrationPlan.run).  From T = init (identity by default), at most max_iterations times: step at T;
    fitness = count / |S|, inlier_rmse = sqrt(sum |r|^2 / count); stop as "converged" when this is not the first step and
    |fitness - previous| < fitness_tol and |inlier_rmse - previous| < rmse_tol * max_corr_dist; else solve, stop as
    "too_few_correspondences" / "degenerate" when the solve says so, else T = the solution.  Otherwise "max_iterations".
    The returned transform is the one the last step was taken at, so fitness and inlier_rmse describe it; after
    too_few_correspondences or degenerate it is the last good transform (init when the first step fails).
  * Stages (register_point_clouds).  stages = [(voxel, max_corr_dist, max_iterations), ...], coarse to fine.  crop, the
    evaluation's inclusive box, first restricts the target to the box and the source to the points whose init p falls inside
    it.  Each stage voxel-downsamples both clouds (evaluate's rule, 0 = off) and runs the loop from the previous stage's
    transform.  A stage that stops on too_few_correspondences or degenerate ends the list.
  * Sums are float64, reduced in a fixed order, no float atomics: the same inputs give bit-identical moments and transforms
    on every run.  The processing order of the source (points sorted by the target cell of init p, a stable sort) only
    changes the order of the sums, never a correspondence.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
import sys

import numpy as np

from .evaluate import check_crop, check_transform

MOMENTS = 18
STOP_FAILED = ("too_few_correspondences", "degenerate")


# ------------------------------------------------------------------------------------------------ host side, no GPU needed

def solve_from_moments(moments, cp, cq, with_scale=False):
    """Kabsch / Umeyama from the 18 moments -> (T, None), T 4x4 float64 with last row exactly 0 0 0 1, or (None, reason),
    reason "too_few_correspondences" or "degenerate" (module docstring)."""
    m = np.asarray(moments, np.float64).reshape(-1)
    if m.shape != (MOMENTS,):
        raise ValueError("moments must hold %d numbers, got %s" % (MOMENTS, m.shape))
    cp, cq = np.asarray(cp, np.float64).reshape(3), np.asarray(cq, np.float64).reshape(3)
    n = m[0]
    if not n >= 3:
        return None, "too_few_correspondences"
    sa, sb = m[2:5], m[5:8]
    H = m[8:17].reshape(3, 3) - np.outer(sa, sb) / n
    var = m[17] - float(sa @ sa) / n
    if not np.isfinite(H).all():
        return None, "degenerate"
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > 1e-12 * S[0] or (with_scale and not var > 0):
        return None, "degenerate"
    D = np.array([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    R = (Vt.T * D) @ U.T
    s = float((S * D).sum()) / var if with_scale else 1.0
    T = np.zeros((4, 4))
    T[:3, :3] = s * R
    T[:3, 3] = (cq + sb / n) - s * (R @ (cp + sa / n))
    T[3, 3] = 1.0
    return T, None


def parse_stages(text):
    """"4:8:30,2:4:30,0:2:30" -> [(4.0, 8.0, 30), (2.0, 4.0, 30), (0.0, 2.0, 30)] (voxel:max_corr_dist:max_iterations)."""
    stages = []
    for part in str(text).split(","):
        if not part.strip():
            continue
        tok = part.split(":")
        if len(tok) != 3:
            raise ValueError("stage %r: voxel:max_corr_dist:max_iterations expected" % part)
        try:
            stages.append((float(tok[0]), float(tok[1]), int(tok[2])))
        except ValueError:
            raise ValueError("stage %r: voxel:max_corr_dist:max_iterations expected" % part)
    return check_stages(stages)


def check_stages(stages):
    out = []
    for st in stages:
        if len(st) != 3:
            raise ValueError("a stage is (voxel, max_corr_dist, max_iterations), got %r" % (st,))
        voxel, dist, iters = float(st[0]), float(st[1]), st[2]
        if not (voxel >= 0 and math.isfinite(voxel)):
            raise ValueError("stage voxel must be >= 0, got %r" % (st[0],))
        if not (dist > 0 and math.isfinite(dist)):
            raise ValueError("stage max_corr_dist must be positive and finite, got %r" % (st[1],))
        if int(iters) != iters or int(iters) < 1:
            raise ValueError("stage max_iterations must be a positive integer, got %r" % (st[2],))
        out.append((voxel, dist, int(iters)))
    if not out:
        raise ValueError("at least one stage is needed")
    return out


def write_transform(path, T):
    """4 lines of 4 numbers in repr precision: np.loadtxt (evaluate --transform) reads back the same float64 bits."""
    T = check_transform(T)
    with open(path, "w") as f:
        for row in T:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def read_transform(path):
    return check_transform(np.loadtxt(path, dtype=np.float64).reshape(4, 4))


def _check_options(max_corr_dist, max_iterations, fitness_tol, rmse_tol):
    d = float(max_corr_dist)
    if not (d > 0 and math.isfinite(d) and math.isfinite(float(np.float32(d)) ** 2)):
        raise ValueError("max_corr_dist must be positive and finite, got %r" % (max_corr_dist,))
    if int(max_iterations) != max_iterations or int(max_iterations) < 1:
        raise ValueError("max_iterations must be a positive integer, got %r" % (max_iterations,))
    for name, v in (("fitness_tol", fitness_tol), ("rmse_tol", rmse_tol)):
        if not (float(v) >= 0 and math.isfinite(float(v))):
            raise ValueError("%s must be >= 0, got %r" % (name, v))
    return d, int(max_iterations), float(fitness_tol), float(rmse_tol)


# ------------------------------------------------------------------------------------------------ device side

class RegistrationPlan:
    """ICP of `source` onto `target` (numpy arrays or device float32 (n,3) tensors) at one correspondence distance.  The
    constructor uploads, picks the target's grid, builds it once, computes the processing order and the two centres (it
    synchronises); ``step(T)`` launches one fused step on torch's current stream and returns the device tensor of the 18
    moments; ``run()`` iterates step, one 144-byte copy to the host, solve -> the result dict of the module docstring."""

    def __init__(self, source, target, *, max_corr_dist, init=None, with_scale=False, max_iterations=50, fitness_tol=1e-6,
                 rmse_tol=1e-6, cell=None, device=None):
        import torch
        from . import _lib
        from . import evaluate as E
        self.max_corr_dist, self.max_iterations, self.fitness_tol, self.rmse_tol = _check_options(
            max_corr_dist, max_iterations, fitness_tol, rmse_tol)
        self.init = check_transform(init) if init is not None else np.eye(4)
        self.with_scale = bool(with_scale)
        self.dev = _lib.device(device, "point-cloud evaluation")
        with torch.cuda.device(self.dev):
            self.source, self.target = E._points(source, "source", self.dev), E._points(target, "target", self.dev)
            ns, nt = self.source.shape[0], self.target.shape[0]
            if ns == 0 or nt == 0:
                raise ValueError("registration needs non-empty clouds")
            self.grid = g = E.choose_grid(self.target, self.max_corr_dist, cell)
            lib = _lib.load()
            wsb = lib.mvs_nn_target_workspace_bytes(nt, *g["dims"])
            if wsb == 0:
                raise ValueError("registration: grid %s not supported" % (g["dims"],))
            self.target_ws = torch.empty(wsb, dtype=torch.uint8, device=self.dev)
            _lib.check(lib.mvs_nn_target_build_f32(_lib.ptr(self.target), nt, *g["origin"], g["cell"], *g["dims"],
                                                   _lib.ptr(self.target_ws), wsb, _lib.stream_ptr()), "mvs_nn_target_build_f32")
            self.step_ws = torch.empty(lib.mvs_icp_step_workspace_bytes(ns), dtype=torch.uint8, device=self.dev)
            self.moments = torch.zeros(MOMENTS, dtype=torch.float64, device=self.dev)
            self._host = torch.empty(MOMENTS, dtype=torch.float64, pin_memory=True)
            self.order = self._processing_order()
            self.cp = self.source.double().mean(0).cpu().numpy()
            self.cq = self.target.double().mean(0).cpu().numpy()
        self._cp = (ctypes.c_double * 3)(*self.cp)
        self._cq = (ctypes.c_double * 3)(*self.cq)

    def _processing_order(self):
        """Source indices sorted (stable) by the target cell of fl32(init p): the lanes of a wave then share cells."""
        import torch
        from . import evaluate as E
        g = self.grid
        p = E._transform(self.source, self.init)
        o = p.new_tensor(g["origin"])
        dims = torch.tensor(g["dims"], dtype=torch.float32, device=self.dev)
        c = torch.minimum(torch.clamp(torch.floor((p - o) / g["cell"]), min=0.0), dims - 1).long()
        cellid = (c[:, 2] * g["dims"][1] + c[:, 1]) * g["dims"][0] + c[:, 0]
        return torch.sort(cellid, stable=True)[1].int().contiguous()

    def step(self, T, *, order="plan", dist=None, index=None):
        """One step at T (4x4) -> self.moments (device, 18 float64), enqueued on torch's current stream.  order: "plan" (the
        plan's processing order), None (input order) or an int32 device tensor; dist / index: optional (n_source) float32 /
        int32 device tensors that receive the correspondences in input order."""
        import torch
        from . import _lib
        T = check_transform(T)
        order = self.order if isinstance(order, str) and order == "plan" else order
        n = self.source.shape[0]
        if order is not None and (order.dtype != torch.int32 or order.numel() != n):
            raise ValueError("order must be an int32 tensor of %d entries" % n)
        if dist is not None and (dist.dtype != torch.float32 or dist.numel() != n):
            raise ValueError("dist must be a float32 tensor of %d entries" % n)
        if index is not None and (index.dtype != torch.int32 or index.numel() != n):
            raise ValueError("index must be an int32 tensor of %d entries" % n)
        g = self.grid
        T34 = (ctypes.c_double * 12)(*T[:3].reshape(-1))
        with torch.cuda.device(self.dev):
            rc = _lib.load().mvs_icp_step_f32(
                _lib.ptr(self.source), n, _lib.ptr(order), T34, self._cp, self._cq, *g["origin"], g["cell"], *g["dims"],
                self.target.shape[0], _lib.ptr(self.target_ws), self.target_ws.numel(), self.max_corr_dist,
                _lib.ptr(self.moments), _lib.ptr(dist), _lib.ptr(index), _lib.ptr(self.step_ws), self.step_ws.numel(),
                _lib.stream_ptr())
        _lib.check(rc, "mvs_icp_step_f32")
        return self.moments

    def step_host(self, T, **kw):
        """step(T) and the one small copy -> (18,) float64 numpy."""
        import torch
        self.step(T, **kw)
        with torch.cuda.device(self.dev):
            self._host.copy_(self.moments, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        return self._host.numpy().copy()

    def run(self):
        T = self.init.copy()
        history, prev, stopped, it = [], None, "max_iterations", 0
        fitness, rmse = 0.0, None
        n = self.source.shape[0]
        while it < self.max_iterations:
            m = self.step_host(T)
            it += 1
            fitness = float(m[0]) / n
            rmse = math.sqrt(float(m[1]) / float(m[0])) if m[0] > 0 else None
            history.append([fitness, rmse])
            if prev is not None and rmse is not None and prev[1] is not None and abs(fitness - prev[0]) < self.fitness_tol \
                    and abs(rmse - prev[1]) < self.rmse_tol * self.max_corr_dist:
                stopped = "converged"
                break
            new, why = solve_from_moments(m, self.cp, self.cq, self.with_scale)
            if new is None:
                stopped = why
                break
            prev, T = (fitness, rmse), new
        return {"transform": T.tolist(), "fitness": fitness, "inlier_rmse": rmse, "iterations": it, "stopped": stopped,
                "history": history}


def register_point_clouds(source, target, *, stages, init=None, with_scale=False, crop=None, fitness_tol=1e-6, rmse_tol=1e-6,
                          device=None):
    """Multi-stage ICP (module docstring) -> {"transform": 4x4 list, "stopped": the last stage's reason, "stages": [each
    stage's RegistrationPlan.run() result plus "voxel", "max_corr_dist", "source_points", "target_points"]}."""
    import torch
    from . import _lib
    from . import evaluate as E
    stages = check_stages(stages)
    T = check_transform(init) if init is not None else np.eye(4)
    box = check_crop(crop) if crop is not None else None
    dev = _lib.device(device, "point-cloud evaluation")
    with torch.cuda.device(dev):
        src, tgt = E._points(source, "source", dev), E._points(target, "target", dev)
        if box is not None:
            tgt = E._crop(tgt, *box)
            moved = E._transform(src, T).double()
            src = src[((moved >= moved.new_tensor(box[0])) & (moved <= moved.new_tensor(box[1]))).all(1)].contiguous()
        for name, t in (("source", src), ("target", tgt)):
            if t.shape[0] == 0:
                raise ValueError("the %s cloud is empty after the crop" % name)
        results = []
        for voxel, dist, iters in stages:
            s = E._voxel(src, voxel, "source") if voxel else src
            t = E._voxel(tgt, voxel, "target") if voxel else tgt
            r = RegistrationPlan(s, t, max_corr_dist=dist, init=T, with_scale=with_scale, max_iterations=iters,
                                 fitness_tol=fitness_tol, rmse_tol=rmse_tol, device=dev).run()
            r.update({"voxel": voxel, "max_corr_dist": dist, "source_points": int(s.shape[0]), "target_points": int(t.shape[0])})
            results.append(r)
            T = check_transform(r["transform"])
            if r["stopped"] in STOP_FAILED:
                break
    return {"transform": T.tolist(), "stopped": results[-1]["stopped"], "stages": results}


# ------------------------------------------------------------------------------------------------ command line

def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", required=True, help="cloud to move (PLY)")
    ap.add_argument("--target", required=True, help="cloud to register to (PLY)")
    ap.add_argument("--stages", required=True, help="voxel:max_corr_dist:max_iterations[,...], coarse to fine; voxel 0 = off")
    ap.add_argument("--init", default=None, help="text file with the 4x4 start transform (identity without it)")
    ap.add_argument("--with_scale", action="store_true", help="solve for a similarity (uniform scale) instead of a rigid motion")
    ap.add_argument("--crop", default=None, help="x0,y0,z0,x1,y1,z1 (inclusive box: the target, and the source after --init)")
    ap.add_argument("--out", required=True, help="the 4x4 transform, readable by mvsnet_amd.evaluate --transform")
    ap.add_argument("--report", default=None, help="also write the JSON report to this file")
    a = ap.parse_args(argv)
    from .evaluate import _floats, read_ply_points
    try:
        stages = parse_stages(a.stages)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.register: %s" % e)
    from ._lib import gpu_ready
    why = gpu_ready()
    if why is not None:
        raise SystemExit("mvsnet_amd.register needs a GPU and the HIP library: %s" % why)
    crop = _floats(a.crop, 6, "--crop") if a.crop else None
    src, _ = read_ply_points(a.source)
    tgt, _ = read_ply_points(a.target)
    try:
        init = read_transform(a.init) if a.init else None
        report = register_point_clouds(src, tgt, stages=stages, init=init, with_scale=a.with_scale, crop=crop)
    except ValueError as e:
        raise SystemExit("mvsnet_amd.register: %s" % e)
    write_transform(a.out, report["transform"])
    line = json.dumps(report)
    print(line)
    if a.report:
        with open(a.report, "w") as f:
            f.write(line + "\n")
    return 1 if report["stopped"] in STOP_FAILED else 0


if __name__ == "__main__":
    sys.exit(main())
