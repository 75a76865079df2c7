"""Float64 numpy restatement of the depth-map fusion of mvsnet_amd/fusion.py (the semantics in its docstring), plus the
analytic scenes the tests and tools/bench_fusion.py run it on.  Views are processed one after the other and sources in
ascending order, as the statement says; within one view the pixels are independent (the marks of view r land only in other
views), so they are evaluated as numpy vectors.

For every pixel the reference also reports its MARGIN: the smallest distance of any quantity it decided on to the boundary of
that decision -- relative distance of prob to prob_threshold, of w and w' to 0 (over d), of the reprojection error to
reproj_threshold and of the relative depth error to depth_rel_threshold (of both when the pair is consistent, else of the
criteria that fail), and the distance in pixels of u/w + 1/2 and v/w + 1/2 to the nearest integer.  A float32 evaluation can only decide differently where the margin is of the order of
float32 error."""
from __future__ import annotations

import numpy as np


def _backproject(cam, x, y, d):
    R, t, K = cam[0][:3, :3], cam[0][:3, 3], cam[1][:3, :3]
    ray = np.linalg.inv(K) @ np.stack([x * 1.0, y * 1.0, np.ones_like(d)])
    return (R.T @ (ray * d - t[:, None])).T                                    # (n,3)


def _project(cam, X):
    R, t, K = cam[0][:3, :3], cam[0][:3, 3], cam[1][:3, :3]
    return (K @ (R @ X.T + t[:, None])).T                                      # (n,3): u, v, w


def _rounding_margin(a):
    return np.abs(a + 0.5 - np.round(a + 0.5))


def reference_fusion(depths, probs, cams, images=None, prob_threshold=0.8, reproj_threshold=1.0, depth_rel_threshold=0.01,
                     num_consistent=3, sources=None, dedupe=True):
    """-> dict(xyz (P,3) float64, rgb (P,3) uint8, view_index (P,) int32, pixel (P,) int64 (row-major index),
    keep (V,H,W) bool, count (V,H,W) int, margin (V,H,W) float64 (inf where nothing was decided))."""
    depths = np.asarray(depths, np.float32).astype(np.float64)
    probs = np.asarray(probs, np.float32).astype(np.float64)
    cams = np.asarray(cams, np.float64)
    V, H, W = depths.shape
    if sources is None:
        sources = [[s for s in range(V) if s != r] for r in range(V)]
    else:
        sources = [[s for s in sorted(set(int(s) for s in l)) if s != r] for r, l in enumerate(sources)]
    finite = np.isfinite(depths) & (depths > 0)
    valid = finite & (probs >= prob_threshold)
    rel = lambda a, thr: np.abs(a - thr) / (abs(thr) if thr != 0 else 1.0)
    used = np.zeros((V, H, W), bool)
    keep = np.zeros((V, H, W), bool)
    count = np.zeros((V, H, W), np.int64)
    margin = np.full((V, H, W), np.inf)
    pts, cols, views, pixels = [], [], [], []
    yy, xx = np.mgrid[0:H, 0:W]
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    for r in range(V):
        m = margin[r].reshape(-1)
        fin = finite[r].reshape(-1)
        m[fin] = np.minimum(m[fin], rel(probs[r].reshape(-1)[fin], prob_threshold))
        ref = valid[r].reshape(-1) & ~(used[r].reshape(-1) if dedupe else False)
        idx = np.nonzero(ref)[0]
        x, y, d = xx[idx], yy[idx], depths[r].reshape(-1)[idx]
        X = _backproject(cams[r], x, y, d)
        total = X.copy()
        n = np.zeros(len(idx), np.int64)
        witnesses = []
        for s in sources[r]:
            pm = np.full(len(idx), np.inf)
            u, v, w = _project(cams[s], X).T
            pm = np.minimum(pm, np.abs(w) / d)
            ok = w > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                us, vs = u / w, v / w
            pm[ok] = np.minimum(pm[ok], np.minimum(_rounding_margin(us[ok]), _rounding_margin(vs[ok])))
            qx = np.where(ok, np.floor(us + 0.5), -1)
            qy = np.where(ok, np.floor(vs + 0.5), -1)
            ok &= (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            qxi, qyi = np.where(ok, qx, 0).astype(np.int64), np.where(ok, qy, 0).astype(np.int64)
            ds = depths[s][qyi, qxi]
            fs = ok & finite[s][qyi, qxi]
            pm[fs] = np.minimum(pm[fs], rel(probs[s][qyi, qxi][fs], prob_threshold))
            ok &= valid[s][qyi, qxi]
            Xs = _backproject(cams[s], qxi, qyi, np.where(ok, ds, 1.0))
            u2, v2, w2 = _project(cams[r], Xs).T
            pm[ok] = np.minimum(pm[ok], np.abs(w2[ok]) / d[ok])
            ok &= w2 > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.hypot(u2 / w2 - x, v2 / w2 - y)
                drel = np.abs(w2 - d) / d
            # the pair is consistent when both criteria hold: if both do, either can flip it; if not, only a failing one can
            ce, cd = err < reproj_threshold, drel < depth_rel_threshold
            with np.errstate(invalid="ignore"):
                me, md = rel(err, reproj_threshold), rel(drel, depth_rel_threshold)
                dm = np.where(ce & cd, np.minimum(me, md), np.maximum(np.where(ce, 0, me), np.where(cd, 0, md)))
            pm[ok] = np.minimum(pm[ok], dm[ok])
            cons = ok & ce & cd
            n += cons
            total[cons] += Xs[cons]
            witnesses.append((s, cons, qyi * W + qxi))
            m[idx] = np.minimum(m[idx], pm)
        kept = n >= float(num_consistent)
        keep[r].reshape(-1)[idx] = kept
        count[r].reshape(-1)[idx] = n
        if dedupe:
            for s, cons, q in witnesses:
                used[s].reshape(-1)[q[cons & kept]] = True
        pts.append(total[kept] / (n[kept] + 1)[:, None])
        views.append(np.full(int(kept.sum()), r, np.int32))
        pixels.append(idx[kept])
        if images is not None:
            img = np.asarray(images[r])
            hi, wi = img.shape[:2]
            ix = ((2 * x[kept] + 1) * wi) // (2 * W)
            iy = ((2 * y[kept] + 1) * hi) // (2 * H)
            cols.append(img[iy, ix].astype(np.uint8))
        else:
            cols.append(np.zeros((int(kept.sum()), 3), np.uint8))
    return dict(xyz=np.concatenate(pts), rgb=np.concatenate(cols), view_index=np.concatenate(views),
                pixel=np.concatenate(pixels), keep=keep, count=count, margin=margin)


# ------------------------------------------------------------------------------------------------ analytic scenes

def _look_at(C, target):
    z = (target - C) / np.linalg.norm(target - C)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])


def make_scene(kind="plane", V=5, H=40, W=48, layout="arc", f=40.0, baseline=0.25, arc_step_deg=4.0, seed=0,
               corrupt_fraction=0.0, corrupt_view=0, low_prob_fraction=0.0, image_scale=1):
    """Depth maps ray-cast in float64 (stored float32) for V cameras in the project's (2,4,4) layout.

    kind: "plane"  fronto-parallel plane Z = 4;
          "step"   Z = 4 for world X < 0 and Z = 3.2 for X >= 0 (two half planes with a step);
          "sphere" sphere of radius 0.8 at (0, 0, 4) in front of the plane Z = 5.5 (occlusions).
    layout: "line" cameras at (i b, 0, 0) looking along +Z (with f = 64, b = 0.25 and Z = 4 every correspondence of the
            plane is a shift of exactly 4 pixels, of the step's near half plane 5); "arc" cameras on an arc through the origin around (0, 0, 4), arc_step_deg
            apart, looking at its centre.
    corrupt_fraction of corrupt_view's valid pixels get depth x U(1.3, 2) or x U(0.5, 0.75); low_prob_fraction of every view's
    pixels get probability 0.3 (the rest 1).  Images: random RGB at image_scale times the depth size.
    -> dict(depths, probs, cams, images, corrupt (H,W) bool of corrupt_view, surface_distance(X) -> (n,) distances)."""
    rs = np.random.RandomState(seed)
    cx, cy = W / 2.0 + 0.1371, H / 2.0 - 0.0613            # off the pixel grid: no projection of the symmetric layouts ties
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    centre = np.array([0.0, 0.0, 4.0])
    cams = np.zeros((V, 2, 4, 4))
    for i in range(V):
        if layout == "line":
            C, R = np.array([i * baseline, 0.0, 0.0]), np.eye(3)
        elif layout == "arc":
            th = np.radians((i - (V - 1) / 2.0) * arc_step_deg)
            C = centre + 4.0 * np.array([np.sin(th), 0.0, -np.cos(th)])
            R = _look_at(C, centre)
        else:
            raise ValueError(layout)
        cams[i, 0, :3, :3] = R
        cams[i, 0, :3, 3] = -R @ C
        cams[i, 0, 3, 3] = 1.0
        cams[i, 1, :3, :3] = K
        cams[i, 1, 3] = [0.5, 0.01, 512, 5.62]

    def planes_hit(C, dirs, Z, cond=None):
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = (Z - C[2]) / dirs[:, 2]
        lam = np.where(np.isfinite(lam) & (lam > 0), lam, np.inf)
        if cond is not None:
            Xh = C + lam[:, None] * dirs
            lam = np.where(cond(Xh), lam, np.inf)
        return lam

    def sphere_hit(C, dirs, c, rho):
        oc = C - c
        a = np.einsum("ij,ij->i", dirs, dirs)
        b = 2 * dirs @ oc
        cc = oc @ oc - rho * rho
        disc = b * b - 4 * a * cc
        sq = np.sqrt(np.maximum(disc, 0))
        l1 = (-b - sq) / (2 * a)
        return np.where((disc >= 0) & (l1 > 0), l1, np.inf)

    sph_c, sph_r = np.array([0.0, 0.0, 4.0]), 0.8
    yy, xx = np.mgrid[0:H, 0:W]
    pix = np.stack([xx.reshape(-1), yy.reshape(-1), np.ones(H * W)]).astype(np.float64)
    depths = np.zeros((V, H, W), np.float32)
    for i in range(V):
        R, t = cams[i, 0, :3, :3], cams[i, 0, :3, 3]
        C = -R.T @ t
        dirs = (R.T @ (np.linalg.inv(K) @ pix)).T                 # world ray per unit of camera depth
        if kind == "plane":
            lam = planes_hit(C, dirs, 4.0)
        elif kind == "step":
            lam = np.minimum(planes_hit(C, dirs, 4.0, lambda X: X[:, 0] < 0), planes_hit(C, dirs, 3.2, lambda X: X[:, 0] >= 0))
        elif kind == "sphere":
            lam = np.minimum(planes_hit(C, dirs, 5.5), sphere_hit(C, dirs, sph_c, sph_r))
        else:
            raise ValueError(kind)
        depths[i] = np.where(np.isfinite(lam), lam, 0).reshape(H, W)

    def surface_distance(X):
        X = np.asarray(X, np.float64)
        if kind == "plane":
            return np.abs(X[:, 2] - 4.0)
        if kind == "step":
            return np.where(X[:, 0] < 0, np.abs(X[:, 2] - 4.0), np.abs(X[:, 2] - 3.2))
        return np.minimum(np.abs(X[:, 2] - 5.5), np.abs(np.linalg.norm(X - sph_c, axis=1) - sph_r))

    probs = np.ones((V, H, W), np.float32)
    if low_prob_fraction:
        probs[rs.rand(V, H, W) < low_prob_fraction] = 0.3
    corrupt = np.zeros((H, W), bool)
    if corrupt_fraction:
        corrupt = (rs.rand(H, W) < corrupt_fraction) & (depths[corrupt_view] > 0)
        factor = np.where(rs.rand(H, W) < 0.5, rs.uniform(1.3, 2.0, (H, W)), rs.uniform(0.5, 0.75, (H, W)))
        depths[corrupt_view] = np.where(corrupt, depths[corrupt_view] * factor, depths[corrupt_view]).astype(np.float32)
    images = rs.randint(0, 256, (V, H * image_scale, W * image_scale, 3)).astype(np.uint8)
    return dict(depths=depths, probs=probs, cams=cams, images=images, corrupt=corrupt, surface_distance=surface_distance)


def plane_kat_counts(V, H, W, shift, num_consistent):
    """Kept pixels of the "plane" scene on the "line" layout, by hand: pixel column x of view i sees column x + (i - j) shift
    of view j, exactly, so n(i, x) = #{j != i : 0 <= x + (i - j) shift < W}.  -> (kept per view without dedupe, kept with
    dedupe = distinct world columns g = x + i shift kept by some view, times H)."""
    per_view, union = [], set()
    for i in range(V):
        k = 0
        for x in range(W):
            n = sum(1 for j in range(V) if j != i and 0 <= x + (i - j) * shift < W)
            if n >= num_consistent:
                k += 1
                union.add(x + i * shift)
        per_view.append(k * H)
    return per_view, len(union) * H
