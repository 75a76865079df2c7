"""Float64 numpy restatement of the normal estimation and of the fusion with normals of mvsnet_amd/fusion.py (the two
"normals" blocks of its docstring).  The scenes, _backproject and _project are those of tests/fusion_reference.py.

reference_normals also evaluates in float32 (dtype=np.float32: every quantity the kernel holds in float32 is float32 here,
the same formula in the same order without fused multiply-adds); the GPU tests take their angular bound from the distance of
that evaluation to the float64 one.

As reference_fusion does, both functions report a per-pixel MARGIN, the smallest distance of any quantity they decided on
to the boundary of that decision.  On top of reference_fusion's margins:
  * the relative distance of each in-image valid neighbour's depth jump |d_q - d| / d to jump_threshold,
  * |n . view direction| (the sign decides the orientation),
  * |n_r . n_s - cos(normal_angle_threshold)| for every geometrically consistent pair when the threshold is set,
  * |N| of a kept pixel whose sum has at least one contribution (without any it is exactly zero everywhere)."""
from __future__ import annotations

import numpy as np

from tests.fusion_reference import _backproject, _project, _rounding_margin, make_scene  # noqa: F401  (make_scene: re-export)


def angle_deg(a, b):
    """Angle between the rows of a and b in degrees, atan2(|a x b|, a . b) in float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))


def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx], 0 outside the image; and the inside mask."""
    H, W = a.shape
    b = np.zeros_like(a)
    inside = np.zeros((H, W), bool)
    ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
    yd, xd = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
    b[ys, xs] = a[yd, xd]
    inside[ys, xs] = True
    return b, inside


def reference_normals(depths, probs, cams, prob_threshold=0.8, jump_threshold=0.05, dtype=np.float64):
    """-> dict(normals (V,H,W,3) dtype in the world frame, (0,0,0) = none; has (V,H,W) bool; margin (V,H,W) float64)."""
    T = np.dtype(dtype).type
    D = np.asarray(depths, np.float32)
    P = np.asarray(probs, np.float32)
    cams = np.asarray(cams, np.float64)
    V, H, W = D.shape
    finite = np.isfinite(D) & (D > 0)
    valid = finite & (P >= np.float32(prob_threshold))
    jump = T(jump_threshold)
    normals = np.zeros((V, H, W, 3), dtype)
    has = np.zeros((V, H, W), bool)
    margin = np.full((V, H, W), np.inf)
    yy, xx = np.mgrid[0:H, 0:W]
    fx, fy = xx.astype(dtype), yy.astype(dtype)
    relp = lambda p: np.abs(p.astype(np.float64) - prob_threshold) / (abs(prob_threshold) if prob_threshold != 0 else 1.0)
    for v in range(V):
        R, K = cams[v][0][:3, :3], cams[v][1][:3, :3]
        A = (R.T @ np.linalg.inv(K)).astype(np.float32).astype(dtype)          # the kernel reads the float32 table
        d = np.where(valid[v], D[v], np.float32(0)).astype(dtype)
        m = margin[v]
        m[finite[v]] = relp(P[v])[finite[v]]
        use = {}
        for name, dy, dx in (("l", 0, -1), ("r", 0, 1), ("u", -1, 0), ("d", 1, 0)):
            dq, inside = _shift(d, dy, dx)
            fq, _ = _shift(finite[v], dy, dx)
            pq, _ = _shift(P[v], dy, dx)
            sel = valid[v] & inside & fq                                        # the neighbour's validity was decided on
            m[sel] = np.minimum(m[sel], relp(pq)[sel])
            with np.errstate(divide="ignore", invalid="ignore"):
                u = valid[v] & inside & (dq > 0) & (np.abs(dq - d) < jump * d)
                sel = valid[v] & inside & (dq > 0)
                jm = np.abs(np.abs(dq.astype(np.float64) - d) / d.astype(np.float64) - jump_threshold) / jump_threshold
            m[sel] = np.minimum(m[sel], jm[sel])
            use[name] = (u, dq)
        (ul, dl), (ur, dr), (uu, du), (ud, dd) = use["l"], use["r"], use["u"], use["d"]
        cand = valid[v] & (ul | ur) & (uu | ud)
        one = T(1)
        xh, dxh, xl, dxl = np.where(ur, fx + one, fx), np.where(ur, dr, d), np.where(ul, fx - one, fx), np.where(ul, dl, d)
        yh, dyh, yl, dyl = np.where(ud, fy + one, fy), np.where(ud, dd, d), np.where(uu, fy - one, fy), np.where(uu, du, d)
        tx = np.stack([xh * dxh - xl * dxl, fy * dxh - fy * dxl, dxh - dxl], -1)
        ty = np.stack([fx * dyh - fx * dyl, yh * dyh - yl * dyl, dyh - dyl], -1)
        q, p = tx @ A.T, ty @ A.T
        c = np.cross(p, q)                                                      # A ty x A tx
        len2 = (c * c).sum(-1)
        ok = cand & (len2 > 0) & np.isfinite(len2)
        with np.errstate(divide="ignore", invalid="ignore"):
            n = c / np.sqrt(len2)[..., None]
        g = np.stack([fx * d, fy * d, d], -1) @ A.T                             # X - C_v
        dot = (n * g).sum(-1)
        n = np.where((dot > 0)[..., None], -n, n)
        normals[v] = np.where(ok[..., None], n, T(0))
        has[v] = ok
        with np.errstate(divide="ignore", invalid="ignore"):
            vm = np.abs(dot.astype(np.float64)) / np.linalg.norm(g.astype(np.float64), axis=-1)
        m[ok] = np.minimum(m[ok], vm[ok])
    return dict(normals=normals, has=has, margin=margin)


def reference_fusion_normals(depths, probs, cams, images=None, prob_threshold=0.8, reproj_threshold=1.0, depth_rel_threshold=0.01,
                             num_consistent=3, sources=None, dedupe=True, normal_angle_threshold=None, jump_threshold=0.05):
    """reference_fusion with normals -> its dict plus normals (P,3) float64 ((0,0,0) = none), geometric_pairs and
    rejected_pairs (geometrically consistent pairs, and those of them the normal test rejected)."""
    depths = np.asarray(depths, np.float32).astype(np.float64)
    probs = np.asarray(probs, np.float32).astype(np.float64)
    cams = np.asarray(cams, np.float64)
    V, H, W = depths.shape
    nm = reference_normals(depths, probs, cams, prob_threshold, jump_threshold)
    NM, HAS, NMM = nm["normals"].reshape(V, H * W, 3), nm["has"].reshape(V, H * W), nm["margin"].reshape(V, H * W)
    thr_on = normal_angle_threshold is not None
    cos_thr = np.cos(np.radians(normal_angle_threshold)) if thr_on else -1.0
    if sources is None:
        sources = [[s for s in range(V) if s != r] for r in range(V)]
    else:
        sources = [[s for s in sorted(set(int(s) for s in l)) if s != r] for r, l in enumerate(sources)]
    finite = np.isfinite(depths) & (depths > 0)
    valid = finite & (probs >= prob_threshold)
    if thr_on:
        valid = valid & nm["has"]                                               # a pixel without a normal is not valid
    rel = lambda a, thr: np.abs(a - thr) / (abs(thr) if thr != 0 else 1.0)
    used = np.zeros((V, H, W), bool)
    keep = np.zeros((V, H, W), bool)
    count = np.zeros((V, H, W), np.int64)
    margin = np.full((V, H, W), np.inf)
    pts, cols, views, pixels, nrms = [], [], [], [], []
    geometric_pairs = rejected_pairs = 0
    yy, xx = np.mgrid[0:H, 0:W]
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    for r in range(V):
        m = margin[r].reshape(-1)
        fin = finite[r].reshape(-1)
        m[fin] = np.minimum(m[fin], np.minimum(rel(probs[r].reshape(-1)[fin], prob_threshold), NMM[r][fin]))
        ref = valid[r].reshape(-1) & ~(used[r].reshape(-1) if dedupe else False)
        idx = np.nonzero(ref)[0]
        x, y, d = xx[idx], yy[idx], depths[r].reshape(-1)[idx]
        X = _backproject(cams[r], x, y, d)
        total = X.copy()
        nr = NM[r][idx]
        N = nr.copy()
        contrib = HAS[r][idx].copy()
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
            q = qyi * W + qxi
            ds = depths[s][qyi, qxi]
            fs = ok & finite[s][qyi, qxi]
            pm[fs] = np.minimum(pm[fs], np.minimum(rel(probs[s][qyi, qxi][fs], prob_threshold), NMM[s][q][fs]))
            ok &= valid[s][qyi, qxi]
            Xs = _backproject(cams[s], qxi, qyi, np.where(ok, ds, 1.0))
            u2, v2, w2 = _project(cams[r], Xs).T
            pm[ok] = np.minimum(pm[ok], np.abs(w2[ok]) / d[ok])
            ok &= w2 > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.hypot(u2 / w2 - x, v2 / w2 - y)
                drel = np.abs(w2 - d) / d
            ce, cd = err < reproj_threshold, drel < depth_rel_threshold
            with np.errstate(invalid="ignore"):
                me, md = rel(err, reproj_threshold), rel(drel, depth_rel_threshold)
                dm = np.where(ce & cd, np.minimum(me, md), np.maximum(np.where(ce, 0, me), np.where(cd, 0, md)))
            pm[ok] = np.minimum(pm[ok], dm[ok])
            cons = ok & ce & cd
            ns = NM[s][q]
            geometric_pairs += int(cons.sum())
            if thr_on:
                dot = (nr * ns).sum(-1)
                pm[cons] = np.minimum(pm[cons], np.abs(dot - cos_thr)[cons])
                rejected_pairs += int((cons & ~(dot > cos_thr)).sum())
                cons &= dot > cos_thr
            n += cons
            total[cons] += Xs[cons]
            N[cons] += ns[cons]
            contrib |= cons & HAS[s][q]
            witnesses.append((s, cons, q))
            m[idx] = np.minimum(m[idx], pm)
        kept = n >= float(num_consistent)
        length = np.linalg.norm(N, axis=1)
        sel = kept & contrib
        m[idx[sel]] = np.minimum(m[idx[sel]], length[sel])
        keep[r].reshape(-1)[idx] = kept
        count[r].reshape(-1)[idx] = n
        if dedupe:
            for s, cons, q in witnesses:
                used[s].reshape(-1)[q[cons & kept]] = True
        pts.append(total[kept] / (n[kept] + 1)[:, None])
        with np.errstate(divide="ignore", invalid="ignore"):
            unit = np.where((length > 0)[:, None], N / length[:, None], 0.0)
        nrms.append(unit[kept])
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
                pixel=np.concatenate(pixels), normals=np.concatenate(nrms), keep=keep, count=count, margin=margin,
                geometric_pairs=geometric_pairs, rejected_pairs=rejected_pairs)
