"""float64 numpy restatement of the point-to-point ICP registration of mvsnet_amd/register.py (its docstring is normative):
the transform and the brute-force correspondences of tests/pointcloud_reference.py, the eighteen moments by math.fsum, the
Kabsch / Umeyama solve, the loop with the module's stop rule, error measures, and a seeded asymmetric scene."""
import math

import numpy as np

from tests import pointcloud_reference as R

MOMENTS = 18


def correspondences(moved, target, max_dist):
    """-> (d (n,) float64, inf beyond; idx (n,) int64, -1 beyond) by brute force (pointcloud_reference.nearest)."""
    d, idx, _, _ = R.nearest(moved, target, max_dist)
    return d, idx


def tree_correspondences(moved, target, max_dist, k=4):
    """The same answer as `correspondences`, faster: a k-d tree proposes k candidates per point, their squared distances are
    recomputed with nearest()'s own expression and ties go to the smallest index; a point whose k candidates all tie (more
    duplicates than k) goes to the brute force.  Without scipy it is the brute force."""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return correspondences(moved, target, max_dist)
    q, t = np.asarray(moved, np.float64), np.asarray(target, np.float64)
    k = min(k, len(t))
    cand = cKDTree(t).query(q, k=k)[1].reshape(len(q), k)
    tc = t[cand]
    d2 = ((q[:, None, 0] - tc[:, :, 0]) ** 2 + (q[:, None, 1] - tc[:, :, 1]) ** 2) + (q[:, None, 2] - tc[:, :, 2]) ** 2
    m = d2.min(1)
    idx = np.where(d2 == m[:, None], cand, np.iinfo(np.int64).max).min(1)
    d_all = np.sqrt(m)
    crowded = (d2 == m[:, None]).all(1) & (len(t) > k)
    if crowded.any():
        _, bi, ball, _ = R.nearest(q[crowded], t, np.inf)
        idx[crowded], d_all[crowded] = bi, ball
    inside = d_all <= max_dist
    return np.where(inside, d_all, np.inf), np.where(inside, idx, -1)


def transform64(points, T):
    """T p in float64, rows left to right as pointcloud_reference.transform, NOT rounded to float32."""
    p = np.asarray(points, np.float32).astype(np.float64)
    T = np.asarray(T, np.float64)
    return np.stack([((p[:, 0] * T[i, 0] + p[:, 1] * T[i, 1]) + p[:, 2] * T[i, 2]) + T[i, 3] for i in range(3)], 1)


def moment_terms(source, target, idx, T, cp, cq):
    """(m, 18) float64: the terms of the moments, one row per source point with a neighbour (idx >= 0), in input order."""
    ok = np.asarray(idx) >= 0
    p = np.asarray(source, np.float32).astype(np.float64)[ok]
    q = np.asarray(target, np.float32).astype(np.float64)[np.asarray(idx)[ok]]
    a, b = p - np.asarray(cp, np.float64), q - np.asarray(cq, np.float64)
    r = transform64(np.asarray(source, np.float32)[ok], T) - q
    return np.concatenate([np.ones((len(p), 1)), ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])[:, None], a, b,
                           (a[:, :, None] * b[:, None, :]).reshape(len(p), 9),
                           ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])[:, None]], 1)


def moments_from_terms(terms):
    """-> (moments (18,) by math.fsum, sum of |term| (18,) by math.fsum)."""
    return (np.array([math.fsum(terms[:, k]) for k in range(MOMENTS)]),
            np.array([math.fsum(np.abs(terms[:, k])) for k in range(MOMENTS)]))


def step(source, target, T, max_dist, cp, cq, nn=correspondences):
    """One registration step -> (moments (18,), idx)."""
    _, idx = nn(R.transform(source, T), target, max_dist)
    return moments_from_terms(moment_terms(source, target, idx, T, cp, cq))[0], idx


def solve_from_moments(moments, cp, cq, with_scale=False):
    """-> (4x4 transform or None, reason or None); the statement of register.solve_from_moments."""
    m = np.asarray(moments, np.float64)
    n = m[0]
    if n < 3:
        return None, "too_few_correspondences"
    sa, sb = m[2:5], m[5:8]
    H = m[8:17].reshape(3, 3) - np.outer(sa, sb) / n
    var = m[17] - float(sa @ sa) / n
    U, S, Vt = np.linalg.svd(H)
    if not (S[1] > 1e-12 * S[0]) or (with_scale and not var > 0):
        return None, "degenerate"
    D = np.array([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    Rm = (Vt.T * D) @ U.T
    s = float((S * D).sum()) / var if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3] = s * Rm
    T[:3, 3] = (np.asarray(cq, np.float64) + sb / n) - s * (Rm @ (np.asarray(cp, np.float64) + sa / n))
    return T, None


def icp(source, target, max_dist, init=None, with_scale=False, max_iterations=50, fitness_tol=1e-6, rmse_tol=1e-6,
        nn=tree_correspondences):
    """The loop of register.RegistrationPlan.run -> the same result dict plus "trajectory": the transform every step was
    taken at."""
    src, tgt = np.asarray(source, np.float32), np.asarray(target, np.float32)
    cp, cq = src.astype(np.float64).mean(0), tgt.astype(np.float64).mean(0)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    history, trajectory, prev, stopped, it = [], [], None, "max_iterations", 0
    fitness, rmse = 0.0, None
    while it < max_iterations:
        m, _ = step(src, tgt, T, max_dist, cp, cq, nn)
        trajectory.append(T.copy())
        it += 1
        fitness = m[0] / len(src)
        rmse = math.sqrt(m[1] / m[0]) if m[0] > 0 else None
        history.append([fitness, rmse])
        if prev is not None and rmse is not None and prev[1] is not None and abs(fitness - prev[0]) < fitness_tol and \
                abs(rmse - prev[1]) < rmse_tol * max_dist:
            stopped = "converged"
            break
        new, why = solve_from_moments(m, cp, cq, with_scale)
        if new is None:
            stopped = why
            break
        prev, T = (fitness, rmse), new
    return {"transform": T.tolist(), "fitness": fitness, "inlier_rmse": rmse, "iterations": it, "stopped": stopped,
            "history": history, "trajectory": trajectory}


# ------------------------------------------------------------------------------------------------ error measures

def errors(T, T0):
    """E = T T0^-1 -> (rotation error: the norm of the skew part of E's rotation, which keeps its precision where arccos of
    the trace loses it below 1e-8; translation error |E[:3,3]|; scale of E)."""
    E = np.asarray(T, np.float64) @ np.linalg.inv(np.asarray(T0, np.float64))
    s = float(np.cbrt(np.linalg.det(E[:3, :3])))
    Rm = E[:3, :3] / s
    K = (Rm - Rm.T) / 2
    return float(np.sqrt(K[2, 1] ** 2 + K[0, 2] ** 2 + K[1, 0] ** 2)), float(np.linalg.norm(E[:3, 3])), s


# ------------------------------------------------------------------------------------------------ seeded generators

def asymmetric_scene(n, seed=0, extent=100.0):
    """A height field z = 8 sin(x/9) cos(y/7) + 5 sin((x+2y)/13) over an extent x extent square (3/4 of the points) and a
    sphere of radius 12 centred at (18, -11, 20): no symmetry leaves a rotation or a translation unconstrained."""
    rs = np.random.RandomState(seed)
    ns = n // 4
    nh = n - ns
    x, y = rs.uniform(-extent / 2, extent / 2, nh), rs.uniform(-extent / 2, extent / 2, nh)
    z = 8 * np.sin(x / 9) * np.cos(y / 7) + 5 * np.sin((x + 2 * y) / 13)
    v = rs.standard_normal((ns, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.concatenate([np.stack([x, y, z], 1), v * 12 + np.array([18.0, -11.0, 20.0])]).astype(np.float32)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rigid(axis=(1, 2, 3), degrees=3.0, translation=(1.5, -1.0, 0.8), scale=1.0):
    T = np.eye(4)
    T[:3, :3] = scale * rotation(axis, degrees)
    T[:3, 3] = translation
    return T


MAX_CORR_DIST = 5.0


def cases():
    """The three registration cases of the tests -> {"target", "T0", "T0s", "A", "B", "C"}: a 9 000-point target; T0 = 3 degrees
    about (1,2,3) with translation (1.5, -1, 0.8); A = T0^-1 of every second target point; B = an independent sample of the
    scene with N(0, 0.3) noise, moved by T0^-1, plus 5 % uniform outliers; C = as A with scale 1.03 (T0s)."""
    tgt = asymmetric_scene(9000, seed=31)
    T0, T0s = rigid(), rigid(scale=1.03)
    return {"target": tgt, "T0": T0, "T0s": T0s,
            "A": R.transform(tgt[::2], np.linalg.inv(T0)),
            "B": R.with_outliers(R.transform(R.noisy(asymmetric_scene(7000, seed=32), 0.3, seed=33), np.linalg.inv(T0)), 0.05,
                                 -60, 60, seed=34),
            "C": R.transform(tgt[::2], np.linalg.inv(T0s))}
