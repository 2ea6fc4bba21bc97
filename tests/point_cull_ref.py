"""TEST INFRASTRUCTURE ONLY — Python restatement of map point culling
(viso_set_point_cull / viso_point_tracks_update / viso_points_cull,
include/viso/viso_c.h; DESIGN.md §Map point culling).  The repo's own spec:
the reference computes every map point's alignment in every tracking frame
(LKAlignment, src/viso.cpp:768-843) and only draws it; its map
(src/viso.cpp:79-96) never loses a point.

Every expression is elementwise numpy fp64 arithmetic in the device's operand
order, that of tests/pose_refine_ref.py: a 3-term dot product is
(a0 b0 + a1 b1) + a2 b2, nothing is contracted (every product and sum is a
ufunc call of its own).  Poses are Tcw, 12 doubles (R row-major, t):
Pc = R Pw + t.  A track record is int32 {age, seen, found, fail_run}.
"""
from __future__ import annotations

import numpy as np


def project(points, pose, K):
    """(u, v, z) of every point under pose (elementwise, the kernel's order);
    u and v are meaningless where z is not positive."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    T = np.asarray(pose, np.float64).reshape(12)
    fx, fy, cx, cy = (float(k) for k in K)
    Pc = [(T[3 * r] * P[:, 0] + T[3 * r + 1] * P[:, 1]) + T[3 * r + 2] * P[:, 2] for r in range(3)]
    x, y, z = Pc[0] + T[9], Pc[1] + T[10], Pc[2] + T[11]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = fx * x / z + cx
        v = fy * y / z + cy
    return u, v, z


def update(tracks, points, pair_kf, success, uv_after, pose, K, reproj_px):
    """One tracking frame's update.  Returns a dict: tracks (n, 4) int32 (a new
    array), counts [paired, good, failed, longest fail_run after the update],
    good (n,) bool, e (n,) the reprojection error in pixels (NaN where the
    point is not paired or not in front of the camera), margin: the smallest
    | e - reproj_px | over the paired, successful points in front of the
    camera (inf: none) — the distance of a flag from flipping."""
    tr = np.array(tracks, np.int32).reshape(-1, 4)
    n = tr.shape[0]
    pk = np.asarray(pair_kf).reshape(-1)
    sc = np.asarray(success).reshape(-1)
    ua = np.asarray(uv_after, np.float64).reshape(-1, 2)
    assert len(pk) == len(sc) == len(ua) == n and np.asarray(points).reshape(-1, 3).shape[0] == n
    r2 = float(reproj_px) * float(reproj_px)
    u, v, z = project(points, pose, K)
    paired = pk >= 0
    front = z > 0
    with np.errstate(invalid="ignore", over="ignore"):
        r0 = ua[:, 0] - u
        r1 = ua[:, 1] - v
        e2 = r0 * r0 + r1 * r1
        within = e2 <= r2
    good = paired & (sc != 0) & front & within
    tr[:, 0] += 1
    tr[paired, 1] += 1
    tr[good, 2] += 1
    tr[good, 3] = 0
    tr[paired & ~good, 3] += 1
    e = np.where(paired & front, np.sqrt(np.where(paired & front, e2, 0.0)), np.nan)
    m = paired & (sc != 0) & front
    margin = float(np.abs(e[m] - float(reproj_px)).min()) if m.any() else float("inf")
    counts = [int(paired.sum()), int(good.sum()), int((paired & ~good).sum()), int(tr[:, 3].max()) if n else 0]
    counts[3] = max(counts[3], 0)
    return {"tracks": tr, "counts": counts, "good": good, "e": e, "margin": margin}


def cull(points, host, tracks, max_fail_run, min_points):
    """One cull.  Returns a dict: keep (n,) uint8, points / host / tracks (the
    kept rows in order), counts [candidates, survivors = n - candidates, kept,
    abandoned], applied (something left the map)."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    hst = np.asarray(host, np.int32).reshape(-1)
    tr = np.asarray(tracks, np.int32).reshape(-1, 4)
    n = len(pts)
    assert len(hst) == n and len(tr) == n
    cand = tr[:, 3] >= int(max_fail_run)
    n_cand = int(cand.sum())
    surv = n - n_cand
    abandoned = n_cand > 0 and surv < int(min_points)
    keep = np.ones(n, bool) if abandoned else ~cand
    idx = np.nonzero(keep)[0]  # ascending: the survivors keep their order
    return {"keep": keep.astype(np.uint8), "points": pts[idx].copy(), "host": hst[idx].copy(),
            "tracks": tr[idx].copy(), "counts": [n_cand, surv, len(idx), int(abandoned)],
            "applied": n_cand > 0 and not abandoned}
