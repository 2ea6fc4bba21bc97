"""TEST INFRASTRUCTURE ONLY — Python restatement of one monocular keyframe
insertion (viso_set_mono_keyframes / viso_mono_points, include/viso/viso_c.h;
DESIGN.md §Monocular keyframe insertion).  The repo's own spec: the reference
sketches the triangulation in Viso::Reconstruct (src/viso.cpp:434-501) and
never calls it.

FAST, the pyramidal KLT, the pyramid and Triangulate come from the CPU oracle
(tests/oracle_lib.py); every other expression is scalar Python float (fp64)
arithmetic in the device's operand order: a 3-term dot product is
(a0 b0 + a1 b1) + a2 b2, nothing is contracted.  Poses are Tcw, 12 doubles
(R row-major, t): Pc = R Pw + t.
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle_lib


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def kinv(K):
    """K.inverse() as the library computes it (cofactors times 1 / det)."""
    fx, fy, cx, cy = (float(x) for x in K)
    m = [fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0]

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[3 * i1 + j1] * m[3 * i2 + j2] - m[3 * i1 + j2] * m[3 * i2 + j1]

    c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]
    det = (c0[0] * m[0] + c0[1] * m[3]) + c0[2] * m[6]
    inv = 1.0 / det
    return [c0[0] * inv, c0[1] * inv, c0[2] * inv,
            cof(0, 1) * inv, cof(1, 1) * inv, cof(2, 1) * inv,
            cof(0, 2) * inv, cof(1, 2) * inv, cof(2, 2) * inv]


def mat_vec(M, v):
    return [dot3(M[3 * r], M[3 * r + 1], M[3 * r + 2], v[0], v[1], v[2]) for r in range(3)]


def relative_motion(pose_c, pose_k):
    """R_kc = R_k R_c^T, T_kc = t_k - R_kc t_c."""
    Rc, tc = [float(x) for x in pose_c[:9]], [float(x) for x in pose_c[9:12]]
    Rk, tk = [float(x) for x in pose_k[:9]], [float(x) for x in pose_k[9:12]]
    R = [dot3(Rk[3 * i], Rk[3 * i + 1], Rk[3 * i + 2], Rc[3 * j], Rc[3 * j + 1], Rc[3 * j + 2])
         for i in range(3) for j in range(3)]
    Rt = mat_vec(R, tc)
    T = [tk[r] - Rt[r] for r in range(3)]
    return R, T


def occupancy(points, pose_c, K, width, height, cell):
    """The set of (cx, cy) cells that a map point projects into in frame c."""
    fx, fy, cx, cy = (float(x) for x in K)
    R, t = [float(x) for x in pose_c[:9]], [float(x) for x in pose_c[9:12]]
    occ = set()
    for P in np.asarray(points, np.float64).reshape(-1, 3):
        Pc = mat_vec(R, [float(P[0]), float(P[1]), float(P[2])])
        Pc = [Pc[r] + t[r] for r in range(3)]
        if not Pc[2] > 0:
            continue
        u = fx * Pc[0] / Pc[2] + cx
        v = fy * Pc[1] / Pc[2] + cy
        if 0 <= u < width and 0 <= v < height:
            occ.add((int(u / cell), int(v / cell)))
    return occ


def cell_winners(xs, ys, sc, occ, cell):
    """Indices (ascending = row-major corner order) of the corners that win
    their unmarked cell: highest score, ties to the first corner."""
    best = {}
    for i in range(len(xs)):
        c = (int(xs[i]) // cell, int(ys[i]) // cell)
        if c in occ:
            continue
        key = (int(sc[i]) << 32) | (0xFFFFFFFF - i)
        if key > best.get(c, -1):
            best[c] = key
    return sorted(0xFFFFFFFF - (k & 0xFFFFFFFF) for k in best.values())


def mono_points(cur_pyr, kf_pyr, width, height, K, pose_c, pose_k, points, cell, min_parallax_deg,
                fast_thresh=50, max_features=32768, projection_error_thresh=0.3,
                photometric_error_thresh=14400.0):
    """One insertion's new points.  cur_pyr / kf_pyr: oracle_lib.pyramid of
    the current frame c and of the latest keyframe k.  Returns a dict:
    points (m, 3) world, xy (winners, 2) int32, accept (winners,) uint8,
    counts [corners, winners, KLT successes, accepted], and per winner the
    values compared with a threshold (err1, err2, cosang; NaN where the
    candidate was rejected before the value exists) with cos_thresh."""
    fx, fy, cx, cy = (float(x) for x in K)
    Ki = kinv(K)
    img = np.ascontiguousarray(cur_pyr[:width * height]).reshape(height, width)
    xs, ys, sc = oracle_lib.fast(img, fast_thresh)
    xs, ys, sc = xs[:max_features], ys[:max_features], sc[:max_features]
    occ = occupancy(points, pose_c, K, width, height, cell)
    win = cell_winners(xs, ys, sc, occ, cell)
    n = len(win)
    R, T = relative_motion(pose_c, pose_k)
    kp1 = np.zeros((n, 2), np.float32)
    kp2 = np.zeros((n, 2), np.float32)
    for j, i in enumerate(win):
        kp1[j] = (np.float32(xs[i]), np.float32(ys[i]))
        x1 = mat_vec(Ki, [float(kp1[j, 0]), float(kp1[j, 1]), 1.0])
        q = mat_vec(R, x1)
        kp2[j] = (np.float32(fx * q[0] / q[2] + cx), np.float32(fy * q[1] / q[2] + cy))
    if n:
        kp2, succ = oracle_lib.klt(cur_pyr, kf_pyr, width, height, kp1, kp2, photometric_error_thresh)
    else:
        succ = np.zeros(0, np.uint8)
    cos_thresh = math.cos(min_parallax_deg * 3.14159265358979323846 / 180.0)
    O2 = [dot3(-R[r], -R[3 + r], -R[6 + r], T[0], T[1], T[2]) for r in range(3)]
    Rc, tc = [float(x) for x in pose_c[:9]], [float(x) for x in pose_c[9:12]]
    accept = np.zeros(n, np.uint8)
    err1 = np.full(n, np.nan)
    err2 = np.full(n, np.nan)
    cosang = np.full(n, np.nan)
    out = []
    for j in range(n):
        if not succ[j]:
            continue
        x1 = mat_vec(Ki, [float(kp1[j, 0]), float(kp1[j, 1]), 1.0])
        x2 = mat_vec(Ki, [float(kp2[j, 0]), float(kp2[j, 1]), 1.0])
        with np.errstate(all="ignore"):
            P = [float(v) for v in oracle_lib.triangulate(R, T, x1, x2)]
        if not all(math.isfinite(v) for v in P):
            continue
        if not P[2] > 0:
            continue
        P2 = mat_vec(R, P)
        P2 = [P2[r] + T[r] for r in range(3)]
        if not P2[2] > 0:
            continue
        dx = (P[0] / P[2] - x1[0]) * fx
        dy = (P[1] / P[2] - x1[1]) * fy
        err1[j] = math.sqrt(dx * dx + dy * dy)
        dx = (P2[0] / P2[2] - x2[0]) * fx
        dy = (P2[1] / P2[2] - x2[1]) * fy
        err2[j] = math.sqrt(dx * dx + dy * dy)
        n2 = [P[r] - O2[r] for r in range(3)]
        d1 = math.sqrt(dot3(P[0], P[1], P[2], P[0], P[1], P[2]))
        d2 = math.sqrt(dot3(n2[0], n2[1], n2[2], n2[0], n2[1], n2[2]))
        cosang[j] = dot3(P[0], P[1], P[2], n2[0], n2[1], n2[2]) / (d1 * d2)
        if not err1[j] <= projection_error_thresh or not err2[j] <= projection_error_thresh:
            continue
        if not cosang[j] <= cos_thresh:
            continue
        accept[j] = 1
        d = [P[r] - tc[r] for r in range(3)]
        out.append([dot3(Rc[k], Rc[3 + k], Rc[6 + k], d[0], d[1], d[2]) for k in range(3)])
    xy = np.array([[xs[i], ys[i]] for i in win], np.int32).reshape(-1, 2)
    return {"points": np.array(out, np.float64).reshape(-1, 3), "xy": xy, "accept": accept,
            "counts": [len(xs), n, int(np.count_nonzero(succ)), int(accept.sum())],
            "err1": err1, "err2": err2, "cosang": cosang, "cos_thresh": cos_thresh,
            "kp2": kp2, "success": np.asarray(succ, np.uint8)}
