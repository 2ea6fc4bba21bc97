"""TEST INFRASTRUCTURE ONLY — numpy restatement of the relocalisation seed
(viso_reloc_seed, viso_set_reloc_seed, include/viso/viso_c.h):
a pose seed for the keyframe alignment from descriptor matches between the
map's points (described in their host keyframes) and the FAST corners of the
current frame.  The repo's own spec.

Integers (descriptors, Hamming distances, ranks, draws) are numpy integer
arithmetic; the hypotheses are scalar Python floats in the device's operand
order through tests/pose_refine_ref.py (`point_terms` with an infinite Huber
bound: the weight is exactly 1.0), its `solve` (inverse6) and `left_update`;
the refinement is `pose_refine_ref.refine` itself on the best hypothesis's
inliers in the LK-row form.  A hypothesis depends on its three draws alone, so
equal triples are computed once.
"""
from __future__ import annotations

import math

import numpy as np

from tests.lk_warp_ref import levels, project
from tests.pose_refine_ref import left_update, point_terms, refine, solve

BITS = 256
BORDER = 6
GN_PASSES = 10
REFINE_ITERATIONS = 10
NAN = float("nan")
_M64 = (1 << 64) - 1


def mix64(z):
    """common.hpp mix64 (splitmix64's finaliser behind one increment)."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def offsets():
    """(256, 4) ints: ax, ay, bx, by of every bit."""
    return np.array([[mix64(4 * b + c) % 13 - 6 for c in range(4)] for b in range(BITS)], np.int64)


_OFF = offsets()


def describe(level1, w1, h1, xs, ys):
    """Descriptors of the level-0 integer pixels (xs, ys) on a level-1 buffer:
    (valid (n,) bool, words (n, 8) uint32, zero where not valid)."""
    xs, ys = np.asarray(xs, np.int64).reshape(-1), np.asarray(ys, np.int64).reshape(-1)
    x1, y1 = xs >> 1, ys >> 1
    valid = (x1 >= BORDER) & (x1 < w1 - BORDER) & (y1 >= BORDER) & (y1 < h1 - BORDER)
    words = np.zeros((xs.size, 8), np.uint32)
    g = np.nonzero(valid)[0]
    if g.size:
        img = np.asarray(level1, np.uint8).reshape(h1, w1)
        a = img[y1[g, None] + _OFF[None, :, 1], x1[g, None] + _OFF[None, :, 0]]
        b = img[y1[g, None] + _OFF[None, :, 3], x1[g, None] + _OFF[None, :, 2]]
        packed = np.packbits(a < b, axis=1, bitorder="little")  # bit b in byte b / 8
        words[g] = np.ascontiguousarray(packed).view("<u4")
    return valid, words


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words.astype("<u4")).view(np.uint8), axis=1,
                         bitorder="little").astype(np.float32)


def hamming(pw, cw):
    """(n_p, n_c) int32 Hamming distances (integers below 2^24 are exact in fp32)."""
    a, b = _bits(pw), _bits(cw)
    return np.rint(a @ (1 - b).T + (1 - a) @ b.T).astype(np.int32)


def map_side(kf_pyrs, kf_poses, points, hosts, w, h, K):
    """Step 2: (described (n,) bool, words (n, 8))."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    hosts = np.asarray(hosts, np.int64).reshape(-1)
    n = pts.shape[0]
    described, words = np.zeros(n, bool), np.zeros((n, 8), np.uint32)
    kf_poses = np.asarray(kf_poses, np.float64).reshape(-1, 12)
    for k in range(kf_poses.shape[0]):
        idx = np.nonzero(hosts == k)[0]
        if idx.size == 0:
            continue
        lv, ws, hs = levels(kf_pyrs[k], w, h)
        with np.errstate(all="ignore"):
            u, v, z = project(kf_poses[k], K, (pts[idx, 0], pts[idx, 1], pts[idx, 2]))
            ok = (z > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        x = np.where(ok, u + 0.5, 0.0).astype(np.int64)
        y = np.where(ok, v + 0.5, 0.0).astype(np.int64)
        val, wd = describe(lv[1], ws[1], hs[1], x, y)
        val &= ok
        described[idx] = val
        words[idx[val]] = wd[val]
    return described, words


def current_side(cur_pyr, w, h, corners_x, corners_y, max_features):
    """Step 3: the kept corners (xs, ys) and their words."""
    xs = np.asarray(corners_x, np.int64).reshape(-1)[:max_features]
    ys = np.asarray(corners_y, np.int64).reshape(-1)[:max_features]
    lv, ws, hs = levels(cur_pyr, w, h)
    val, wd = describe(lv[1], ws[1], hs[1], xs, ys)
    return xs[val], ys[val], wd[val]


def match(described, pw, cw, max_hamming, ratio_permille):
    """Step 4: the match list (M, 3) int32 = (point, kept corner, distance) and
    per point (best, second, corner) (n, 3), -1 / 257 where there is none."""
    n, nc = described.shape[0], cw.shape[0]
    per_point = np.tile(np.array([257, 257, -1], np.int32), (n, 1))
    d_idx = np.nonzero(described)[0]
    if nc == 0 or d_idx.size == 0:
        return np.zeros((0, 3), np.int32), per_point
    D = hamming(pw[d_idx], cw)
    ci = D.argmin(axis=1)  # the first minimum: the lowest corner index
    rows = np.arange(d_idx.size)
    best = D[rows, ci]
    if nc >= 2:
        D2 = D.copy()
        D2[rows, ci] = 1 << 20
        second = D2.min(axis=1)
    else:
        second = np.full(d_idx.size, 257, np.int32)
    per_point[d_idx, 0], per_point[d_idx, 1], per_point[d_idx, 2] = best, second, ci
    back = d_idx[D.argmin(axis=0)]  # every corner's best point: the lowest point index
    ok = (best <= max_hamming) & (best.astype(np.int64) * 1000 < ratio_permille * second.astype(np.int64)) & \
         (back[ci] == d_idx)
    return np.stack([d_idx[ok], ci[ok], best[ok]], 1).astype(np.int32), per_point


def draw(seed, h, M):
    """Hypothesis h's three distinct list positions."""
    r = [mix64((seed + 4 * h + k) & _M64) for k in range(3)]
    i0 = r[0] % M
    i1 = r[1] % (M - 1)
    if i1 >= i0:
        i1 += 1
    i2 = r[2] % (M - 2)
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


def hypothesis(P3, uv3, S, K):
    """Ten unweighted Gauss-Newton passes on three matches from S: the pose
    (12 floats), or None when a depth is <= 0 or a step is not finite."""
    T = [float(x) for x in S]
    for _ in range(GN_PASSES):
        t = []
        for k in range(3):
            r = point_terms(P3[k], uv3[k], T, K, math.inf)
            if r is None:
                return None
            t.append(r[0])
        sums = [(t[0][j] + t[1][j]) + t[2][j] for j in range(27)]
        xi = solve(sums)
        if not all(math.isfinite(x) for x in xi):
            return None
        T = left_update(xi, T)
    return T


def score(T, P, uv, K, inlier_px):
    """Inlier flags of every match at pose T (depth > 0 and squared error <=
    inlier_px^2), elementwise in point_terms' order."""
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[9]
        y = ((T[3] * X + T[4] * Y) + T[5] * Z) + T[10]
        z = ((T[6] * X + T[7] * Y) + T[8] * Z) + T[11]
        r0 = uv[:, 0] - (K[0] * x / z + K[2])
        r1 = uv[:, 1] - (K[1] * y / z + K[3])
        e2 = r0 * r0 + r1 * r1
        return (z > 0) & (e2 <= inlier_px * inlier_px)


def reloc_seed(kf_pyrs, kf_poses, points, hosts, cur_pyr, w, h, K, start, corners_x, corners_y, max_features=32768,
               hypotheses=256, max_hamming=48, ratio_permille=800, inlier_px=2.0, min_inliers=30, seed=0):
    """The whole stage.  Returns a dict: report (12,), pose (12,), matches
    (M, 3) int32, inliers (M,) uint8, per_point (n, 3), kept (n_c, 2)."""
    K = [float(x) for x in K]
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    hosts = np.asarray(hosts, np.int64).reshape(-1)
    start = np.asarray(start, np.float64).reshape(12)
    n_kf = np.asarray(kf_poses).reshape(-1, 12).shape[0]
    described, pw = map_side(kf_pyrs, kf_poses, pts, hosts, w, h, K)
    cx, cy, cw = current_side(cur_pyr, w, h, corners_x, corners_y, max_features)
    matches, per_point = match(described, pw, cw, max_hamming, ratio_permille)
    M = matches.shape[0]
    rep = np.array([0, described.sum(), cx.size, M, 0, -1, 0, -1, NAN, 0, -1, 0], np.float64)
    out = {"report": rep, "pose": start.copy(), "matches": matches, "inliers": np.zeros(M, np.uint8),
           "per_point": per_point, "kept": np.stack([cx, cy], 1).astype(np.int32)}
    if M < 3:
        rep[0] = 1
        return out
    P = pts[matches[:, 0]]
    uv = np.stack([cx[matches[:, 1]], cy[matches[:, 1]]], 1).astype(np.float64)
    Pl, uvl = P.tolist(), uv.tolist()
    cache = {}
    best_h, best_score, best_T, best_flags, solved = -1, -1, None, None, 0
    for hyp in range(hypotheses):
        tri = draw(seed, hyp, M)
        if tri not in cache:
            T = hypothesis([Pl[i] for i in tri], [uvl[i] for i in tri], start, K)
            cache[tri] = None if T is None else (T, score(T, P, uv, K, inlier_px))
        if cache[tri] is None:
            continue
        solved += 1
        T, flags = cache[tri]
        s = int(flags.sum())
        if s > best_score:
            best_h, best_score, best_T, best_flags = hyp, s, T, flags
    rep[4] = solved
    if solved:
        rep[5], rep[6] = best_h, best_score
    if not solved or best_score < min_inliers:
        rep[0] = 2
        return out
    out["inliers"] = best_flags.astype(np.uint8)
    # the inliers as an LK row over the map: uv_before = uv_after = the corner pixel
    n = pts.shape[0]
    pair_kf, succ, row_uv = np.full(n, -1, np.int32), np.zeros(n, np.uint8), np.zeros((n, 2))
    inl = matches[best_flags]
    pair_kf[inl[:, 0]] = hosts[inl[:, 0]]
    succ[inl[:, 0]] = 1
    row_uv[inl[:, 0]] = uv[best_flags]
    r = refine(pts, pair_kf, succ, row_uv, row_uv, best_T, K, REFINE_ITERATIONS, inlier_px, 1.0)
    st = int(r["report"][5])
    rep[7], rep[8], rep[9] = st, r["report"][3], r["report"][4]
    counts = np.bincount(hosts[inl[:, 0]], minlength=n_kf)
    rep[10] = int(counts.argmax())  # the first maximum: the lowest keyframe index
    out["pose"] = np.asarray(r["pose"] if st in (0, 3) else best_T, np.float64)
    out["refine"] = r
    return out
