"""TEST INFRASTRUCTURE ONLY — numpy restatement of the keyframe alignment
(viso_kf_align, include/viso/viso_c.h): the recovery of a lost
pose by an iterated photometric Gauss-Newton from each keyframe to the current
frame.  The repo's own spec; the per-point arithmetic is the direct pose's
(oracle_track.cpp direct_point_partials, the factored tree form).

Elementwise numpy fp64 over the points of a pass (numpy's ufuncs neither
reassociate nor contract), scalar Python floats for the decisions, in the
operand order of the rule.  The sums: per point the six pixel sums by
``tree_sum_desc64``; across points, list position p adds its 28 terms to
accumulator p mod 16 in ascending p, and the 16 accumulators are added
neighbours first (0+1, 2+3, ...).

``margins`` (a dict) collects the smallest distance of every kind of decision
from its threshold: sees_px / good_px (pixels to an image border), z (a depth
to 0), cost_b (|cost_j - cost_{j-1}| / cost_{j-1}), cost_c (|1 - cost_j /
cost_{j-1} - 0.005|), max_cost (|cost - max_cost| / max_cost at the result)
and winner (the relative gap between the two best accepted costs).
"""
from __future__ import annotations

import math

import numpy as np

from tests.lk_warp_ref import SCALE, levels, project, sample, tree_sum_desc64
from tests.pose_refine_ref import left_update, solve

N_ACC = 16
N_TERMS = 28  # H upper triangle (21, row-major), b (6), cost
DELTA_THRESH = 0.005
HP = 4.0
NAN = float("nan")

_LANE = np.arange(64)
_PX = ((_LANE >> 3) - 4).astype(np.float64)[None, :]  # x outer
_PY = ((_LANE & 7) - 4).astype(np.float64)[None, :]   # y inner


def _note(margins, key, d):
    if margins is None:
        return
    d = np.asarray(d, np.float64)
    d = d[np.isfinite(d)]
    if d.size:
        margins[key] = min(margins.get(key, np.inf), float(d.min()))


def _inside(u, v, w, h):
    return (u >= 0) & (u < w) & (v >= 0) & (v < h)


def _border(u, v, w, h):
    return np.minimum(np.minimum(np.abs(u), np.abs(u - w)), np.minimum(np.abs(v), np.abs(v - h)))


def select_points(points, kf_pose, K, w, h, max_points, margins=None):
    """Step 1: the indices of the first max_points map points keyframe k sees
    (depth > 0 and the level-0 projection inside the image), in map order."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    if pts.shape[0] == 0:
        return np.zeros(0, np.int64)
    with np.errstate(all="ignore"):
        u, v, z = project(kf_pose, K, (pts[:, 0], pts[:, 1], pts[:, 2]))
        sees = (z > 0) & _inside(u, v, w, h)
        _note(margins, "z", np.abs(z))
        _note(margins, "sees_px", _border(u, v, w, h)[z > 0])
    return np.nonzero(sees)[0][:max_points]


def d_pixel_d_xi(T, K, P, scale):
    """dPixeldXi (oracle_track.cpp d_pixel_d_xi) for the points P at pose T:
    two lists of six arrays (rows u and v)."""
    X, Y, Z = P
    x = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[9]
    y = ((T[3] * X + T[4] * Y) + T[5] * Z) + T[10]
    z = ((T[6] * X + T[7] * Y) + T[8] * Z) + T[11]
    fx, fy = K[0] * scale, K[1] * scale
    zz, xy = z * z, x * y
    zero = np.zeros_like(z)
    J0 = [fx / z, zero, -fx * x / zz, -fx * xy / zz, fx + fx * x * x / zz, -fx * y / z]
    J1 = [zero, fy / z, -fy * y / zz, -fy - fy * y * y / zz, fy * xy / zz, fy * x / z]
    return J0, J1


def point_terms(kf_buf, cur_buf, w, h, kf_pose, T, K, P, level, margins=None):
    """One pass's per-point part at pyramid level `level` (buffers and size of
    that level): good (m,) and the 28 terms (m, 28), zero where not good."""
    s = SCALE[level]
    with np.errstate(all="ignore"):
        u0, v0, zr = project(kf_pose, K, P)
        u1, v1, zc = project(T, K, P)
        ur, vr, uc, vc = s * u0, s * v0, s * u1, s * v1
        good = (_inside(ur - HP, vr - HP, w, h) & _inside(ur + HP, vr + HP, w, h) &
                _inside(uc - HP, vc - HP, w, h) & _inside(uc + HP, vc + HP, w, h) & (zr > 0) & (zc > 0))
        if margins is not None:
            _note(margins, "z", np.abs(zc))
            front = (zr > 0) & (zc > 0)
            for u, v in ((ur, vr), (uc, vc)):
                _note(margins, "good_px", np.minimum(_border(u - HP, v - HP, w, h), _border(u + HP, v + HP, w, h))[front])
        m = good.shape[0]
        terms = np.zeros((m, N_TERMS))
        g = np.nonzero(good)[0]
        if g.size == 0:
            return good, terms
        Pg = tuple(c[g] for c in P)
        J0, J1 = d_pixel_d_xi(T, K, Pg, s)
        c = lambda a: a[g][:, None]
        xr, yr = c(ur) + _PX, c(vr) + _PY
        xc, yc = c(uc) + _PX, c(vc) + _PY
        err = sample(kf_buf, w, h, xr, yr) - sample(cur_buf, w, h, xc, yc)
        g0 = 0.5 * (sample(cur_buf, w, h, xc + 1, yc) - sample(cur_buf, w, h, xc - 1, yc))
        g1 = 0.5 * (sample(cur_buf, w, h, xc, yc + 1) - sample(cur_buf, w, h, xc, yc - 1))
        G = [tree_sum_desc64(v) for v in (g0 * g0, g0 * g1, g1 * g1, err * g0, err * g1, err * err)]
        k = 0
        for a in range(6):
            for b in range(a, 6):
                terms[g, k] = (G[0] * (J0[a] * J0[b]) + G[1] * (J0[a] * J1[b] + J1[a] * J0[b])) + G[2] * (J1[a] * J1[b])
                k += 1
        for a in range(6):
            terms[g, 21 + a] = G[3] * J0[a] + G[4] * J1[a]
        terms[g, 27] = G[5]
    return good, terms


def pass_sums(good, terms):
    """(S[28], n): list position p into accumulator p mod 16 in ascending p,
    then the neighbour-pairs tree over the accumulators."""
    m = good.shape[0]
    acc = np.zeros((N_ACC, N_TERMS))
    with np.errstate(all="ignore"):
        for r in range(0, m, N_ACC):
            blk = terms[r:r + N_ACC]
            acc[:blk.shape[0]] = acc[:blk.shape[0]] + blk  # a point that is not good adds +0.0
        v = acc
        while v.shape[0] > 1:
            v = v[0::2] + v[1::2]
    return [float(x) for x in v[0]], int(good.sum())


def align_level(kf_buf, cur_buf, w, h, kf_pose, T0, K, P, level, iterations, margins=None, trace=None):
    """One level: (kept pose, exit, steps applied, n, cost)."""
    T = [float(x) for x in T0]
    prev = None  # (pose, n, cost) of pass j - 1
    j = 0
    while True:
        good, terms = point_terms(kf_buf, cur_buf, w, h, kf_pose, T, K, P, level, margins)
        S, n = pass_sums(good, terms)
        with np.errstate(all="ignore"):
            cost = float(np.float64(S[27]) / np.float64(n))
        if trace is not None:
            trace.append((level, j, n, cost))
        if n < 6 or not math.isfinite(cost):
            if j == 0:
                return T, 4, 0, n, NAN
            return prev[0], 5, j - 1, prev[1], prev[2]
        if j >= 1:
            if margins is not None:
                _note(margins, "cost_b", abs(cost - prev[2]) / prev[2])
                _note(margins, "cost_c", abs((1 - cost / prev[2]) - DELTA_THRESH))
            if cost >= prev[2]:
                return prev[0], 1, j - 1, prev[1], prev[2]
            if (1 - cost / prev[2]) < DELTA_THRESH:
                return T, 2, j, n, cost
        if j == iterations:
            return T, 0, j, n, cost
        xi = solve(S)
        if not all(math.isfinite(x) for x in xi):
            return T, 3, j, n, cost
        prev = (T, n, cost)
        T = left_update(xi, T)
        j += 1


def align_candidate(kf_pyr, kf_pose, cur_pyr, w, h, K, points, seed, iterations, max_points, max_cost,
                    min_good_permille, margins=None, trace=None):
    """One candidate: (pose (12,), report (20,))."""
    K = [float(x) for x in K]
    kf_pose = np.asarray(kf_pose, np.float64).reshape(12)
    seed = [float(x) for x in np.asarray(seed, np.float64).reshape(12)]
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    idx = select_points(pts, kf_pose, K, w, h, max_points, margins)
    m = int(idx.size)
    rep = np.full(20, NAN)
    rep[1] = m
    if m < 6:
        rep[0], rep[2] = 1, 0
        for q in range(4):
            rep[4 + 4 * q:7 + 4 * q] = (-1, 0, 0)
        return np.array(seed), rep
    P = (pts[idx, 0], pts[idx, 1], pts[idx, 2])
    kl, ws, hs = levels(kf_pyr, w, h)
    cl, _, _ = levels(cur_pyr, w, h)
    T = seed
    for q, level in enumerate((3, 2, 1, 0)):
        T, ex, steps, n, cost = align_level(kl[level], cl[level], ws[level], hs[level], kf_pose, T, K, P, level,
                                            iterations, margins, trace)
        rep[4 + 4 * q:8 + 4 * q] = (ex, steps, n, cost)
    rep[2], rep[3] = n, cost
    if ex == 4:
        rep[0] = 2
    elif n * 1000 < min_good_permille * m:
        rep[0] = 3
    elif not (cost <= max_cost):
        rep[0] = 4
    else:
        rep[0] = 0
    if margins is not None and ex != 4:
        _note(margins, "max_cost", abs(cost - max_cost) / max_cost)
    return np.array(T, np.float64), rep


def pick_winner(report, margins=None):
    """The accepted candidate of least cost, ties to the lowest index; -1."""
    best, second, win = math.inf, math.inf, -1
    for c, r in enumerate(report):
        if r[0] != 0:
            continue
        if r[3] < best:
            best, second, win = float(r[3]), best, c
        elif r[3] < second:
            second = float(r[3])
    if margins is not None and math.isfinite(second):
        _note(margins, "winner", (second - best) / second)
    return win


def kf_align(kf_pyrs, kf_poses, cur_pyr, w, h, K, points, extra_seed=None, iterations=10, max_points=512,
             max_cost=57600.0, min_good_permille=500, margins=None, trace=None):
    """viso_kf_align: dict(poses (n_cand, 12), report (n_cand, 20), winner).
    Candidate (1 + n_extra) k + s: keyframe k from its own pose (s = 0) or
    from the extra seed (s = 1)."""
    kf_poses = np.asarray(kf_poses, np.float64).reshape(-1, 12)
    seeds = [None] if extra_seed is None else [None, np.asarray(extra_seed, np.float64).reshape(12)]
    poses, reps = [], []
    for k in range(kf_poses.shape[0]):
        for s in seeds:
            tr = None if trace is None else []
            pose, rep = align_candidate(kf_pyrs[k], kf_poses[k], cur_pyr, w, h, K, points,
                                        kf_poses[k] if s is None else s, iterations, max_points, max_cost,
                                        min_good_permille, margins, tr)
            if trace is not None:
                trace.append(tr)
            poses.append(pose)
            reps.append(rep)
    report = np.array(reps).reshape(-1, 20)
    return {"poses": np.array(poses).reshape(-1, 12), "report": report, "winner": pick_winner(report, margins)}
