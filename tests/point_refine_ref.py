"""TEST INFRASTRUCTURE ONLY — Python restatement of the point refinement
(viso_set_point_refine / viso_point_obs_record / viso_points_refine,
include/viso/viso_c.h; DESIGN.md §Point refinement).  The repo's own spec: the
reference computes every map point's aligned position in every tracking frame
(LKAlignment, src/viso.cpp:768-843) and only draws it; its map points
(src/viso.cpp:79-96) keep the coordinates of their creation.

A point's LK template is its anchor keyframe's patch at the point's projection
there, so the aligned positions measure the depth along the ray from the
anchor's centre C through the point; the refinement moves P = C + D to
C + D / (1 + delta) and nothing else.

Every expression is elementwise numpy fp64 arithmetic in the device's operand
order, that of tests/point_cull_ref.py: a 3-term dot product is
(a0 b0 + a1 b1) + a2 b2, nothing is contracted (every product and sum is a
ufunc call of its own), and the three sums of a pass are the pairwise tree over
the ring's slots 0..7, ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), an
absent, unflagged or skipped slot contributing +0.0.  Poses are Tcw, 12 doubles
(R row-major, t): Pc = R Pw + t.

Statuses: 0 all passes run, 1 too few observations, 2 the step is not finite
or leaves (0.5, 2), 3 the cost stopped falling (the previous point is kept),
4 too little parallax against the anchor, 5 no anchor.
"""
from __future__ import annotations

import numpy as np

SLOTS = 8


def tree8(v):
    """The canonical sum of 8 slot rows (8, n)."""
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))


def record(pair_kf, success, uv_before, uv_after, max_shift_px):
    """One frame's record: (valid (n,) uint8, uv (n, 2) = uv_after, margin:
    the smallest | |d|^2 - max_shift_px^2 | over the paired, successful
    points (inf: none))."""
    pk = np.asarray(pair_kf).reshape(-1)
    sc = np.asarray(success).reshape(-1)
    ub = np.asarray(uv_before, np.float64).reshape(-1, 2)
    ua = np.asarray(uv_after, np.float64).reshape(-1, 2)
    s2 = float(max_shift_px) * float(max_shift_px)
    with np.errstate(invalid="ignore", over="ignore"):
        d0 = ua[:, 0] - ub[:, 0]
        d1 = ua[:, 1] - ub[:, 1]
        d2 = d0 * d0 + d1 * d1
        within = d2 <= s2
    cand = (pk >= 0) & (sc != 0)
    margin = float(np.abs(d2[cand] - s2).min()) if cand.any() else float("inf")
    return (cand & within).astype(np.uint8), ua.copy(), margin


def centres(kf_poses):
    """C = -R^T t of every keyframe pose, (k, 3)."""
    A = np.asarray(kf_poses, np.float64).reshape(-1, 12)
    return np.stack([-((A[:, j] * A[:, 9] + A[:, 3 + j] * A[:, 10]) + A[:, 6 + j] * A[:, 11]) for j in range(3)], 1)


def anchors(points, kf_poses, K, w, h):
    """The LK templates' keyframe choice (lk_template_kernel; LKAlignment,
    src/viso.cpp:774-800): among the keyframes a point projects into, the one
    with the smallest viewing angle, the later of equals; -1: none.  Returns
    (anchor (n,) int32, margin): the smallest distance in pixels of a
    projection from the image border and in degrees between the chosen angle
    and another keyframe's."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    A = np.asarray(kf_poses, np.float64).reshape(-1, 12)
    fx, fy, cx, cy = (float(k) for k in K)
    n = len(P)
    best = np.full(n, 180.0)
    kf = np.full(n, -1, np.int32)
    margin = float("inf")
    angles = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j, T in enumerate(A):
            x = ((T[0] * P[:, 0] + T[1] * P[:, 1]) + T[2] * P[:, 2]) + T[9]
            y = ((T[3] * P[:, 0] + T[4] * P[:, 1]) + T[5] * P[:, 2]) + T[10]
            z = ((T[6] * P[:, 0] + T[7] * P[:, 1]) + T[8] * P[:, 2]) + T[11]
            u = (x / z) * fx + cx
            v = (y / z) * fy + cy
            inside = (u >= 0) & (u < w) & (v >= 0) & (v < h)
            for d in (u, u - w, v, v - h):
                d = np.abs(d[np.isfinite(d)])
                if d.size:
                    margin = min(margin, float(d.min()))
            nrm = (x * x + y * y) + z * z
            sn = np.sqrt(nrm)
            cz = np.where(nrm > 0, z / sn, z)
            ang = np.abs(np.arccos(cz) / 3.14159265358979323846 * 180)
            take = inside & ~((ang > 180.0) | (ang > best))
            angles.append(np.where(inside, ang, np.inf))
            best = np.where(take, ang, best)
            kf = np.where(take, j, kf).astype(np.int32)
    if len(A) > 1 and n:
        a = np.sort(np.stack(angles), 0)
        gap = (a[1] - a[0])[np.isfinite(a[1])]
        if gap.size:
            margin = min(margin, float(gap.min()))
    return kf, margin


class Margins:
    """The smallest distance of any decision from its threshold: z (Pc.z
    against 0), huber (e against huber_px), parallax (H max_rel_sigma^2
    against 1, relative), cost (cost_k against cost_{k-1}, relative), step
    (1 + delta against 0.5 and 2)."""

    def __init__(self):
        self.z = self.huber = self.parallax = self.cost = self.step = float("inf")

    def note(self, name, values):
        v = np.asarray(values, np.float64)
        v = v[np.isfinite(v)]
        if v.size:
            setattr(self, name, min(getattr(self, name), float(np.abs(v).min())))

    def smallest(self):
        return min(self.z, self.huber, self.parallax, self.cost, self.step)

    def __repr__(self):
        return "Margins(z=%.3g huber=%.3g parallax=%.3g cost=%.3g step=%.3g)" % (
            self.z, self.huber, self.parallax, self.cost, self.step)


def refine(points, anchor_kf, kf_poses, frame_poses, obs_valid, obs_uv, K, iterations, huber_px, min_obs,
           max_rel_sigma):
    """One refinement.  points (n, 3), anchor_kf (n,), kf_poses (k, 12),
    frame_poses (m, 12): the live slots, obs_valid (m, n), obs_uv (m, n, 2).
    Returns a dict: points (n, 3) (a new array), status, steps (n,) uint8,
    costs (n, 2): cost_0 and the cost at the result (0 where no pass ran),
    counts [eligible, moved, status 4, status 2], delta0 (n,): the first step
    (NaN where none was computed), margins (Margins)."""
    P = np.array(points, np.float64).reshape(-1, 3)
    n = P.shape[0]
    an = np.asarray(anchor_kf, np.int64).reshape(-1)
    kfp = np.asarray(kf_poses, np.float64).reshape(-1, 12)
    fp = np.asarray(frame_poses, np.float64).reshape(-1, 12)
    m = fp.shape[0]
    valid = np.asarray(obs_valid).reshape(m, n) != 0
    uv = np.asarray(obs_uv, np.float64).reshape(m, n, 2)
    assert 1 <= m <= SLOTS and len(an) == n
    fx, fy, cx, cy = (float(k) for k in K)
    hub, sig2 = float(huber_px), float(max_rel_sigma) * float(max_rel_sigma)
    iterations, min_obs = int(iterations), int(min_obs)
    mg = Margins()

    status = np.full(n, -1, np.int64)
    steps = np.zeros(n, np.int64)
    costs = np.zeros((n, 2), np.float64)
    delta0 = np.full(n, np.nan)
    anchored = (an >= 0) & (an < len(kfp))
    status[~anchored] = 5
    C = centres(kfp)[np.where(anchored, an, 0)]
    n_obs = valid.sum(0)
    eligible = anchored & (n_obs >= min_obs)
    status[anchored & ~eligible] = 1

    Pk = P.copy()      # P_k of the live points
    Pprev = P.copy()   # P_{k-1}
    cost_prev = np.zeros(n)
    live = eligible.copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(iterations + 1):
            if not live.any():
                break
            D = Pk - C
            hs, bs, cs = np.zeros((SLOTS, n)), np.zeros((SLOTS, n)), np.zeros((SLOTS, n))
            used = np.zeros(n, np.int64)
            for s in range(m):
                T = fp[s]
                x = ((T[0] * Pk[:, 0] + T[1] * Pk[:, 1]) + T[2] * Pk[:, 2]) + T[9]
                y = ((T[3] * Pk[:, 0] + T[4] * Pk[:, 1]) + T[5] * Pk[:, 2]) + T[10]
                z = ((T[6] * Pk[:, 0] + T[7] * Pk[:, 1]) + T[8] * Pk[:, 2]) + T[11]
                seen = live & valid[s]
                ok = seen & (z > 0)
                mg.note("z", z[seen])
                Dc0 = (T[0] * D[:, 0] + T[1] * D[:, 1]) + T[2] * D[:, 2]
                Dc1 = (T[3] * D[:, 0] + T[4] * D[:, 1]) + T[5] * D[:, 2]
                Dc2 = (T[6] * D[:, 0] + T[7] * D[:, 1]) + T[8] * D[:, 2]
                r0 = uv[s, :, 0] - (fx * x / z + cx)
                r1 = uv[s, :, 1] - (fy * y / z + cy)
                e2 = r0 * r0 + r1 * r1
                e = np.sqrt(e2)
                mg.note("huber", (e - hub)[ok])
                inl = e <= hub
                w = np.where(inl, 1.0, hub / e)
                rho = np.where(inl, 0.5 * e2, hub * (e - 0.5 * hub))
                g0 = fx * (x * Dc2 / (z * z) - Dc0 / z)
                g1 = fy * (y * Dc2 / (z * z) - Dc1 / z)
                hs[s] = np.where(ok, w * (g0 * g0 + g1 * g1), 0.0)
                bs[s] = np.where(ok, w * (g0 * r0 + g1 * r1), 0.0)
                cs[s] = np.where(ok, rho, 0.0)
                used += ok
            H, b, cost = tree8(hs), tree8(bs), tree8(cs)
            if k == 0:
                costs[live, 0] = cost[live]
                costs[live, 1] = cost[live]
                few = live & (used < min_obs)
                status[few] = 1
                live &= ~few
                mg.note("parallax", (H * sig2 - 1.0)[live])
                flat = live & (H * sig2 < 1.0)
                status[flat] = 4
                live &= ~flat
            else:
                mg.note("cost", ((cost - cost_prev) / cost_prev)[live & (cost_prev > 0)])
                worse = live & (cost >= cost_prev)
                status[worse] = 3
                steps[worse] = k - 1
                Pk[worse] = Pprev[worse]
                costs[worse, 1] = cost_prev[worse]
                live &= ~worse
            steps[live] = k
            costs[live, 1] = cost[live]
            if k == iterations:
                status[live] = 0
                break
            delta = b / H
            q = 1.0 + delta
            if k == 0:
                delta0[live] = delta[live]
            mg.note("step", np.concatenate([(q - 0.5)[live], (q - 2.0)[live]]))
            bad = live & ~(np.isfinite(delta) & (0.5 < q) & (q < 2.0))
            status[bad] = 2
            live &= ~bad
            cost_prev = np.where(live, cost, cost_prev)
            Pprev[live] = Pk[live]
            Pk[live] = (C + D / q[:, None])[live]
    assert (status >= 0).all()
    out = np.where((steps >= 1)[:, None], Pk, P)
    counts = [int(eligible.sum()), int((steps >= 1).sum()), int((status == 4).sum()), int((status == 2).sum())]
    return {"points": out, "status": status.astype(np.uint8), "steps": steps.astype(np.uint8), "costs": costs,
            "counts": counts, "delta0": delta0, "margins": mg}


class Ring:
    """The observation ring carried along a run (the frame path's state)."""

    def __init__(self, window, max_shift_px):
        self.window, self.shift = int(window), float(max_shift_px)
        self.reset()

    def reset(self):
        self.count = 0
        self.poses, self.valid, self.uv = [None] * self.window, [None] * self.window, [None] * self.window
        self.margin = float("inf")

    def record(self, row, pose):
        pk, sc, ub, ua = row
        v, uv, mg = record(pk, sc, ub, ua, self.shift)
        s = self.count % self.window
        self.poses[s], self.valid[s], self.uv[s] = np.asarray(pose, np.float64).reshape(12).copy(), v, uv
        self.count += 1
        self.margin = min(self.margin, mg)

    def live(self):
        m = min(self.count, self.window)
        return np.stack(self.poses[:m]), np.stack(self.valid[:m]), np.stack(self.uv[:m])
