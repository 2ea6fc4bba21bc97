"""Restatement of the warped LK alignment (viso_set_lk_warp)
in elementwise numpy fp64, in the operand order of the rule.

Vectorised over the points: every element sees the operations the rule
states, in its order (numpy's elementwise ufuncs neither reassociate nor
contract).  The 64-pixel sums follow oracle_common.hpp: ``tree_sum`` (the
ascending pairwise tree) for H, ``tree_sum_desc64`` (descending strides) for
B0, B1 and the cost.

``lk_align_warped`` returns the LK row (pair_kf, success, uv_before,
uv_after) and the warp row (A, shift, status).  ``A_override`` replaces the
computed affine map (tests: the identity pin, the thresholds); ``anchors``
replaces the keyframe choice by given (tmpl_kf, tmpl_uv); ``margins`` (a
dict) collects the smallest relative margin of every decision class, and per
point the smallest one of its `cost > lastCost` comparisons
(``cost_vs_last_per_point``; inf for a point that made none).
"""
from __future__ import annotations

import numpy as np

LEVELS = 4
SCALE = (1.0, 0.5, 0.25, 0.125)
H_STEP = 4.0
HP = 4.0
THIRD = 1.0 / 3.0


def pyr_dims(w: int, h: int):
    ws, hs, offs, off = [], [], [], 0
    for l in range(LEVELS):
        if l > 0:
            w, h = int(w * 0.5), int(h * 0.5)
        ws.append(w)
        hs.append(h)
        offs.append(off)
        off += w * h
    return ws, hs, offs


def levels(pyr: np.ndarray, w: int, h: int):
    """The four level buffers (flat uint8 views) of a pyramid."""
    ws, hs, offs = pyr_dims(w, h)
    pyr = np.ascontiguousarray(pyr, np.uint8).reshape(-1)
    return [pyr[offs[l]:offs[l] + ws[l] * hs[l]] for l in range(LEVELS)], ws, hs


def sample(buf, w, h, x, y):
    """GetPixelValue on a continuous level buffer (the project's sample_px):
    int() base, floor() weights, taps outside the buffer read 0."""
    n = w * h
    fin = (x > -1e9) & (x < 1e9) & (y > -1e9) & (y < 1e9)
    xi = np.trunc(np.where(fin, x, 0.0)).astype(np.int64)
    yi = np.trunc(np.where(fin, y, 0.0)).astype(np.int64)
    base = np.where(fin, yi * w + xi, -(1 << 40))

    def tap(i):
        ok = (i >= 0) & (i < n)
        return np.where(ok, buf[np.where(ok, i, 0)], 0).astype(np.float64)

    d0, d1, d2, d3 = tap(base), tap(base + 1), tap(base + w), tap(base + w + 1)
    xx = x - np.floor(x)
    yy = y - np.floor(y)
    return (1 - xx) * (1 - yy) * d0 + xx * (1 - yy) * d1 + (1 - xx) * yy * d2 + xx * yy * d3


def tree_sum(v):
    """oracle_common.hpp tree_sum over the last axis (64 leaves)."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def tree_sum_desc64(v):
    """oracle_common.hpp tree_sum_desc64 over the last axis."""
    s = 32
    while s >= 1:
        v = v[..., :s] + v[..., s:2 * s]
        s >>= 1
    return v[..., 0]


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def transform(pose, P):
    """R P + t, rows as mat3_vec; P (n, 3) or three arrays."""
    R = pose[:9]
    X, Y, Z = P
    return (dot3(R[0], R[1], R[2], X, Y, Z) + pose[9], dot3(R[3], R[4], R[5], X, Y, Z) + pose[10],
            dot3(R[6], R[7], R[8], X, Y, Z) + pose[11])


def project(pose, K, P):
    """project_px at level 0: (u, v, depth)."""
    x, y, z = transform(pose, P)
    return x / z * K[0] + K[2], y / z * K[1] + K[3], z


def inside(u, v, w, h):
    return (u >= 0) & (u < w) & (v >= 0) & (v < h)


def choose_kf(points, kf_poses, K, w, h):
    """lk_choose_kf: the keyframe of the smallest viewing angle among those
    the point projects into, and its projection there."""
    P = (points[:, 0], points[:, 1], points[:, 2])
    n = points.shape[0]
    best = np.full(n, 180.0)
    kf = np.full(n, -1, np.int32)
    buv = np.zeros((n, 2))
    for j, pose in enumerate(kf_poses):
        u, v, _ = project(pose, K, P)
        x, y, z = transform(pose, P)
        nrm = (x * x + y * y) + z * z
        sn = np.where(nrm > 0, np.sqrt(np.where(nrm > 0, nrm, 1.0)), 1.0)
        angle = np.abs(np.arccos(np.where(nrm > 0, z / sn, z)) / 3.14159265358979323846 * 180)
        take = inside(u, v, w, h) & ~((angle > 180.0) | (angle > best))
        best = np.where(take, angle, best)
        kf = np.where(take, j, kf).astype(np.int32)
        buv[:, 0] = np.where(take, u, buv[:, 0])
        buv[:, 1] = np.where(take, v, buv[:, 1])
    return kf, buv


def _note(margins, key, a, b, scale=None):
    """Record the smallest relative distance of a from its threshold b."""
    if margins is None:
        return
    a = np.asarray(a, np.float64)
    b = np.broadcast_to(np.asarray(b, np.float64), a.shape)
    ok = np.isfinite(a) & np.isfinite(b)
    if not ok.any():
        return
    den = np.maximum(np.abs(a[ok]), np.abs(b[ok])) if scale is None else scale
    den = np.maximum(den, 1e-300)
    m = float(np.min(np.abs(a[ok] - b[ok]) / den))
    margins[key] = min(margins.get(key, np.inf), m)


def affine(points, anchor, buv, kf_poses, cur_pose, K, uc, vc):
    """Step 2 of the rule: A (n, 4) = A00, A01, A10, A11, and the depths za,
    z(Qu), z(Qv), for the points with an anchor (anchor >= 0; others 0)."""
    kp = np.asarray(kf_poses, np.float64).reshape(-1, 12)[np.maximum(anchor, 0)].T  # (12, n)
    P = (points[:, 0], points[:, 1], points[:, 2])
    fx, fy, cx, cy = K
    za = dot3(kp[6], kp[7], kp[8], *P) + kp[11]
    out = []
    for du, dv in ((H_STEP, 0.0), (0.0, H_STEP)):
        qu = buv[:, 0] + du if du else buv[:, 0]
        qv = buv[:, 1] + dv if dv else buv[:, 1]
        d0 = (qu - cx) / fx * za - kp[9]
        d1 = (qv - cy) / fy * za - kp[10]
        d2 = za - kp[11]
        W = tuple((kp[j] * d0 + kp[3 + j] * d1) + kp[6 + j] * d2 for j in range(3))
        u, v, z = project(cur_pose, K, W)
        out.append(((u - uc) / H_STEP, (v - vc) / H_STEP, z))
    (a00, a10, zu), (a01, a11, zv) = out
    return np.stack([a00, a01, a10, a11], 1), za, zu, zv


def level_shift(D, margins=None):
    """Step 3's shift for the (accepted) area ratios D."""
    D = np.array(D, np.float64)
    shift = np.zeros(D.shape, np.int32)
    big = D > 3.0
    small = ~big & (D < THIRD)
    _note(margins, "D_vs_3", D, 3.0)
    _note(margins, "D_vs_third", D[~big], THIRD)
    for _ in range(3):
        go = big & (D > 3.0) & (shift > -3)
        shift = np.where(go, shift - 1, shift)
        D = np.where(go, D * 0.25, D)
        _note(margins, "D_vs_3", D[big & (shift > -3)], 3.0)
        go = small & (D < THIRD) & (shift < 3)
        shift = np.where(go, shift + 1, shift)
        D = np.where(go, D * 4.0, D)
        _note(margins, "D_vs_third", D[small & (shift < 3)], THIRD)
    return shift


def lk_align_warped(kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, points, thresh=14400.0, max_area_ratio=64.0,
                    anchors=None, A_override=None, margins=None):
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    kf_poses = np.ascontiguousarray(kf_poses, np.float64).reshape(-1, 12)
    cur_pose = np.ascontiguousarray(cur_pose, np.float64).reshape(12)
    K = [float(k) for k in K]
    n = points.shape[0]
    res = dict(pair_kf=np.full(n, -1, np.int32), success=np.zeros(n, np.uint8), uv_before=np.zeros((n, 2)),
               uv_after=np.zeros((n, 2)), A=np.zeros((n, 4)), shift=np.zeros(n, np.int8),
               status=np.ones(n, np.uint8))
    if n == 0:
        return res
    with np.errstate(all="ignore"):
        _align(res, kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, points, float(thresh), float(max_area_ratio),
               anchors, A_override, margins)
    return res


def _align(res, kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, points, thresh, ratio, anchors, A_override, margins):
    n = points.shape[0]
    P = (points[:, 0], points[:, 1], points[:, 2])
    uc, vc, _ = project(cur_pose, K, P)
    view = inside(uc, vc, w, h)
    if anchors is None:
        akf, buv = choose_kf(points, kf_poses, K, w, h)
    else:
        akf = np.asarray(anchors[0], np.int32).reshape(-1)
        buv = np.asarray(anchors[1], np.float64).reshape(-1, 2)
    paired = view & (akf >= 0)
    res["pair_kf"][:] = np.where(paired, akf, -1)
    res["uv_before"][paired, 0] = uc[paired]
    res["uv_before"][paired, 1] = vc[paired]
    res["uv_after"][:] = res["uv_before"]
    A, za, zu, zv = affine(points, akf, buv, kf_poses, cur_pose, K, uc, vc)
    if A_override is not None:
        A = np.broadcast_to(np.asarray(A_override, np.float64).reshape(-1, 4), (n, 4)).copy()
    A[~paired] = 0.0
    res["A"][:] = A
    a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    det = a00 * a11 - a01 * a10
    D = np.abs(det)
    lo = 1.0 / ratio
    ok = paired & (za > 0) & (zu > 0) & (zv > 0) & np.isfinite(A).all(1) & (lo <= D) & (D <= ratio)
    geo = paired & (za > 0) & (zu > 0) & (zv > 0) & np.isfinite(A).all(1)
    _note(margins, "D_vs_ratio", D[geo], ratio)
    _note(margins, "D_vs_ratio", D[geo], lo)
    res["status"][paired & ~ok] = 2
    idx = np.nonzero(ok)[0]
    if idx.size == 0:
        return
    shift = np.zeros(n, np.int32)
    shift[idx] = level_shift(D[idx], margins)
    res["shift"][:] = shift
    ai00, ai01, ai10, ai11 = a11[idx] / det[idx], (-a01[idx]) / det[idx], (-a10[idx]) / det[idx], a00[idx] / det[idx]
    cur_l, ws, hs = levels(cur_pyr, w, h)
    kf_l = [levels(k, w, h)[0] for k in kf_pyrs]
    m = idx.size
    lane = np.arange(64)
    px = ((lane >> 3) - 4).astype(np.float64)[None, :]
    py = ((lane & 7) - 4).astype(np.float64)[None, :]
    bu, bv = buv[idx, 0][:, None], buv[idx, 1][:, None]
    kfi = akf[idx]
    cu, cv = uc[idx].copy(), vc[idx].copy()
    succ = np.zeros(m, bool)
    skipped = np.zeros(m, np.int32)
    cost_margin = np.full(m, np.inf)  # per point: the smallest relative | cost - lastCost | it compared
    sh = shift[idx]
    c = lambda v: v[:, None]
    for level in range(LEVELS - 1, -1, -1):
        s = SCALE[level]
        r = np.clip(level + sh, 0, LEVELS - 1)
        sr = np.array(SCALE)[r]
        k = c(sr / s)
        x = bu * c(sr) + ((c(ai00) * px + c(ai01) * py) * k)
        y = bv * c(sr) + ((c(ai10) * px + c(ai11) * py) * k)
        ex0, ex1, ey0, ey1 = c(ai00) * k, c(ai10) * k, c(ai01) * k, c(ai11) * k
        xs = [x, x + ex0, x - ex0, x + ey0, x - ey0]
        ys = [y, y + ex1, y - ex1, y + ey1, y - ey1]
        wr, hr = c(np.array(ws)[r].astype(np.float64)), c(np.array(hs)[r].astype(np.float64))
        valid = np.ones(m, bool)
        vm = np.full(m, np.inf)
        for X, Y in zip(xs, ys):
            valid &= ((0 <= X) & (X + 1 < wr) & (0 <= Y) & (Y + 1 < hr)).all(1)
            vm = np.minimum(vm, np.min(np.minimum(np.minimum(np.abs(X), np.abs(wr - (X + 1))),
                                                  np.minimum(np.abs(Y), np.abs(hr - (Y + 1)))), 1))
        if margins is not None and m:
            margins["template_valid_px"] = min(margins.get("template_valid_px", np.inf), float(np.nanmin(vm)))
        skipped += ~valid
        succ[~valid] = False
        # the templates, per (anchor keyframe, reference level) group
        I1 = np.zeros((m, 64))
        J0 = np.zeros((m, 64))
        J1 = np.zeros((m, 64))
        for j in np.unique(kfi[valid]):
            for rl in np.unique(r[valid & (kfi == j)]):
                g = np.nonzero(valid & (kfi == j) & (r == rl))[0]
                buf, gw, gh = kf_l[j][rl], ws[rl], hs[rl]
                smp = [sample(buf, gw, gh, X[g], Y[g]) for X, Y in zip(xs, ys)]
                I1[g] = smp[0]
                J0[g] = -0.5 * (smp[1] - smp[2])
                J1[g] = -0.5 * (smp[3] - smp[4])
        v = np.nonzero(valid)[0]
        if v.size == 0:
            continue
        H00, H01, H11 = tree_sum(J0[v] * J0[v]), tree_sum(J0[v] * J1[v]), tree_sum(J1[v] * J1[v])
        H10 = H01
        invdet = 1.0 / (H00 * H11 - H10 * H01)
        ih = (H11 * invdet, -H01 * invdet, -H10 * invdet, H00 * invdet)  # i00, i01, i10, i11
        dx, dy, sc, pm = _iterate(I1[v], J0[v], J1[v], ih, cur_l[level], ws[level], hs[level], cu[v] * s, cv[v] * s,
                                  px, py, thresh, margins)
        succ[v] = sc
        cost_margin[v] = np.minimum(cost_margin[v], pm)
        cu[v] = cu[v] + dx / s
        cv[v] = cv[v] + dy / s
    res["success"][idx] = succ
    res["uv_after"][idx, 0] = cu
    res["uv_after"][idx, 1] = cv
    res["status"][idx] = (skipped << 4).astype(np.uint8)
    if margins is not None:
        per_point = np.full(n, np.inf)
        per_point[idx] = cost_margin
        margins["cost_vs_last_per_point"] = per_point


def _iterate(I1, J0, J1, ih, cur, w, h, bx, by, px, py, thresh, margins):
    """lk_iterate<100, false> for every point of the level: bx, by the
    current coordinates at this level (bounds test and sample base)."""
    m = I1.shape[0]
    i00, i01, i10, i11 = ih
    dx, dy = np.zeros(m), np.zeros(m)
    last = np.zeros(m)
    succ = np.ones(m, bool)
    pm = np.full(m, np.inf)
    act = np.arange(m)
    cx, cy = bx[:, None] + px, by[:, None] + py
    for it in range(100):
        if act.size == 0:
            break
        qx, qy = bx[act] + dx[act], by[act] + dy[act]
        q = np.stack([qx + -HP, qy + -HP, qx + HP, qy + HP], 1)
        lim = np.array([w, h, w, h], np.float64)[None, :]
        out = ~((q >= 0) & (q < lim)).all(1)
        if margins is not None:
            fin = np.isfinite(q)
            if fin.any():
                d = np.minimum(np.abs(q), np.abs(lim - q))[fin]
                margins["bounds_px"] = min(margins.get("bounds_px", np.inf), float(d.min()))
        succ[act[out]] = False
        act = act[~out]
        if act.size == 0:
            break
        smp = sample(cur, w, h, cx[act] + dx[act][:, None], cy[act] + dy[act][:, None])
        e = I1[act] - smp
        B0, B1 = tree_sum_desc64(-J0[act] * e), tree_sum_desc64(-J1[act] * e)
        cost = tree_sum_desc64(e * e)
        u0 = i00[act] * B0 + i01[act] * B1
        u1 = i10[act] * B0 + i11[act] * B1
        nan = np.isnan(u0)
        succ[act[nan]] = False
        worse = ~nan & (cost > last[act]) if it > 0 else np.zeros(act.size, bool)
        if it > 0:
            _note(margins, "cost_vs_last", cost[~nan], last[act][~nan])
            a, b = cost[~nan], last[act][~nan]
            pm[act[~nan]] = np.minimum(pm[act[~nan]], np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300))
        go = ~nan & ~worse
        g = act[go]
        dx[g] += u0[go]
        dy[g] += u1[go]
        last[g] = cost[go]
        succ[g] = ~(cost[go] > thresh)
        _note(margins, "last_vs_thresh", cost[go], thresh)
        act = g
    return dx, dy, succ, pm
