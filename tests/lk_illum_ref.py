"""Restatement of the illumination-invariant LK alignment (viso_set_lk_illum;
DESIGN.md §24) in elementwise numpy fp64, in the operand order of the rule,
over the helpers of tests/lk_warp_ref.py (§17's geometry, template sampling
and sums are unchanged).

Per level the Jacobian is projected off span{1, T}; per iteration five
descending-tree sums give B, and the projected residual's energy by
subtraction; after level 0 the gain is bounded.

``lk_align_illum`` returns lk_warp_ref's rows plus ``gain_offset`` (n, 2): the
last accepted level-0 iteration's pair, NaN where there was none.  With
``mode=0`` it calls through to ``lk_warp_ref.lk_align_warped`` unchanged (no
``gain_offset`` row).  ``margins`` (a dict) collects, per point,
``flag_margin``: the smallest relative margin of its flag-changing decisions
(lastCost against thresh, the gain against its bounds, stt against 64, D's
thresholds, the bounds test and the template validity, the last two in
pixels over the image's larger side), and ``cost_ties``: how many of its
`cost > lastCost` comparisons were within 1e-9 relative.
"""
from __future__ import annotations

import numpy as np

from tests import lk_warp_ref as lk
from tests.lk_warp_ref import HP, LEVELS, SCALE, THIRD, sample, tree_sum, tree_sum_desc64

STT_MIN = 64.0
INV64 = 1.0 / 64.0


def project_out(T, J0, J1):
    """Steps 1 and 3 of the rule for (m, 64) arrays: m, Tc, stt, P0, P1."""
    c = lambda v: v[:, None]
    m = tree_sum(T) * INV64
    Tc = T - c(m)
    stt = tree_sum(Tc * Tc)
    P = []
    for J in (J0, J1):
        a = tree_sum(J) * INV64
        cc = tree_sum(Tc * J) / stt
        P.append((J - c(a)) - c(cc) * Tc)
    return m, Tc, stt, P[0], P[1]


def iteration_sums(T, Tc, P0, P1, stt, smp):
    """One iteration's five sums and the cost: (B0, B1, see, se, ste, cost)."""
    e = T - smp
    B0, B1 = tree_sum_desc64(-P0 * e), tree_sum_desc64(-P1 * e)
    see, se, ste = tree_sum_desc64(e * e), tree_sum_desc64(e), tree_sum_desc64(Tc * e)
    cost = (see - (se * se) * INV64) - (ste * ste) / stt
    return B0, B1, see, se, ste, cost


def gain_offset(m, stt, se, ste):
    gain = 1.0 - ste / stt
    return gain, (m - se * INV64) - gain * m


def _rel(a, b):
    """Relative distance of a from its threshold b (inf where not finite)."""
    a = np.asarray(a, np.float64)
    b = np.broadcast_to(np.asarray(b, np.float64), a.shape)
    ok = np.isfinite(a) & np.isfinite(b)
    out = np.full(a.shape, np.inf)
    den = np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    out[ok] = (np.abs(a - b) / den)[ok]
    return out


def lk_align_illum(kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, points, thresh=14400.0, max_area_ratio=64.0,
                   mode=1, max_gain=4.0, anchors=None, A_override=None, margins=None):
    if not mode:
        return lk.lk_align_warped(kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, points, thresh=thresh,
                                  max_area_ratio=max_area_ratio, anchors=anchors, A_override=A_override,
                                  margins=margins)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    kf_poses = np.ascontiguousarray(kf_poses, np.float64).reshape(-1, 12)
    cur_pose = np.ascontiguousarray(cur_pose, np.float64).reshape(12)
    K = [float(k) for k in K]
    n = points.shape[0]
    res = dict(pair_kf=np.full(n, -1, np.int32), success=np.zeros(n, np.uint8), uv_before=np.zeros((n, 2)),
               uv_after=np.zeros((n, 2)), A=np.zeros((n, 4)), shift=np.zeros(n, np.int8),
               status=np.ones(n, np.uint8), gain_offset=np.full((n, 2), np.nan))
    if margins is not None:
        margins["flag_margin"] = np.full(n, np.inf)
        margins["cost_ties"] = np.zeros(n, np.int64)
    if n == 0:
        return res
    with np.errstate(all="ignore"):
        _align(res, kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, points, float(thresh), float(max_area_ratio),
               float(max_gain), anchors, A_override, margins)
    return res


def _align(res, kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, points, thresh, ratio, max_gain, anchors, A_override,
           margins):
    n = points.shape[0]
    side = float(max(w, h))
    fm = margins["flag_margin"] if margins is not None else None
    P = (points[:, 0], points[:, 1], points[:, 2])
    uc, vc, _ = lk.project(cur_pose, K, P)
    view = lk.inside(uc, vc, w, h)
    if anchors is None:
        akf, buv = lk.choose_kf(points, kf_poses, K, w, h)
    else:
        akf = np.asarray(anchors[0], np.int32).reshape(-1)
        buv = np.asarray(anchors[1], np.float64).reshape(-1, 2)
    paired = view & (akf >= 0)
    res["pair_kf"][:] = np.where(paired, akf, -1)
    res["uv_before"][paired, 0] = uc[paired]
    res["uv_before"][paired, 1] = vc[paired]
    res["uv_after"][:] = res["uv_before"]
    A, za, zu, zv = lk.affine(points, akf, buv, kf_poses, cur_pose, K, uc, vc)
    if A_override is not None:
        A = np.broadcast_to(np.asarray(A_override, np.float64).reshape(-1, 4), (n, 4)).copy()
    A[~paired] = 0.0
    res["A"][:] = A
    a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    det = a00 * a11 - a01 * a10
    D = np.abs(det)
    lo = 1.0 / ratio
    geo = paired & (za > 0) & (zu > 0) & (zv > 0) & np.isfinite(A).all(1)
    ok = geo & (lo <= D) & (D <= ratio)
    if fm is not None:
        # D against the ratio bounds, and against every value the shift loop
        # can compare (D 4^k against 3 and 1/3, k = -3 .. 3)
        g = np.nonzero(geo)[0]
        fm[g] = np.minimum(fm[g], np.minimum(_rel(D[g], ratio), _rel(D[g], lo)))
        for k in range(-3, 4):
            Dk = D[g] * 4.0 ** k
            fm[g] = np.minimum(fm[g], np.minimum(_rel(Dk, 3.0), _rel(Dk, THIRD)))
    res["status"][paired & ~ok] = 2
    idx = np.nonzero(ok)[0]
    if idx.size == 0:
        return
    shift = np.zeros(n, np.int32)
    shift[idx] = lk.level_shift(D[idx])
    res["shift"][:] = shift
    ai00, ai01, ai10, ai11 = a11[idx] / det[idx], (-a01[idx]) / det[idx], (-a10[idx]) / det[idx], a00[idx] / det[idx]
    cur_l, ws, hs = lk.levels(cur_pyr, w, h)
    kf_l = [lk.levels(k, w, h)[0] for k in kf_pyrs]
    m = idx.size
    lane = np.arange(64)
    px = ((lane >> 3) - 4).astype(np.float64)[None, :]
    py = ((lane & 7) - 4).astype(np.float64)[None, :]
    bu, bv = buv[idx, 0][:, None], buv[idx, 1][:, None]
    kfi = akf[idx]
    cu, cv = uc[idx].copy(), vc[idx].copy()
    succ = np.zeros(m, bool)
    skipped = np.zeros(m, np.int32)
    gain = np.full(m, np.nan)
    offset = np.full(m, np.nan)
    pfm = np.full(m, np.inf)           # flag margins of the points of idx
    ties = np.zeros(m, np.int64)
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
            vm = np.fmin(vm, np.nanmin(np.minimum(np.minimum(np.abs(X), np.abs(wr - (X + 1))),
                                                   np.minimum(np.abs(Y), np.abs(hr - (Y + 1)))), 1))
        pfm = np.fmin(pfm, vm / side)
        T = np.zeros((m, 64))
        J0 = np.zeros((m, 64))
        J1 = np.zeros((m, 64))
        for j in np.unique(kfi[valid]):
            for rl in np.unique(r[valid & (kfi == j)]):
                g = np.nonzero(valid & (kfi == j) & (r == rl))[0]
                buf, gw, gh = kf_l[j][rl], ws[rl], hs[rl]
                smp = [sample(buf, gw, gh, X[g], Y[g]) for X, Y in zip(xs, ys)]
                T[g] = smp[0]
                J0[g] = -0.5 * (smp[1] - smp[2])
                J1[g] = -0.5 * (smp[3] - smp[4])
        # steps 1 and 2: the flat-template floor, written so that NaN skips
        mean, Tc, stt, P0, P1 = project_out(T, J0, J1)
        pfm[valid] = np.minimum(pfm[valid], _rel(stt[valid], STT_MIN))
        run = valid & (stt >= STT_MIN)
        skipped += ~run
        succ[~run] = False
        v = np.nonzero(run)[0]
        if v.size == 0:
            continue
        H00, H01, H11 = tree_sum(P0[v] * P0[v]), tree_sum(P0[v] * P1[v]), tree_sum(P1[v] * P1[v])
        H10 = H01
        invdet = 1.0 / (H00 * H11 - H10 * H01)
        ih = (H11 * invdet, -H01 * invdet, -H10 * invdet, H00 * invdet)
        dx, dy, sc, se, ste, acc, lm, lt = _iterate(T[v], Tc[v], P0[v], P1[v], stt[v], ih, cur_l[level], ws[level],
                                                    hs[level], cu[v] * s, cv[v] * s, px, py, thresh, side)
        succ[v] = sc
        pfm[v] = np.minimum(pfm[v], lm)
        ties[v] += lt
        cu[v] = cu[v] + dx / s
        cv[v] = cv[v] + dy / s
        if level == 0:
            g, o = gain_offset(mean[v], stt[v], se, ste)
            gain[v] = np.where(acc, g, np.nan)
            offset[v] = np.where(acc, o, np.nan)
    # after level 0: the gain's bounds (NaN fails)
    glo, ghi = 1.0 / max_gain, max_gain
    bad = succ & ~((glo <= gain) & (gain <= ghi))
    pfm[succ] = np.minimum(pfm[succ], np.minimum(_rel(gain[succ], glo), _rel(gain[succ], ghi)))
    res["success"][idx] = succ & ~bad
    res["uv_after"][idx, 0] = cu
    res["uv_after"][idx, 1] = cv
    res["status"][idx] = ((skipped << 4) | np.where(bad, 3, 0)).astype(np.uint8)
    res["gain_offset"][idx, 0] = gain
    res["gain_offset"][idx, 1] = offset
    if margins is not None:
        fm[idx] = np.minimum(fm[idx], pfm)
        margins["cost_ties"][idx] = ties


def _iterate(T, Tc, P0, P1, stt, ih, cur, w, h, bx, by, px, py, thresh, side):
    """lk_iterate_illum for every point of the level.  Returns dx, dy, succ,
    the last accepted iteration's se and ste, whether there was one, the
    smallest flag margin and the number of tied cost comparisons per point."""
    m = T.shape[0]
    i00, i01, i10, i11 = ih
    dx, dy = np.zeros(m), np.zeros(m)
    last = np.zeros(m)
    se_acc, ste_acc = np.zeros(m), np.zeros(m)
    acc = np.zeros(m, bool)
    succ = np.ones(m, bool)
    fm = np.full(m, np.inf)
    ties = np.zeros(m, np.int64)
    act = np.arange(m)
    cx, cy = bx[:, None] + px, by[:, None] + py
    lim = np.array([w, h, w, h], np.float64)[None, :]
    for it in range(100):
        if act.size == 0:
            break
        qx, qy = bx[act] + dx[act], by[act] + dy[act]
        q = np.stack([qx + -HP, qy + -HP, qx + HP, qy + HP], 1)
        out = ~((q >= 0) & (q < lim)).all(1)
        d = np.where(np.isfinite(q), np.minimum(np.abs(q), np.abs(lim - q)), np.inf).min(1)
        fm[act] = np.minimum(fm[act], d / side)
        succ[act[out]] = False
        act = act[~out]
        if act.size == 0:
            break
        smp = sample(cur, w, h, cx[act] + dx[act][:, None], cy[act] + dy[act][:, None])
        B0, B1, see, se, ste, cost = iteration_sums(T[act], Tc[act], P0[act], P1[act], stt[act], smp)
        u0 = i00[act] * B0 + i01[act] * B1
        u1 = i10[act] * B0 + i11[act] * B1
        nan = np.isnan(u0)
        succ[act[nan]] = False
        worse = ~nan & (cost > last[act]) if it > 0 else np.zeros(act.size, bool)
        if it > 0:
            tie = ~nan & (_rel(cost, last[act]) <= 1e-9)
            ties[act[tie]] += 1
        go = ~nan & ~worse
        g = act[go]
        dx[g] += u0[go]
        dy[g] += u1[go]
        last[g] = cost[go]
        succ[g] = ~(cost[go] > thresh)
        fm[g] = np.minimum(fm[g], _rel(cost[go], thresh))
        acc[g] = True
        se_acc[g] = se[go]
        ste_acc[g] = ste[go]
        act = g
    return dx, dy, succ, se_acc, ste_acc, acc, fm, ties
