"""Restatement of the depth seeds (viso_depth_seeds_create / _update /
_promote) in elementwise numpy fp64, in the operand order of
the rule.

A seed is a corner of a keyframe with an inverse depth ``mu`` (of z in the
host camera) and its variance ``s2``.  Every later frame searches the seed's
epipolar segment ``mu ± 2 sigma`` for the host patch and fuses the depth of the
best step into (mu, s2); a converged seed becomes a map point.

Vectorised over the seeds: every element sees the operations the rule states,
in its order (numpy's elementwise ufuncs neither reassociate nor contract).
``sample``, ``tree_sum``, ``project``, ``level_shift`` and the affine map are
those of tests/lk_warp_ref.py; the details DESIGN.md §18 decides (the warp's
area ratio, the step count, the order of the promotion's classes) are decided
here.
"""
from __future__ import annotations

import numpy as np

from tests import lk_warp_ref as lk
from tests import mono_kf_ref, oracle_lib

K_MAX_SEEDS = 8192
AREA_RATIO = 64.0     # the warp is rejected outside 1/64 <= |det A| <= 64 (§17's default)
TAU_FLOOR = 1e-4      # tau >= this share of the inverse depth range
SCALE = np.array(lk.SCALE)


def params(max_steps=32, depth_min=2.0, depth_max=60.0, max_score=64 * 30.0 ** 2, uniqueness=1.5, min_good=3,
           conv_rel=0.05, max_bad=4, max_lost=4):
    return dict(max_steps=int(max_steps), depth_min=float(depth_min), depth_max=float(depth_max),
                max_score=float(max_score), uniqueness=float(uniqueness), min_good=int(min_good),
                conv_rel=float(conv_rel), max_bad=int(max_bad), max_lost=int(max_lost))


def empty_rows(n=0):
    """Seed rows: h, uv, mu, s2, cnt = (good, bad, lost, status)."""
    return dict(h=np.zeros(n, np.int32), uv=np.zeros((n, 2)), mu=np.zeros(n), s2=np.zeros(n),
                cnt=np.zeros((n, 4), np.int32))


def copy_rows(rows):
    return {k: np.array(v, copy=True) for k, v in rows.items()}


def take_rows(rows, idx):
    return {k: np.array(v[idx], copy=True) for k, v in rows.items()}


def concat_rows(a, b):
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def new_rows(xy, host, depth_min, depth_max):
    """The rows of fresh seeds at the corners xy (n, 2)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    rho_min, rho_max = 1.0 / depth_max, 1.0 / depth_min
    r = empty_rows(n)
    r["h"][:] = host
    r["uv"][:] = xy
    r["mu"][:] = (rho_min + rho_max) / 2.0
    s = (rho_max - rho_min) / 4.0
    r["s2"][:] = s * s
    return r


# ---------------------------------------------------------------- creation
def create(image, width, height, K, pose_c, points, cell, host, depth_min, depth_max, n_live=0, fast_thresh=50,
           max_features=32768):
    """The seeds a new keyframe c adds: the cell winners (§12 steps 1-2) of
    c's level-0 FAST corners in the cells the map leaves unmarked, in corner
    order, up to K_MAX_SEEDS - n_live.  Returns (rows, winners)."""
    img = np.ascontiguousarray(image, np.uint8).reshape(height, width)
    xs, ys, sc = oracle_lib.fast(img, fast_thresh)
    xs, ys, sc = xs[:max_features], ys[:max_features], sc[:max_features]
    occ = mono_kf_ref.occupancy(points, pose_c, K, width, height, cell)
    win = mono_kf_ref.cell_winners(xs, ys, sc, occ, cell)
    xy = np.array([[xs[i], ys[i]] for i in win], np.float64).reshape(-1, 2)
    room = max(0, K_MAX_SEEDS - int(n_live))
    return new_rows(xy[:room], host, depth_min, depth_max), len(win)


# ---------------------------------------------------------------- geometry
def relative(cur_pose, host_poses):
    """R = R_c R_h^T (9 arrays), t = t_c - R t_h (3 arrays); host_poses (12, n)."""
    c, hp = cur_pose, host_poses
    R = [lk.dot3(c[3 * i], c[3 * i + 1], c[3 * i + 2], hp[3 * j], hp[3 * j + 1], hp[3 * j + 2])
         for i in range(3) for j in range(3)]
    t = [c[9 + i] - lk.dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], hp[9], hp[10], hp[11]) for i in range(3)]
    return R, t


def ray(uv, K, R):
    """f = ((u - cx) / fx, (v - cy) / fy, 1) and q = R f."""
    fx, fy, cx, cy = K
    f = ((uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(uv.shape[0]))
    q = [lk.dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], f[0], f[1], f[2]) for i in range(3)]
    return f, q


def px(q, t, rho, K):
    """The pixel of inverse depth rho: project_px of q + rho t; (u, v, z)."""
    X = [q[i] + rho * t[i] for i in range(3)]
    return X[0] / X[2] * K[0] + K[2], X[1] / X[2] * K[1] + K[3], X[2]


def rho_of(m_k, k, q, t, K):
    """The inverse depth whose pixel has coordinate m_k on axis k (0: x, 1: y)."""
    c_k = np.where(k == 0, K[2], K[3])
    f_k = np.where(k == 0, K[0], K[1])
    q_k = np.where(k == 0, q[0], q[1])
    t_k = np.where(k == 0, t[0], t[1])
    n_k = (m_k - c_k) / f_k
    return (n_k * q[2] - q_k) / (t_k - n_k * t[2])


def seed_affine(uv, mu, hp, cur_pose, K, uc, vc):
    """§17 step 2 with anchor h, (bu, bv) = (u, v), za = 1 / mu."""
    fx, fy, cx, cy = K
    za = 1.0 / mu
    out = []
    for du, dv in ((lk.H_STEP, 0.0), (0.0, lk.H_STEP)):
        qu = uv[:, 0] + du if du else uv[:, 0]
        qv = uv[:, 1] + dv if dv else uv[:, 1]
        d0 = (qu - cx) / fx * za - hp[9]
        d1 = (qv - cy) / fy * za - hp[10]
        d2 = za - hp[11]
        W = tuple((hp[j] * d0 + hp[3 + j] * d1) + hp[6 + j] * d2 for j in range(3))
        u, v, z = lk.project(cur_pose, K, W)
        out.append(((u - uc) / lk.H_STEP, (v - vc) / lk.H_STEP, z))
    (a00, a10, zu), (a01, a11, zv) = out
    return np.stack([a00, a01, a10, a11], 1), za, zu, zv


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        m = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.where(np.isfinite(m), m, np.inf)


# ---------------------------------------------------------------- update
def update(rows, kf_pyrs, kf_poses, cur_pyr, cur_pose, w, h, K, prm):
    """One frame's update of every seed.  Returns (rows, diag): diag holds the
    search level ``l`` and the best step ``jstar`` (-1 where not reached), the
    scores ``S`` (n, 64; inf = invalid), and ``margin`` (n,): the seed's
    smallest relative distance from any threshold it compared."""
    rows = copy_rows(rows)
    n = rows["h"].shape[0]
    diag = dict(l=np.full(n, -1, np.int32), jstar=np.full(n, -1, np.int32), S=np.full((n, 64), np.inf),
                margin=np.full(n, np.inf), shift=np.zeros(n, np.int32))
    if n == 0:
        return rows, diag
    with np.errstate(all="ignore"):
        _update(rows, diag, kf_pyrs, np.ascontiguousarray(kf_poses, np.float64).reshape(-1, 12),
                np.ascontiguousarray(cur_pose, np.float64).reshape(12), cur_pyr, w, h, [float(k) for k in K], prm)
    return rows, diag


def _update(rows, diag, kf_pyrs, kf_poses, cur_pose, cur_pyr, w, h, K, prm):
    n = rows["h"].shape[0]
    hst, uv, mu, s2, cnt = rows["h"], rows["uv"], rows["mu"], rows["s2"], rows["cnt"]
    margin = diag["margin"]
    max_steps = prm["max_steps"]
    rho_min, rho_max = 1.0 / prm["depth_max"], 1.0 / prm["depth_min"]
    status = np.full(n, -1, np.int32)
    todo = lambda: status < 0

    def note(sel, a, b):
        m = _rel(a, b)
        margin[sel] = np.minimum(margin[sel], m)

    def note_px(sel, dist_px):  # a distance in pixels, against coordinates of at most max(w, h)
        margin[sel] = np.minimum(margin[sel], np.abs(dist_px) / max(w, h))

    # 1. the segment
    hp = kf_poses[hst].T  # (12, n)
    R, t = relative(cur_pose, hp)
    f, q = ray(uv, K, R)
    sig = np.sqrt(s2)
    rlo = np.maximum(mu - 2.0 * sig, rho_min)
    rhi = np.minimum(mu + 2.0 * sig, rho_max)
    ax, ay, az = px(q, t, rlo, K)
    bx, by, bz = px(q, t, rhi, K)
    mx, my, mz = px(q, t, mu, K)
    ok = (az > 0) & (bz > 0) & (mz > 0) & lk.inside(mx, my, w, h)
    status[~ok] = 1
    act = todo()
    note_px(act, np.minimum(np.minimum(mx, w - mx), np.minimum(my, h - my))[act])
    # 2. the level and the steps
    dx, dy = bx - ax, by - ay
    Lm = np.maximum(np.abs(dx), np.abs(dy))
    k = np.where(np.abs(dx) >= np.abs(dy), 0, 1)
    lvl = np.full(n, -1, np.int32)
    for l in range(3, -1, -1):
        lvl = np.where(Lm * lk.SCALE[l] <= max_steps - 1, l, lvl)
    for l in range(4):
        note(act, (Lm * lk.SCALE[l])[act], float(max_steps - 1))
    status[todo() & (lvl < 0)] = 3
    ks = SCALE[np.maximum(lvl, 0)]
    Ls = Lm * ks
    act = todo()
    note(act, Ls[act], 1.0)
    status[act & (Ls < 1)] = 4
    act = todo()
    nst = np.where(act, np.floor(np.where(act, Ls, 0.0)) + 1, 0).astype(np.int32)
    note(act, Ls[act], np.floor(Ls[act]))
    note(act, Ls[act], np.floor(Ls[act]) + 1)
    note(act, np.abs(dx)[act], np.abs(dy)[act])
    ex, ey = dx / Lm, dy / Lm
    diag["l"][:] = np.where(act, lvl, -1)
    # 3. the template
    A, za, zu, zv = seed_affine(uv, mu, hp, cur_pose, K, mx, my)
    a00, a01, a10, a11 = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    det = a00 * a11 - a01 * a10
    D = np.abs(det)
    wok = (za > 0) & (zu > 0) & (zv > 0) & np.isfinite(A).all(1) & (1.0 / AREA_RATIO <= D) & (D <= AREA_RATIO)
    note(act, D[act], AREA_RATIO)
    note(act, D[act], 1.0 / AREA_RATIO)
    status[act & ~wok] = 2
    act = todo()
    idx = np.nonzero(act)[0]
    if idx.size:
        shift = lk.level_shift(D[idx])
        for i in range(4):  # every comparison level_shift can make, per seed
            note(idx, D[idx] * 0.25 ** i, 3.0)
            note(idx, D[idx] * 4.0 ** i, lk.THIRD)
        diag["shift"][idx] = shift
        _search(rows, diag, status, idx, shift, (a00, a01, a10, a11, det), kf_pyrs, cur_pyr, w, h, K, prm,
                (ax, ay, ex, ey, ks, nst, k, q, t, lvl), note, note_px)
    # the counters: 1, 2, 5, 6 lose the seed once more; 3 and 4 change nothing;
    # 0 and 7..9 found a search to score, so lost = 0
    lost_up = np.isin(status, (1, 2, 5, 6))
    scored = (status == 0) | (status >= 7)
    cnt[:, 2] = np.where(lost_up, cnt[:, 2] + 1, np.where(scored, 0, cnt[:, 2]))
    cnt[:, 1] = np.where(status >= 7, cnt[:, 1] + 1, cnt[:, 1])
    cnt[:, 0] = np.where(status == 0, cnt[:, 0] + 1, cnt[:, 0])
    cnt[:, 3] = status


def _search(rows, diag, status, idx, shift, Aall, kf_pyrs, cur_pyr, w, h, K, prm, geo, note, note_px):
    a00, a01, a10, a11, det = (v[idx] for v in Aall)
    ax, ay, ex, ey, ks, nst, k = (v[idx] for v in geo[:7])
    q = [v[idx] for v in geo[7]]
    t = [v[idx] for v in geo[8]]
    lvl = geo[9][idx]
    uv, mu, s2, hst = rows["uv"][idx], rows["mu"][idx], rows["s2"][idx], rows["h"][idx]
    m = idx.size
    rho_min, rho_max = 1.0 / prm["depth_max"], 1.0 / prm["depth_min"]
    st = np.full(m, -1, np.int32)
    c = lambda v: v[:, None]
    ai00, ai01, ai10, ai11 = a11 / det, (-a01) / det, (-a10) / det, a00 / det
    cur_l, ws, hs = lk.levels(cur_pyr, w, h)
    kf_l = [lk.levels(p, w, h)[0] for p in kf_pyrs]
    wsa, hsa = np.array(ws, np.float64), np.array(hs, np.float64)
    lane = np.arange(64)
    pxo = ((lane >> 3) - 4).astype(np.float64)[None, :]
    pyo = ((lane & 7) - 4).astype(np.float64)[None, :]
    # the template at level r = clamp(l + shift, 0, 3)
    r = np.clip(lvl + shift, 0, 3)
    sr = SCALE[r]
    kk = c(sr / ks)
    x = c(uv[:, 0]) * c(sr) + ((c(ai00) * pxo + c(ai01) * pyo) * kk)
    y = c(uv[:, 1]) * c(sr) + ((c(ai10) * pxo + c(ai11) * pyo) * kk)
    wr, hr = c(wsa[r]), c(hsa[r])
    tin = ((0 <= x) & (x + 1 < wr) & (0 <= y) & (y + 1 < hr)).all(1)
    note_px(idx, np.min(np.minimum(np.minimum(np.abs(x), np.abs(wr - (x + 1))),
                                   np.minimum(np.abs(y), np.abs(hr - (y + 1)))), 1))
    st[~tin] = 5
    I1 = np.zeros((m, 64))
    for j in np.unique(hst[tin]):
        for rl in np.unique(r[tin & (hst == j)]):
            g = np.nonzero(tin & (hst == j) & (r == rl))[0]
            I1[g] = lk.sample(kf_l[j][rl], ws[rl], hs[rl], x[g], y[g])
    tt = I1 - c(lk.tree_sum(I1) / 64.0)
    # 4. the scores
    S = np.full((m, 64), np.inf)
    valid = np.zeros((m, 64), bool)
    for j in range(64):
        pxj, pyj = ax * ks + j * ex, ay * ks + j * ey
        X, Y = c(pxj) + pxo, c(pyj) + pyo
        wl, hl = c(wsa[lvl]), c(hsa[lvl])
        run = (st < 0) & (j < nst)
        vin = ((0 <= X) & (X < wl - 1) & (0 <= Y) & (Y < hl - 1)).all(1)
        if run.any():
            note_px(idx[run], np.min(np.minimum(np.minimum(np.abs(X), np.abs(wl - 1 - X)),
                                                np.minimum(np.abs(Y), np.abs(hl - 1 - Y))), 1)[run])
        go = run & vin
        for l in np.unique(lvl[go]):
            g = np.nonzero(go & (lvl == l))[0]
            cs = lk.sample(cur_l[l], ws[l], hs[l], X[g], Y[g])
            cb = lk.tree_sum(cs) / 64.0
            e = (cs - c(cb)) - tt[g]
            S[g, j] = lk.tree_sum(e * e)
            valid[g, j] = True
    st[(st < 0) & (valid.sum(1) < 3)] = 6
    diag["S"][idx] = S
    # 5. the best step and the second best
    jst = np.argmin(S, 1)  # the first of the least
    Sst = S[np.arange(m), jst]
    far = np.abs(np.arange(64)[None, :] - c(jst)) > 1
    S2 = np.min(np.where(far, S, np.inf), 1)
    act = st < 0
    diag["jstar"][idx[act]] = jst[act]
    # (the least against the next: any other valid step)
    other = np.min(np.where(np.arange(64)[None, :] != c(jst), S, np.inf), 1)
    note(idx[act], Sst[act], other[act])
    note(idx[act], Sst[act], prm["max_score"])
    st[act & (Sst > prm["max_score"])] = 7
    act = st < 0
    note(idx[act], (Sst * prm["uniqueness"])[act], S2[act])
    st[act & (Sst * prm["uniqueness"] > S2)] = 8
    act = st < 0
    # 6. the sub-step
    jm, jp = np.maximum(jst - 1, 0), np.minimum(jst + 1, 63)
    Sm = np.where(jst > 0, S[np.arange(m), jm], np.inf)
    Sp = np.where(jst < 63, S[np.arange(m), jp], np.inf)
    den = (Sm - 2.0 * Sst) + Sp
    par = (jst > 0) & (jst < 63) & valid[np.arange(m), jm] & valid[np.arange(m), jp] & (den > 0)
    delta = np.where(par, np.minimum(np.maximum(0.5 * (Sm - Sp) / np.where(par, den, 1.0), -0.5), 0.5), 0.0)
    pk = np.where(k == 0, ax * ks + jst * ex, ay * ks + jst * ey)
    ek = np.where(k == 0, ex, ey)
    m_k = (pk + delta * ek) / ks
    # 7. the depth
    robs = rho_of(m_k, k, q, t, K)
    r1 = rho_of(m_k + 1.0 / ks, k, q, t, K)
    good = np.isfinite(robs) & np.isfinite(r1) & (rho_min <= robs) & (robs <= rho_max)
    note(idx[act], robs[act], rho_min)
    note(idx[act], robs[act], rho_max)
    st[act & ~good] = 9
    act = st < 0
    dr = r1 - robs
    fl = TAU_FLOOR * (rho_max - rho_min)
    tau2 = np.maximum(dr * dr, fl * fl)
    # 8. the fusion
    v = s2 + tau2
    mu_new = (tau2 * mu + s2 * robs) / v
    s2_new = s2 * tau2 / v
    st[act] = 0
    rows["mu"][idx[act]] = mu_new[act]
    rows["s2"][idx[act]] = s2_new[act]
    status[idx] = st


# ---------------------------------------------------------------- promotion
def classify(rows, prm):
    """Per seed: 2 converged, 1 dropped, 0 neither (converged comes first)."""
    cnt, mu, s2 = rows["cnt"], rows["mu"], rows["s2"]
    lim = prm["conv_rel"] * mu
    conv = (cnt[:, 0] >= prm["min_good"]) & (s2 <= lim * lim)
    drop = (cnt[:, 1] >= prm["max_bad"]) | (cnt[:, 2] >= prm["max_lost"])
    return np.where(conv, 2, np.where(drop, 1, 0)), _rel(s2, lim * lim)


def promote(rows, kf_poses, K, room, prm):
    """One promotion.  Returns dict(points (p, 3) world, host (p,), rows (the
    survivors, in order), counts [converged, promoted, dropped, survivors])."""
    kf_poses = np.ascontiguousarray(kf_poses, np.float64).reshape(-1, 12)
    fx, fy, cx, cy = (float(x) for x in K)
    cls, _ = classify(rows, prm)
    conv = cls == 2
    rank = np.cumsum(conv) - 1
    prom = conv & (rank < room)
    surv = ~prom & (cls != 1)
    i = np.nonzero(prom)[0]
    hp = kf_poses[rows["h"][i]].T
    mu, uv = rows["mu"][i], rows["uv"][i]
    with np.errstate(all="ignore"):
        d = [((uv[:, 0] - cx) / fx) / mu - hp[9], ((uv[:, 1] - cy) / fy) / mu - hp[10], 1.0 / mu - hp[11]]
        P = np.stack([(hp[j] * d[0] + hp[3 + j] * d[1]) + hp[6 + j] * d[2] for j in range(3)], 1)
    return dict(points=P.reshape(-1, 3), host=rows["h"][i].copy(), rows=take_rows(rows, np.nonzero(surv)[0]),
                counts=[int(conv.sum()), int(prom.sum()), int((cls == 1).sum()), int(surv.sum())])
