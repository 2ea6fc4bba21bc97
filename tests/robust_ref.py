"""TEST INFRASTRUCTURE ONLY — numpy restatement of the robust form of the
brightness-compensated tracking stage (viso_track_robust, viso_set_robust;
include/viso/viso_c.h): tests/bright_ref.py's rule with a Huber
weight per patch pixel.  The repo's own spec.

It is bright_ref's rule with these changes and no others.  Per pixel, with
e = (g_j R + o_j) - C as there: r = |e|, out = r > k (strict), w = out ? k / r
: 1.0.  Each of the 14 pixel sums has the leaf w * x, x being bright_ref's leaf
computed as it computes it (w * (g0 * g0), w * (e * R), ...), but sum 5, the
cost, whose leaf is out ? k * (2.0 * r - k) : e * e (twice the Huber
function).  A fifteenth sum, sum w, by the same descending 64-leaf tree, and
the count of `out` pixels of the point.  The 46 terms of a point: 0..43 as in
bright_ref from the weighted sums, 44 = sum w, 45 = the count; all through the
canonical map tree, +0.0 for a point that is not good.  The step takes d11 =
S[44] in place of 64 n_j; cost_j = S[27] / n_j.  The decisions, the exits, the
restore on exits 1 and 5 and the level hand-down are bright_ref's.

The report has 28 columns: 0..22 as bright_ref's, 23 = k, 24 and 25 = S[44] and
S[45] of the last pass evaluated on level 0, 26 and 27 = 0.  The weights are
that pass's sum w per point, 0 where the point is not good.  "The last pass
evaluated" is the last pass whose sums were formed: after exit 1 or 5 that is
the pass that was rejected, not the kept one.

With a k that no residual exceeds every w is 1.0, w * x is x, S[44] is 64 n_j
exactly and the rule is bright_ref's bit for bit.

``margins`` collects bright_ref's keys and ``huber``: the smallest |r - k| over
all evaluated pixels (a pixel closer to k than the device's and this file's
residuals differ could be weighted on one side only).
"""
from __future__ import annotations

import math

import numpy as np

from tests import bright_ref as br
from tests.kf_align_ref import DELTA_THRESH, HP, NAN, _PX, _PY, _border, _inside, _note, d_pixel_d_xi
from tests.lk_warp_ref import SCALE, levels, project, sample, tree_sum_desc64
from tests.pose_refine_ref import left_update

N_TERMS = 46
f64 = np.float64


def pixel_sums(last_buf, cur_buf, w, h, ur, vr, uc, vc, g, o, k, margins=None):
    """The 14 weighted pixel sums, sum w and the `out` count of the points
    whose patch centres are (ur, vr) and (uc, vc): a list of 16 arrays."""
    c = lambda a: a[:, None]
    k = f64(k)
    xc, yc = c(uc) + _PX, c(vc) + _PY
    R = sample(last_buf, w, h, c(ur) + _PX, c(vr) + _PY)
    C = sample(cur_buf, w, h, xc, yc)
    g0 = 0.5 * (sample(cur_buf, w, h, xc + 1, yc) - sample(cur_buf, w, h, xc - 1, yc))
    g1 = 0.5 * (sample(cur_buf, w, h, xc, yc + 1) - sample(cur_buf, w, h, xc, yc - 1))
    e = (g * R + o) - C
    r = np.abs(e)
    out = r > k
    _note(margins, "huber", np.abs(r - k))
    wt = np.where(out, k / np.where(out, r, 1.0), 1.0)
    rho = np.where(out, k * (2.0 * r - k), e * e)
    leaves = [wt * x for x in (g0 * g0, g0 * g1, g1 * g1, e * g0, e * g1)] + [rho] + \
             [wt * x for x in (g0 * R, g1 * R, g0, g1, R * R, R, e * R, e)] + [wt]
    return [tree_sum_desc64(v) for v in leaves] + [out.sum(axis=1).astype(np.float64)]


def point_terms(last_buf, cur_buf, w, h, L, T, g, o, k, K, P, level, margins=None):
    """One pass's per-point part at pyramid level `level`: good (n,) and the
    46 terms (n, 46), zero where not good."""
    s = SCALE[level]
    g, o = f64(g), f64(o)
    with np.errstate(all="ignore"):
        u0, v0, zr = project(L, K, P)
        u1, v1, zc = project(T, K, P)
        ur, vr, uc, vc = s * u0, s * v0, s * u1, s * v1
        good = (_inside(ur - HP, vr - HP, w, h) & _inside(ur + HP, vr + HP, w, h) &
                _inside(uc - HP, vc - HP, w, h) & _inside(uc + HP, vc + HP, w, h) & (zr > 0) & (zc > 0))
        if margins is not None:
            _note(margins, "z", np.abs(zc))
            front = (zr > 0) & (zc > 0)
            for u, v in ((ur, vr), (uc, vc)):
                _note(margins, "good_px", np.minimum(_border(u - HP, v - HP, w, h), _border(u + HP, v + HP, w, h))[front])
        terms = np.zeros((good.shape[0], N_TERMS))
        i = np.nonzero(good)[0]
        if i.size == 0:
            return good, terms
        J0, J1 = d_pixel_d_xi(T, K, tuple(c[i] for c in P), s)
        G = pixel_sums(last_buf, cur_buf, w, h, ur[i], vr[i], uc[i], vc[i], g, o, k, margins)
        t = 0
        for a in range(6):
            for b in range(a, 6):
                terms[i, t] = (G[0] * (J0[a] * J0[b]) + G[1] * (J0[a] * J1[b] + J1[a] * J0[b])) + G[2] * (J1[a] * J1[b])
                t += 1
        for a in range(6):
            terms[i, 21 + a] = G[3] * J0[a] + G[4] * J1[a]
            terms[i, 28 + a] = -(G[6] * J0[a] + G[7] * J1[a])
            terms[i, 34 + a] = -(G[8] * J0[a] + G[9] * J1[a])
        terms[i, 27] = G[5]
        terms[i, 40] = G[10]
        terms[i, 41] = G[11]
        terms[i, 42] = -G[12]
        terms[i, 43] = -G[13]
        terms[i, 44] = G[14]
        terms[i, 45] = G[15]
    return good, terms


def step(S):
    """(xi[6], dg, do) from a pass's 46 sums: bright_ref.step with d11 =
    S[44].  bright_ref.step forms d11 as 64.0 * n; S[44] / 64 is exact (a power
    of two), so 64.0 * (S[44] / 64.0) is S[44] itself."""
    return br.step(S[:44], f64(S[44]) / f64(64.0))


def track_level(last_buf, cur_buf, w, h, L, state, k, K, P, level, iterations, margins=None, trace=None):
    """One level from state = (T, g, o): (kept state, exit, steps applied, n,
    cost, the last evaluated pass's (S[44], S[45], weights))."""
    T, g, o = [float(x) for x in state[0]], float(state[1]), float(state[2])
    prev = None  # (state, n, cost) of pass j - 1
    j = 0
    while True:
        good, terms = point_terms(last_buf, cur_buf, w, h, L, T, g, o, k, K, P, level, margins)
        S = [float(x) for x in br.map_tree_sum(terms)]
        n = int(good.sum())
        ev = (S[44], S[45], terms[:, 44].copy())
        with np.errstate(all="ignore"):
            cost = float(f64(S[27]) / f64(n))
        if trace is not None:
            trace.append((level, j, n, cost, g, o))
        if n < 6 or not math.isfinite(cost):
            if j == 0:
                return (T, g, o), 4, 0, n, NAN, ev
            return prev[0], 5, j - 1, prev[1], prev[2], ev
        if j >= 1:
            if margins is not None:
                _note(margins, "cost_b", abs(cost - prev[2]) / prev[2])
                _note(margins, "cost_c", abs((1 - cost / prev[2]) - DELTA_THRESH))
            if cost >= prev[2]:
                return prev[0], 1, j - 1, prev[1], prev[2], ev
            if (1 - cost / prev[2]) < DELTA_THRESH:
                return (T, g, o), 2, j, n, cost, ev
        if j == iterations:
            return (T, g, o), 0, j, n, cost, ev
        xi, dg, do = step(S)
        if not all(math.isfinite(x) for x in list(xi) + [dg, do]):
            return (T, g, o), 3, j, n, cost, ev
        prev = ((T, g, o), n, cost)
        T, g, o = left_update(xi, T), g + dg, o + do
        j += 1


def track_robust(last_pyr, cur_pyr, w, h, K, points, pose_last, seed, iterations=10, k=9.0, margins=None, trace=None):
    """viso_track_robust: (pose (12,), report (28,), weights (n,))."""
    K = [float(x) for x in K]
    L = [float(x) for x in np.asarray(pose_last, np.float64).reshape(12)]
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    ll, ws, hs = levels(last_pyr, w, h)
    cl, _, _ = levels(cur_pyr, w, h)
    state = ([float(x) for x in np.asarray(seed, np.float64).reshape(12)], 1.0, 0.0)
    rep = np.zeros(28)
    total = 0
    for q, level in enumerate((3, 2, 1, 0)):
        state, ex, steps, n, cost, ev = track_level(ll[level], cl[level], ws[level], hs[level], L, state, k, K, P,
                                                    level, iterations, margins, trace)
        rep[4 + 4 * q:8 + 4 * q] = (ex, steps, n, cost)
        total += steps
    rep[0] = 2 if ex == 4 else 0
    rep[1], rep[2], rep[3] = pts.shape[0], n, cost
    rep[20], rep[21], rep[22] = state[1], state[2], total
    rep[23], rep[24], rep[25] = k, ev[0], ev[1]
    return np.array(state[0], np.float64), rep, ev[2]
