"""TEST INFRASTRUCTURE ONLY — numpy restatement of the brightness-compensated
tracking stage (viso_track_affine, viso_set_brightness; include/viso/viso_c.h;
DESIGN.md §22): the frame's pose estimated together with an affine brightness
map (g, o) from the last frame to the current one, iterated on every pyramid
level.  The repo's own spec.

State (T, g, o), (seed, 1, 0) on level 3; each lower level starts from the
result of the level above.  Pass j on a level at (T_j, g_j, o_j): a point is
good as in the keyframe alignment (both 8x8 patches inside the level, depth > 0
under the last pose L and under T_j); per patch pixel (x outer, y inner)
R = sample(last), C = sample(cur), (g0, g1) = gradient(cur), e = (g_j R + o_j)
- C; the 14 pixel sums by ``tree_sum_desc64``; the 44 terms of a point:

    0..27   the keyframe alignment's 28 (A's upper triangle row-major in the
            factored form, b_a = G3 J0a + G4 J1a, the cost G5), with this e
    28..33  B_a0 = -((sum g0 R) J0a + (sum g1 R) J1a)
    34..39  B_a1 = -((sum g0) J0a + (sum g1) J1a)
    40, 41  d00 = sum R R, d01 = sum R
    42, 43  c0 = -(sum e R), c1 = -(sum e)

and d11 = 64 n_j.  Across points every term goes through the direct pose's
canonical map tree (oracle_common.hpp map_tree_sum, groups = 256, +0.0 for a
point that is not good).  The step eliminates (g, o) by the Schur complement
(``step``) and reuses pose_refine_ref.solve; the decisions are the keyframe
alignment's (kf_align_ref.align_level) with "(T, g, o)" for "T" and exit 3
also on a non-finite dg or do.

Elementwise numpy fp64 over the points of a pass (numpy's ufuncs neither
reassociate nor contract), numpy fp64 scalars for the step and the decisions,
in the operand order of the rule.

``margins`` (a dict) collects the smallest distance of every kind of decision
from its threshold, with kf_align_ref's keys (good_px, z, cost_b, cost_c).
"""
from __future__ import annotations

import math

import numpy as np

from tests.kf_align_ref import DELTA_THRESH, HP, NAN, _PX, _PY, _border, _inside, _note, d_pixel_d_xi
from tests.lk_warp_ref import SCALE, levels, project, sample, tree_sum_desc64
from tests.pose_refine_ref import left_update, solve

N_TERMS = 44
GROUPS = 256
f64 = np.float64


def map_tile(n):
    """oracle_common.hpp map_tile(n, 256)."""
    return max(1, min(64, (n + GROUPS - 1) // GROUPS))


def _tree(v):
    """oracle_common.hpp tree_sum over axis 0: the leaves padded with +0.0 to
    a power of two, neighbours first."""
    n = v.shape[0]
    p = 1
    while p < n:
        p <<= 1
    if p > n:
        v = np.concatenate([v, np.zeros((p - n,) + v.shape[1:])])
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def map_tree_sum(terms):
    """oracle_common.hpp map_tree_sum over axis 0 of (n, k) leaves."""
    n = terms.shape[0]
    if n <= 0:
        return np.zeros(terms.shape[1:])
    T = map_tile(n)
    with np.errstate(all="ignore"):
        tiles = np.stack([_tree(terms[t:t + T]) for t in range(0, n, T)])
        return _tree(tiles)


def pixel_sums(last_buf, cur_buf, w, h, ur, vr, uc, vc, g, o):
    """The 14 pixel sums of the points whose patch centres are (ur, vr) in the
    last level and (uc, vc) in the current one: a list of 14 arrays."""
    c = lambda a: a[:, None]
    xc, yc = c(uc) + _PX, c(vc) + _PY
    R = sample(last_buf, w, h, c(ur) + _PX, c(vr) + _PY)
    C = sample(cur_buf, w, h, xc, yc)
    g0 = 0.5 * (sample(cur_buf, w, h, xc + 1, yc) - sample(cur_buf, w, h, xc - 1, yc))
    g1 = 0.5 * (sample(cur_buf, w, h, xc, yc + 1) - sample(cur_buf, w, h, xc, yc - 1))
    e = (g * R + o) - C
    return [tree_sum_desc64(v) for v in (g0 * g0, g0 * g1, g1 * g1, e * g0, e * g1, e * e, g0 * R, g1 * R, g0, g1,
                                         R * R, R, e * R, e)]


def point_terms(last_buf, cur_buf, w, h, L, T, g, o, K, P, level, margins=None):
    """One pass's per-point part at pyramid level `level`: good (n,) and the
    44 terms (n, 44), zero where not good."""
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
        G = pixel_sums(last_buf, cur_buf, w, h, ur[i], vr[i], uc[i], vc[i], g, o)
        k = 0
        for a in range(6):
            for b in range(a, 6):
                terms[i, k] = (G[0] * (J0[a] * J0[b]) + G[1] * (J0[a] * J1[b] + J1[a] * J0[b])) + G[2] * (J1[a] * J1[b])
                k += 1
        for a in range(6):
            terms[i, 21 + a] = G[3] * J0[a] + G[4] * J1[a]
            terms[i, 28 + a] = -(G[6] * J0[a] + G[7] * J1[a])
            terms[i, 34 + a] = -(G[8] * J0[a] + G[9] * J1[a])
        terms[i, 27] = G[5]
        terms[i, 40] = G[10]
        terms[i, 41] = G[11]
        terms[i, 42] = -G[12]
        terms[i, 43] = -G[13]
    return good, terms


def step(S, n):
    """(xi[6], dg, do) from a pass's 44 sums and its n: (g, o) eliminated by
    the Schur complement, the 6x6 solve of pose_refine_ref.solve."""
    S = [f64(x) for x in S]
    with np.errstate(all="ignore"):
        d00, d01, c0, c1 = S[40], S[41], S[42], S[43]
        d11 = f64(64.0) * f64(n)
        det = d00 * d11 - d01 * d01
        q0 = (d11 * c0 - d01 * c1) / det
        q1 = (d00 * c1 - d01 * c0) / det
        B0, B1 = S[28:34], S[34:40]
        Y0 = [(d11 * B0[a] - d01 * B1[a]) / det for a in range(6)]
        Y1 = [(d00 * B1[a] - d01 * B0[a]) / det for a in range(6)]
        Sp = [0.0] * 28
        k = 0
        for a in range(6):
            for b in range(a, 6):
                Sp[k] = float(S[k] - (B0[a] * Y0[b] + B1[a] * Y1[b]))
                k += 1
        for a in range(6):
            Sp[21 + a] = float(S[21 + a] - (B0[a] * q0 + B1[a] * q1))
        xi = solve(Sp)
        s0 = Y0[0] * f64(xi[0])
        s1 = Y1[0] * f64(xi[0])
        for a in range(1, 6):
            s0 = s0 + Y0[a] * f64(xi[a])
            s1 = s1 + Y1[a] * f64(xi[a])
        dg, do = q0 - s0, q1 - s1
    return xi, float(dg), float(do)


def track_level(last_buf, cur_buf, w, h, L, state, K, P, level, iterations, margins=None, trace=None):
    """One level from state = (T, g, o): (kept state, exit, steps applied, n,
    cost)."""
    T, g, o = [float(x) for x in state[0]], float(state[1]), float(state[2])
    prev = None  # (state, n, cost) of pass j - 1
    j = 0
    while True:
        good, terms = point_terms(last_buf, cur_buf, w, h, L, T, g, o, K, P, level, margins)
        S = [float(x) for x in map_tree_sum(terms)]
        n = int(good.sum())
        with np.errstate(all="ignore"):
            cost = float(f64(S[27]) / f64(n))
        if trace is not None:
            trace.append((level, j, n, cost, g, o))
        if n < 6 or not math.isfinite(cost):
            if j == 0:
                return (T, g, o), 4, 0, n, NAN
            return prev[0], 5, j - 1, prev[1], prev[2]
        if j >= 1:
            if margins is not None:
                _note(margins, "cost_b", abs(cost - prev[2]) / prev[2])
                _note(margins, "cost_c", abs((1 - cost / prev[2]) - DELTA_THRESH))
            if cost >= prev[2]:
                return prev[0], 1, j - 1, prev[1], prev[2]
            if (1 - cost / prev[2]) < DELTA_THRESH:
                return (T, g, o), 2, j, n, cost
        if j == iterations:
            return (T, g, o), 0, j, n, cost
        xi, dg, do = step(S, n)
        if not all(math.isfinite(x) for x in list(xi) + [dg, do]):
            return (T, g, o), 3, j, n, cost
        prev = ((T, g, o), n, cost)
        T, g, o = left_update(xi, T), g + dg, o + do
        j += 1


def track_affine(last_pyr, cur_pyr, w, h, K, points, pose_last, seed, iterations=10, margins=None, trace=None):
    """viso_track_affine: (pose (12,), report (24,))."""
    K = [float(x) for x in K]
    L = [float(x) for x in np.asarray(pose_last, np.float64).reshape(12)]
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    ll, ws, hs = levels(last_pyr, w, h)
    cl, _, _ = levels(cur_pyr, w, h)
    state = ([float(x) for x in np.asarray(seed, np.float64).reshape(12)], 1.0, 0.0)
    rep = np.zeros(24)
    total = 0
    for q, level in enumerate((3, 2, 1, 0)):
        state, ex, steps, n, cost = track_level(ll[level], cl[level], ws[level], hs[level], L, state, K, P, level,
                                                iterations, margins, trace)
        rep[4 + 4 * q:8 + 4 * q] = (ex, steps, n, cost)
        total += steps
    rep[0] = 2 if ex == 4 else 0
    rep[1], rep[2], rep[3] = pts.shape[0], n, cost
    rep[20], rep[21], rep[22] = state[1], state[2], total
    return np.array(state[0], np.float64), rep
