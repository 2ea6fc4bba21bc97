"""TEST INFRASTRUCTURE ONLY — numpy restatement of the keyframe alignment with
an affine brightness map per candidate (viso_kf_align_illum,
viso_set_reloc_illum; include/viso/viso_c.h).  The repo's own
spec, composed from the restatements it extends:

* the points, the candidates, the report and the winner are the keyframe
  alignment's (kf_align_ref: select_points, pick_winner, §19's steps 1 and 5);
* a good point's 44 terms are bright_ref.point_terms with keyframe k's level
  image as "last" and keyframe k's pose as L, e = (g_j R + o_j) - C;
* across points §19's order, not the map tree: list position p adds its terms
  to accumulator p mod 16 in ascending p, the 16 accumulators are added
  neighbours first (kf_align_ref.pass_sums, column by column);
* the step is bright_ref.step (d11 = 64 n_j), the decisions are
  bright_ref.track_level's on the state (T, g, o);
* the status adds 5 between 3 and 4: not (1 / max_gain <= g <= max_gain).

``margins`` has kf_align_ref's keys and ``gain``: the smallest relative
distance of a judged g from either bound.
"""
from __future__ import annotations

import math

import numpy as np

from tests import bright_ref as br, kf_align_ref as ka
from tests.kf_align_ref import DELTA_THRESH, NAN, _note
from tests.lk_warp_ref import levels
from tests.pose_refine_ref import left_update

N_TERMS = br.N_TERMS  # 44
f64 = np.float64


def pass_sums(good, terms):
    """(S[44], n) in §19's order: kf_align_ref.pass_sums adds every column on
    its own, so the 44 columns go through it as two overlapping sets of 28."""
    lo, n = ka.pass_sums(good, terms[:, :ka.N_TERMS])
    hi, _ = ka.pass_sums(good, terms[:, N_TERMS - ka.N_TERMS:])
    return lo + hi[2 * ka.N_TERMS - N_TERMS:], n


def align_level(kf_buf, cur_buf, w, h, kf_pose, state, K, P, level, iterations, margins=None, trace=None):
    """One level from state = (T, g, o): (kept state, exit, steps applied, n,
    cost) — bright_ref.track_level with pass_sums for the map tree."""
    T, g, o = [float(x) for x in state[0]], float(state[1]), float(state[2])
    prev = None  # (state, n, cost) of pass j - 1
    j = 0
    while True:
        good, terms = br.point_terms(kf_buf, cur_buf, w, h, kf_pose, T, g, o, K, P, level, margins)
        S, n = pass_sums(good, terms)
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
        xi, dg, do = br.step(S, n)
        if not all(math.isfinite(x) for x in list(xi) + [dg, do]):
            return (T, g, o), 3, j, n, cost
        prev = ((T, g, o), n, cost)
        T, g, o = left_update(xi, T), g + dg, o + do
        j += 1


def align_candidate(kf_pyr, kf_pose, cur_pyr, w, h, K, points, seed, iterations, max_points, max_cost,
                    min_good_permille, max_gain, margins=None, trace=None):
    """One candidate: (pose (12,), report (20,), (g, o))."""
    K = [float(x) for x in K]
    kf_pose = [float(x) for x in np.asarray(kf_pose, np.float64).reshape(12)]
    seed = [float(x) for x in np.asarray(seed, np.float64).reshape(12)]
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    idx = ka.select_points(pts, kf_pose, K, w, h, max_points, margins)
    m = int(idx.size)
    rep = np.full(20, NAN)
    rep[1] = m
    if m < 6:
        rep[0], rep[2] = 1, 0
        for q in range(4):
            rep[4 + 4 * q:7 + 4 * q] = (-1, 0, 0)
        return np.array(seed), rep, (1.0, 0.0)
    P = (pts[idx, 0], pts[idx, 1], pts[idx, 2])
    kl, ws, hs = levels(kf_pyr, w, h)
    cl, _, _ = levels(cur_pyr, w, h)
    state = (seed, 1.0, 0.0)
    for q, level in enumerate((3, 2, 1, 0)):
        state, ex, steps, n, cost = align_level(kl[level], cl[level], ws[level], hs[level], kf_pose, state, K, P, level,
                                                iterations, margins, trace)
        rep[4 + 4 * q:8 + 4 * q] = (ex, steps, n, cost)
    rep[2], rep[3] = n, cost
    g = state[1]
    lo = float(f64(1.0) / f64(max_gain))
    if ex == 4:
        rep[0] = 2
    elif n * 1000 < min_good_permille * m:
        rep[0] = 3
    elif not (lo <= g and g <= max_gain):
        rep[0] = 5
    elif not (cost <= max_cost):
        rep[0] = 4
    else:
        rep[0] = 0
    if margins is not None and ex != 4:
        _note(margins, "max_cost", abs(cost - max_cost) / max_cost)
        _note(margins, "gain", min(abs(g - lo) / lo, abs(g - max_gain) / max_gain))
    return np.array(state[0], np.float64), rep, (state[1], state[2])


def kf_align_illum(kf_pyrs, kf_poses, cur_pyr, w, h, K, points, extra_seed=None, iterations=10, max_points=512,
                   max_cost=57600.0, min_good_permille=500, max_gain=4.0, margins=None, trace=None):
    """viso_kf_align_illum: dict(poses (n_cand, 12), report (n_cand, 20),
    gain_offset (n_cand, 2), winner); the candidates as in kf_align_ref."""
    kf_poses = np.asarray(kf_poses, np.float64).reshape(-1, 12)
    seeds = [None] if extra_seed is None else [None, np.asarray(extra_seed, np.float64).reshape(12)]
    poses, reps, gos = [], [], []
    for k in range(kf_poses.shape[0]):
        for s in seeds:
            tr = None if trace is None else []
            pose, rep, go = align_candidate(kf_pyrs[k], kf_poses[k], cur_pyr, w, h, K, points,
                                            kf_poses[k] if s is None else s, iterations, max_points, max_cost,
                                            min_good_permille, max_gain, margins, tr)
            if trace is not None:
                trace.append(tr)
            poses.append(pose)
            reps.append(rep)
            gos.append(go)
    report = np.array(reps).reshape(-1, 20)
    return {"poses": np.array(poses).reshape(-1, 12), "report": report,
            "gain_offset": np.array(gos, np.float64).reshape(-1, 2), "winner": ka.pick_winner(report, margins)}
