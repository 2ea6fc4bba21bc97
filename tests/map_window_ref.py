"""TEST INFRASTRUCTURE ONLY — Python restatement of one retirement of the
sliding-window map (viso_set_map_window / viso_map_retire,
include/viso/viso_c.h; DESIGN.md §Sliding-window map).  The repo's own spec:
the reference's map (src/viso.cpp:79-96) never loses a point.

Every expression is scalar Python float (fp64) arithmetic in the device's
operand order, that of tests/mono_kf_ref.py: a 3-term dot product is
(a0 b0 + a1 b1) + a2 b2, nothing is contracted.  Poses are Tcw, 12 doubles
(R row-major, t): Pc = R Pw + t.
"""
from __future__ import annotations

import numpy as np

from tests.mono_kf_ref import mat_vec


class Margin:
    """The smallest distance of any decision from its threshold: z against 0,
    u and v against the image bounds, and (for the check frame, whose cells
    are used) u / cell and v / cell against an integer."""

    def __init__(self):
        self.value = float("inf")

    def note(self, d):
        if d < self.value:
            self.value = d


def project(pose, P, K):
    """(u, v, z) of P under pose; u and v are None when z is not positive."""
    Pc = mat_vec(pose[:9], P)
    Pc = [Pc[r] + pose[9 + r] for r in range(3)]
    if not Pc[2] > 0:
        return None, None, Pc[2]
    return K[0] * Pc[0] / Pc[2] + K[2], K[1] * Pc[1] / Pc[2] + K[3], Pc[2]


def seen_cell(pose, P, K, width, height, cell, margin=None, cells=False):
    """The cell (cx, cy) of the image grid that pose sees P in, or None: P in
    front of the camera and inside the image."""
    u, v, z = project(pose, P, K)
    if margin is not None:
        margin.note(abs(z))
    if u is None:
        return None
    if margin is not None:
        for d in (abs(u), abs(u - width), abs(v), abs(v - height)):
            margin.note(d)
    if not (0 <= u < width and 0 <= v < height):
        return None
    if margin is not None and cells:
        for q in (u / cell, v / cell):
            margin.note(abs(q - round(q)))
    return int(u / cell), int(v / cell)


def retire(points, host, pose_c, kf_poses, K, width, height, cell):
    """Keyframe 0 of kf_poses (n_kf, 12) is retired with check frame c.
    points (n, 3) world, host (n,) keyframe indices.  Returns a dict: keep
    (n,) uint8, points / host (the kept points in order with their new
    hosts), counts [retired-host, of those seen by c, candidates, survivors],
    margin (the smallest distance of a decision from its threshold)."""
    K = [float(x) for x in K]
    pc = [float(x) for x in np.asarray(pose_c, np.float64).reshape(12)]
    kfs = [[float(x) for x in row] for row in np.asarray(kf_poses, np.float64).reshape(-1, 12)]
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    P = pts.tolist()
    hst = [int(h) for h in np.asarray(host).reshape(-1)]
    n, n_kf = len(P), len(kfs)
    assert len(hst) == n
    margin = Margin()
    # every point's cell in c; the live ones mark theirs
    cell_of = [seen_cell(pc, P[i], K, width, height, cell, margin, cells=True) for i in range(n)]
    marked = {cell_of[i] for i in range(n) if hst[i] != 0 and cell_of[i] is not None}
    # retired-host points: candidates claim their cell, the highest index wins
    new_host = [h - 1 for h in hst]
    winner = {}
    n_retired = n_visible = n_cand = 0
    for i in range(n):
        if hst[i] != 0:
            continue
        n_retired += 1
        new_host[i] = -1
        c = cell_of[i]
        if c is None:
            continue
        n_visible += 1
        if c in marked:
            continue
        for k in range(n_kf - 1, 0, -1):  # newest first
            if seen_cell(kfs[k], P[i], K, width, height, cell, margin) is not None:
                new_host[i] = k - 1
                break
        if new_host[i] < 0:
            continue
        n_cand += 1
        if i > winner.get(c, -1):
            winner[c] = i
    keep = np.zeros(n, np.uint8)
    for i in range(n):
        if hst[i] != 0 or (new_host[i] >= 0 and winner.get(cell_of[i]) == i):
            keep[i] = 1
    idx = np.nonzero(keep)[0]
    n_surv = sum(1 for i in idx if hst[i] == 0)
    return {"keep": keep, "points": pts[idx].copy(), "host": np.array([new_host[i] for i in idx], np.int32),
            "counts": [n_retired, n_visible, n_cand, n_surv], "margin": margin.value}
