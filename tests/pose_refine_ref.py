"""TEST INFRASTRUCTURE ONLY — Python restatement of the pose refinement
(viso_set_pose_refine / viso_refine_pose, include/viso/viso_c.h; DESIGN.md
§Pose refinement).  The repo's own spec: the reference computes the
LK-aligned feature positions (src/viso.cpp:121) and only draws them
(src/viso.cpp:123-135).

Every expression is scalar Python float (fp64) arithmetic in the device's
operand order, that of tests/mono_kf_ref.py: a 3-term dot product is
(a0 b0 + a1 b1) + a2 b2, nothing is contracted.  Poses are Tcw, 12 doubles
(R row-major, t): Pc = R Pw + t.

Summation order (DESIGN.md §Pose refinement, "The sums"): lane l of 1,024
takes the points i = l, l + 1024, ... in ascending i, each sum starting at
+0.0; the 1,024 lane values are then added pairwise, neighbours first
(0+1, 2+3, ...), level by level, down to one value.
"""
from __future__ import annotations

import math

import numpy as np

from tests.mono_kf_ref import mat_vec

LANES = 1024
N_SUMS = 29  # H upper triangle (21, row-major), b (6), cost, sum of e^2


class Margin:
    """The smallest distance of each kind of decision from its threshold:
    shift (the squared LK shift against max_shift_px^2), z (Pc.z against 0),
    huber (e against huber_px), cost (|cost_k - cost_{k-1}| / cost_{k-1}) and
    count (n_0 against 6, at least 0.5 for integers)."""

    def __init__(self):
        self.shift = self.z = self.huber = self.cost = float("inf")

    def note(self, kind, d):
        if d < getattr(self, kind):
            setattr(self, kind, d)

    @property
    def value(self):
        return min(self.shift, self.z, self.huber, self.cost)


# ------------------------------------------------------------------ SE(3)
def quat_from_matrix(m):
    t = (m[0] + m[4]) + m[8]
    q = [0.0] * 4
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[3 * i + i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[3 * i + i] - m[3 * j + j] - m[3 * k + k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return q


def quat_to_matrix(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def quat_mul(a, b):
    w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    return [x, y, z, w]


def quat_rotate(q, v):
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    c0 = q[1] * uv[2] - q[2] * uv[1]
    c1 = q[2] * uv[0] - q[0] * uv[2]
    c2 = q[0] * uv[1] - q[1] * uv[0]
    return [v[0] + q[3] * uv[0] + c0, v[1] + q[3] * uv[1] + c1, v[2] + q[3] * uv[2] + c2]


def se3_mul(aq, at, bq, bt):
    rt = quat_rotate(aq, bt)
    t = [at[0] + rt[0], at[1] + rt[1], at[2] + rt[2]]
    q = quat_mul(aq, bq)
    sq = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    if sq != 1.0:
        f = 2.0 / (1.0 + sq)
        q = [x * f for x in q]
    return q, t


def se3_exp(a):
    """Sophus SE3::exp of a = [upsilon; omega] as device_math.hpp states it:
    (quaternion xyzw, translation)."""
    eps = 1e-10
    w = a[3:6]
    theta_sq = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    theta = math.sqrt(theta_sq)
    half_theta = 0.5 * theta
    if theta < eps:
        theta_po4 = theta_sq * theta_sq
        imag = 0.5 - (1.0 / 48.0) * theta_sq + (1.0 / 3840.0) * theta_po4
        real = 1.0 - 0.5 * theta_sq + (1.0 / 384.0) * theta_po4
    else:
        imag = math.sin(half_theta) / theta
        real = math.cos(half_theta)
    q = [imag * w[0], imag * w[1], imag * w[2], real]
    if theta < eps:
        V = quat_to_matrix(q)
    else:
        O = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
        O2 = [(O[3 * i + 0] * O[0 + j] + O[3 * i + 1] * O[3 + j]) + O[3 * i + 2] * O[6 + j]
              for i in range(3) for j in range(3)]
        th2 = theta * theta
        c1 = (1.0 - math.cos(theta)) / th2
        c2 = (theta - math.sin(theta)) / (th2 * theta)
        V = [((1.0 if i % 4 == 0 else 0.0) + c1 * O[i]) + c2 * O2[i] for i in range(9)]
    return q, mat_vec(V, a[0:3])


def left_update(xi, pose):
    """exp(xi) * pose (12 doubles): the pose's rotation as a quaternion, the
    Sophus product, back to a matrix."""
    eq, et = se3_exp(xi)
    q, t = se3_mul(eq, et, quat_from_matrix(pose[:9]), list(pose[9:12]))
    return quat_to_matrix(q) + t


def inverse6(Hin):
    """Eigen's 6x6 inverse() through PartialPivLU, as device_math.hpp."""
    lu = list(Hin)
    tr = [0] * 6
    for k in range(6):
        p = k
        best = abs(lu[6 * k + k])
        for i in range(k + 1, 6):
            s = abs(lu[6 * i + k])
            if s > best:
                best = s
                p = i
        tr[k] = p
        if best != 0.0:
            if p != k:
                for j in range(6):
                    lu[6 * k + j], lu[6 * p + j] = lu[6 * p + j], lu[6 * k + j]
            for i in range(k + 1, 6):
                lu[6 * i + k] = _div(lu[6 * i + k], lu[6 * k + k])
        for i in range(k + 1, 6):
            for j in range(k + 1, 6):
                lu[6 * i + j] = lu[6 * i + j] - lu[6 * i + k] * lu[6 * k + j]
    x = [1.0 if i % 7 == 0 else 0.0 for i in range(36)]
    for k in range(6):
        if tr[k] != k:
            for j in range(6):
                x[6 * k + j], x[6 * tr[k] + j] = x[6 * tr[k] + j], x[6 * k + j]
    for c in range(6):
        for j in range(6):
            for i in range(j + 1, 6):
                x[6 * i + c] = x[6 * i + c] - lu[6 * i + j] * x[6 * j + c]
        for j in range(5, -1, -1):
            x[6 * j + c] = _div(x[6 * j + c], lu[6 * j + j])
            for i in range(j):
                x[6 * i + c] = x[6 * i + c] - lu[6 * i + j] * x[6 * j + c]
    return x


def _div(a, b):
    """IEEE division (a zero divisor gives inf / nan instead of raising)."""
    return float(np.float64(a) / np.float64(b))


# ------------------------------------------------------------------ the sums
def tree_sum(vals):
    """Neighbours first, level by level (a power-of-two count)."""
    v = list(vals)
    while len(v) > 1:
        v = [v[2 * i] + v[2 * i + 1] for i in range(len(v) // 2)]
    return v[0]


def point_terms(P, uv, pose, K, huber, margin=None):
    """One observation at `pose`: None when Pc.z <= 0, else (the 29 terms in
    sum order, inlier flag)."""
    fx, fy, cx, cy = K
    Pc = mat_vec(pose[:9], P)
    x, y, z = Pc[0] + pose[9], Pc[1] + pose[10], Pc[2] + pose[11]
    if margin is not None:
        margin.note("z", abs(z))
    if not z > 0:
        return None
    r0 = uv[0] - (fx * x / z + cx)
    r1 = uv[1] - (fy * y / z + cy)
    e2 = r0 * r0 + r1 * r1
    e = math.sqrt(e2)
    if margin is not None:
        margin.note("huber", abs(e - huber))
    zz, xy = z * z, x * y
    J = [fx / z, 0.0, -fx * x / zz, -fx * xy / zz, fx + fx * x * x / zz, -fx * y / z,
         0.0, fy / z, -fy * y / zz, -fy - fy * y * y / zz, fy * xy / zz, fy * x / z]
    inl = e <= huber
    w = 1.0 if inl else huber / e
    rho = 0.5 * e2 if inl else huber * (e - 0.5 * huber)
    t = []
    for a in range(6):
        for b in range(a, 6):
            t.append(w * (J[a] * J[b] + J[6 + a] * J[6 + b]))
    for a in range(6):
        t.append(w * (J[a] * r0 + J[6 + a] * r1))
    t.append(rho)
    t.append(e2)
    return t, inl


def observations(pair_kf, success, uv_before, uv_after, max_shift_px, margin=None):
    m2 = max_shift_px * max_shift_px
    obs = []
    for i in range(len(pair_kf)):
        if not (pair_kf[i] >= 0 and success[i] != 0):
            continue
        d0 = uv_after[i][0] - uv_before[i][0]
        d1 = uv_after[i][1] - uv_before[i][1]
        d2 = d0 * d0 + d1 * d1
        if margin is not None and d2 == d2:
            margin.note("shift", abs(d2 - m2))
        if d2 <= m2:
            obs.append(i)
    return obs


def pass_sums(P, uv, obs, pose, K, huber, margin=None, order=None):
    """(S[29], n used, inliers) of one pass.  order: None = the device's
    (lanes, then the tree); else a permutation of obs summed left to right
    (the sensitivity test)."""
    n = inl = 0
    if order is not None:
        S = [0.0] * N_SUMS
        for i in order:
            r = point_terms(P[i], uv[i], pose, K, huber, margin)
            if r is None:
                continue
            n += 1
            inl += 1 if r[1] else 0
            for k in range(N_SUMS):
                S[k] = S[k] + r[0][k]
        return S, n, inl
    lanes = [[0.0] * N_SUMS for _ in range(LANES)]
    for i in obs:  # ascending i: each lane's points in ascending order
        r = point_terms(P[i], uv[i], pose, K, huber, margin)
        if r is None:
            continue
        n += 1
        inl += 1 if r[1] else 0
        acc = lanes[i % LANES]
        for k in range(N_SUMS):
            acc[k] = acc[k] + r[0][k]
    return [tree_sum([lanes[l][k] for l in range(LANES)]) for k in range(N_SUMS)], n, inl


def solve(S):
    """xi = H^-1 b from a pass's sums (H's upper triangle mirrored)."""
    H = [0.0] * 36
    k = 0
    for a in range(6):
        for b in range(a, 6):
            H[6 * a + b] = S[k]
            H[6 * b + a] = S[k]
            k += 1
    with np.errstate(all="ignore"):
        Hi = inverse6(H)
        xi = []
        for a in range(6):
            s = Hi[6 * a] * S[21]
            for b in range(1, 6):
                s = s + Hi[6 * a + b] * S[21 + b]
            xi.append(s)
    return xi


def refine(points, pair_kf, success, uv_before, uv_after, pose_in, K, iterations, huber_px, max_shift_px,
           permute_seed=None):
    """The refinement of one frame.  Returns a dict: pose (12,), report (8,)
    = [observations, steps applied, cost_0, cost at the result, inliers at
    the result, status, rms at T_0, rms at the result], passes (per pass: n
    used, cost, inliers), margin (Margin).  permute_seed: sum every pass in a
    shuffled order instead of the device's (the sensitivity test)."""
    K = [float(x) for x in K]
    P = np.asarray(points, np.float64).reshape(-1, 3).tolist()
    pk = [int(x) for x in np.asarray(pair_kf).reshape(-1)]
    sc = [int(x) for x in np.asarray(success).reshape(-1)]
    ub = np.asarray(uv_before, np.float64).reshape(-1, 2).tolist()
    ua = np.asarray(uv_after, np.float64).reshape(-1, 2).tolist()
    X = [float(x) for x in np.asarray(pose_in, np.float64).reshape(12)]
    huber, shift = float(huber_px), float(max_shift_px)
    margin = Margin()
    obs = observations(pk, sc, ub, ua, shift, margin)
    rng = np.random.default_rng(permute_seed) if permute_seed is not None else None

    def rms_of(S, n):
        return math.sqrt(S[28] / n) if n > 0 else 0.0

    T = X
    prev = None  # (pose, cost, inliers, rms) of pass k - 1
    passes = []
    k = 0
    while True:
        order = [obs[j] for j in rng.permutation(len(obs))] if rng is not None else None
        S, n, inl = pass_sums(P, ua, obs, T, K, huber, margin, order)
        cost, rms = S[27], rms_of(S, n)
        passes.append((n, cost, inl))
        if k == 0:
            cost0, rms0 = cost, rms
            if n < 6:
                res, status, steps, stats = X, 1, 0, (cost, inl, rms)
                break
        if k >= 1:
            if prev[1] > 0:
                margin.note("cost", abs(cost - prev[1]) / prev[1])
            if cost >= prev[1]:
                res, status, steps, stats = prev[0], 3, k - 1, prev[1:]
                break
        if k == iterations:
            res, status, steps, stats = T, 0, k, (cost, inl, rms)
            break
        xi = solve(S)
        if not all(math.isfinite(v) for v in xi):
            res, status, steps, stats = T, 2, k, (cost, inl, rms)
            break
        prev = (T, cost, inl, rms)
        T = left_update(xi, T)
        k += 1
    report = [float(len(obs)), float(steps), cost0, stats[0], float(stats[1]), float(status), rms0, stats[2]]
    return {"pose": np.array(res, np.float64), "report": np.array(report, np.float64), "passes": passes,
            "margin": margin, "observations": obs}
