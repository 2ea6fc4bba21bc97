"""Crafted inputs for the stereo VO stage tests (tests/test_svo_cases.py on the
CPU, tests/test_svo_stages.py on the GPU): feature sets for circular matching
and match lists for the motion stage, built as data so that the edges of
`best_match` / `svo_circle_kernel` and of `svo_refine_kernel`
(viso_amd/csrc/svo.hip) are reached on purpose rather than by renderer luck.

Pure numpy; nothing here loads a library.  Every case is deterministic (own
seed).  What each case is meant to hit is *checked* by the census in
tests/test_svo_cases.py from a brute-force matcher, not assumed here.
"""
from __future__ import annotations

import numpy as np

K = (718.856, 718.856, 607.19, 185.22, 0.54)  # fx, fy, cu, cv, base of the KITTI-like rig
DESC = 32


# ====================================================================== motion stage
def synthetic_matches(motion, n=300, seed=0, noise=0.0):
    """Points in front of camera t-1 -> integer observations of both pairs."""
    rng = np.random.default_rng(seed)
    fx, fy, cu, cv, b = K
    R, t = motion[:9].reshape(3, 3), motion[9:]
    out = []
    while len(out) < n:
        Z = rng.uniform(5, 40)
        u1, v1 = rng.uniform(20, 1220), rng.uniform(20, 355)
        d1 = np.round(fx * b / Z)
        if d1 < 1:
            continue
        u1, v1 = np.round(u1), np.round(v1)
        Zq = fx * b / d1
        P = np.array([(u1 - cu) * Zq / fx, (v1 - cv) * Zq / fy, Zq])
        Q = R @ P + t
        if Q[2] <= 1:
            continue
        uL = fx * Q[0] / Q[2] + cu + rng.normal(0, noise)
        vL = fy * Q[1] / Q[2] + cv + rng.normal(0, noise)
        uR = fx * (Q[0] - b) / Q[2] + cu + rng.normal(0, noise)
        out.append([u1, v1, u1 - d1, v1, np.round(uL), np.round(vL), np.round(uR), np.round(vL)])
    return np.array(out, np.int32)


# the context parameter sets of the motion cases: (width, height, overrides);
# mcap = buckets x bucket_max = 25 x 8 x bucket_max
MOTION_CONTEXTS = {
    "default": (1242, 375, {}),                 # mcap 800
    "large": (1242, 375, {"bucket_max": 40}),   # mcap 8000: lv_out == 7 of svo_refine_kernel
}
MOTION_MCAP = {"default": 800, "large": 8000}

FORWARD = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.05, 0, 0.7], np.float64)
_a = 0.02
TURN = np.concatenate([np.array([[np.cos(_a), -np.sin(_a), 0], [np.sin(_a), np.cos(_a), 0], [0, 0, 1]]).ravel(),
                       [0.1, -0.05, 0.8]])


class MotionCase:
    """One call of the motion stage: `uv8` (M x 8 int32), sampler `frame`, the
    context (`ctx`, a key of MOTION_CONTEXTS); `kind` names the family, and
    `refused` is the error a context must answer instead of a result."""

    def __init__(self, name, uv8, frame, ctx="default", kind="size", refused=None):
        self.name, self.uv8, self.frame, self.ctx, self.kind, self.refused = name, uv8, frame, ctx, kind, refused

    def __repr__(self):
        return self.name


def _with_outliers(uv8, seed):
    """20 % gross outliers (at least one): u_l2 shifted by 20..59 px."""
    rng = np.random.default_rng(1000 + seed)
    n_bad = max(1, int(round(0.2 * len(uv8))))
    bad = rng.choice(len(uv8), n_bad, replace=False)
    uv8 = uv8.copy()
    uv8[bad, 4] += rng.integers(20, 60, n_bad).astype(np.int32)
    return uv8


DEFAULT_M = (5, 6, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 800)
LARGE_M = (4095, 4096, 4097, 8000)
# (n, noise, seed) found by search: best hypothesis count 6, refined count 5
LATE_FAILURES = ((8, 1.0, 5), (7, 1.0, 44), (8, 1.0, 51), (10, 1.0, 47), (10, 1.5, 28), (12, 1.5, 42))

# (recipe, n, noise, seed) found by search: a hypothesis with >= 6 inliers whose
# refinement system is singular, so the hypothesis is kept.  "rep3": three
# distinct matches repeated, of which the best hypothesis keeps two (a
# two-point refinement); "line": all matches on one image row at one disparity.
REFINE_FAILURES = (("rep3", 9, 1.0, 2), ("rep3", 12, 1.0, 3), ("rep3", 13, 1.0, 41), ("line", 13, 1.0, 5),
                   ("line", 6, 0.0, 14), ("line", 12, 0.5, 14))


def _degenerate_matches(recipe, n, noise, seed):
    if recipe == "rep3":
        return synthetic_matches(FORWARD, 3, seed, noise)[np.arange(n) % 3]
    uv8 = synthetic_matches(FORWARD, n, seed, noise)
    uv8[:, [1, 3, 5, 7]] = 100
    d = uv8[0, 0] - uv8[0, 2]
    uv8[:, 2], uv8[:, 6] = uv8[:, 0] - d, uv8[:, 4] - d
    return uv8


_motion_cache = None


def motion_cases():
    """All motion cases (built once, shared, never modified)."""
    global _motion_cache
    if _motion_cache is not None:
        return _motion_cache
    cases = []
    for M in DEFAULT_M:
        for noise in (0.0, 0.5):
            base = synthetic_matches(TURN, n=M, seed=M, noise=noise)
            for out in (False, True):
                uv8 = _with_outliers(base, M) if out else base
                cases.append(MotionCase(f"m{M}_noise{noise:g}{'_out' if out else ''}", uv8, M % 5))
    # the sets of M = 4095 / 4096 / 4097 are prefixes of one another's recipe
    # but not of one another's data: each is drawn with its own seed
    for M in LARGE_M:
        for noise in (0.0, 0.5):
            base = synthetic_matches(TURN, n=M, seed=M, noise=noise)
            for out in (False, True):
                uv8 = _with_outliers(base, M) if out else base
                cases.append(MotionCase(f"m{M}_noise{noise:g}{'_out' if out else ''}", uv8, M % 5, ctx="large"))
    for n, noise, seed in LATE_FAILURES:
        cases.append(MotionCase(f"late_n{n}_noise{noise:g}_seed{seed}", synthetic_matches(FORWARD, n, seed, noise),
                                seed % 5, kind="late_failure"))
    for recipe, n, noise, seed in REFINE_FAILURES:
        cases.append(MotionCase(f"refine_fail_{recipe}_n{n}_noise{noise:g}_seed{seed}",
                                _degenerate_matches(recipe, n, noise, seed), seed % 5, kind="refine_failed"))
    # two distinct matches, six times each: every 3-sample holds a repeated
    # match, so every hypothesis system is rank-deficient
    two = synthetic_matches(FORWARD, 2, seed=9)
    cases.append(MotionCase("all_fail_two_points_x6", np.tile(two, (6, 1)), 3, kind="all_fail"))
    # six exact matches: every hypothesis that solves counts all six
    cases.append(MotionCase("count_tie_m6", synthetic_matches(FORWARD, 6, seed=2), 1, kind="count_tie"))
    cases.append(MotionCase("m801_refused", synthetic_matches(TURN, 801, seed=801), 1, kind="refused",
                            refused="VISO_ERR_CAPACITY"))
    cases.append(MotionCase("m8001_refused", synthetic_matches(TURN, 8001, seed=8001), 1, ctx="large",
                            kind="refused", refused="VISO_ERR_CAPACITY"))
    _motion_cache = cases
    return cases


# ====================================================================== matching stage
class Feats:
    """A feature set as viso_svo_match takes it: u, v, cls (int32), desc
    (n x 32 u8), rows non-decreasing."""

    def __init__(self, u, v, cls, desc):
        self.u, self.v, self.cls, self.desc = u, v, cls, desc

    def __len__(self):
        return len(self.u)


L1, R1, L2, R2 = range(4)
SET_NAMES = ("L1", "R1", "L2", "R2")


class MatchCase:
    """Four feature sets and their context: image size `w`, `h` and parameter
    overrides `kw` (nms_n fixes the column-band width 64 - 2 nms_n)."""

    def __init__(self, name, w, h, f4, kw):
        self.name, self.w, self.h, self.f4, self.kw = name, w, h, f4, dict(kw)

    @property
    def ctx_key(self):
        return (self.w, self.h) + tuple(sorted(self.kw.items()))

    def __repr__(self):
        return self.name


class _Scene:
    """Builder: features are added per set in any order and sorted by row at
    the end (stable: within a row they keep the order they were added in, so a
    case decides which candidate is the last of its row)."""

    def __init__(self, name, w, h, seed, **kw):
        self.name, self.w, self.h, self.kw = name, w, h, kw
        self.D = kw.get("disp_max", 255)
        self.Rr = kw.get("match_radius", 96)
        self.rng = np.random.default_rng(seed)
        self.items = [[] for _ in range(4)]

    def desc(self):
        return self.rng.integers(0, 256, DESC, dtype=np.int64).astype(np.uint8)

    def noisy(self, d, amp):
        if amp == 0:
            return d.copy()
        return np.clip(d.astype(np.int64) + self.rng.integers(-amp, amp + 1, DESC), 0, 255).astype(np.uint8)

    def add(self, k, u, v, c, d):
        assert 0 <= u < self.w and 0 <= v < self.h and 0 <= c < 4, (self.name, SET_NAMES[k], u, v, c)
        self.items[k].append((int(u), int(v), int(c), np.asarray(d, np.uint8)))

    def track(self, u2, v2, c, d2, flow=(0, 0), d1=None, desc=None, noise=2, dvr=0):
        """One scene point seen in all four images: L2 (u2, v2), R2 d2 columns
        to its left (dvr rows below), R1 = R2 + flow, L1 d1 columns to the
        right of R1; descriptor `desc` plus independent noise per image."""
        if desc is None:
            desc = self.desc()
        if d1 is None:
            d1 = d2
        self.add(L2, u2, v2, c, self.noisy(desc, noise))
        self.add(R2, u2 - d2, v2 + dvr, c, self.noisy(desc, noise))
        self.add(R1, u2 - d2 + flow[0], v2 + dvr + flow[1], c, self.noisy(desc, noise))
        self.add(L1, u2 - d2 + flow[0] + d1, v2 + dvr + flow[1], c, self.noisy(desc, noise))

    def background(self, n, classes=(0, 1, 2, 3), rows=None, cols=None, distractors=0):
        """n random tracks (disparity 1..60, flow within +-20) and random
        unmatched features in every set."""
        lo_v, hi_v = rows if rows else (0, self.h)
        lo_u, hi_u = cols if cols else (0, self.w)
        for _ in range(n):
            d2 = int(self.rng.integers(1, 61))
            du, dv = (int(x) for x in self.rng.integers(-20, 21, 2))
            d1 = int(np.clip(d2 - du + self.rng.integers(-5, 6), 1, 80))
            u2 = int(self.rng.integers(max(lo_u, 90), hi_u))
            v2 = int(self.rng.integers(lo_v, hi_v))
            ur1, vr1 = u2 - d2 + du, v2 + dv
            if not (lo_u <= u2 - d2 and 0 <= ur1 and ur1 + d1 < self.w and lo_v <= vr1 < hi_v):
                continue
            self.track(u2, v2, int(self.rng.choice(classes)), d2, (du, dv), d1)
        for k in range(4):
            for _ in range(distractors):
                self.add(k, self.rng.integers(lo_u, hi_u), self.rng.integers(lo_v, hi_v),
                         int(self.rng.choice(classes)), self.desc())

    def finish(self, empty=None):
        f4 = []
        for k in range(4):
            it = [] if k == empty else self.items[k]
            order = np.argsort(np.array([x[1] for x in it], np.int64), kind="stable") if it else []
            it = [it[i] for i in order]
            f4.append(Feats(np.array([x[0] for x in it], np.int32), np.array([x[1] for x in it], np.int32),
                            np.array([x[2] for x in it], np.int32),
                            np.array([x[3] for x in it], np.uint8).reshape(len(it), DESC)))
        return MatchCase(self.name, self.w, self.h, f4, self.kw)


# the common small context: 54-column bands (nms_n 5), 640 = 11 bands + 46 columns
W0, H0 = 640, 200
KW0 = dict(max_features=2048)
QU, QV = 400, 100  # the crafted query of the tie / dense cases: window columns 145..400 = bands 2..7


def _bump(d, byte, by):
    d = d.copy()
    d[byte] = d[byte] + by
    return d


def _case_tie():
    s = _Scene("tie_index_vs_band", W0, H0, 11, **KW0)
    # (a) class 0: three R2 candidates with one descriptor (SAD 6 to the
    # query); the lowest index (row 99) lies in band 7, the later rows in
    # bands 3 and 2, which the band-major scan meets first
    q = np.clip(s.desc(), 0, 200)
    t = _bump(q, 3, 6)
    s.add(L2, QU, QV, 0, q)
    s.add(R2, 395, 99, 0, t)
    s.add(R2, 200, 100, 0, t)
    s.add(R2, 150, 101, 0, t)
    s.add(R1, 400, 102, 0, t)
    s.add(L1, 406, 102, 0, t)
    # (b) class 1: two tied candidates inside one band (7), rows 99 and 100
    q = np.clip(s.desc(), 0, 200)
    t = _bump(q, 5, 9)
    s.add(L2, QU, QV, 1, q)
    s.add(R2, 390, 99, 1, t)
    s.add(R2, 385, 100, 1, t)
    s.add(R1, 386, 95, 1, t)
    s.add(L1, 396, 95, 1, t)
    # (c) class 2: the tie straddles the halves of a 128-candidate step: the
    # later index in slot 0 (band 2, row 101), 70 others, the earlier index
    # (band 7, row 99) in slot 71; (d) class 3: 63 others, slots 0 and 64
    # (one lane holds both)
    for c, fill in ((2, 70), (3, 63)):
        q = np.clip(s.desc(), 0, 200)
        t = _bump(q, 7, 4)
        s.add(L2, QU, QV, c, q)
        s.add(R2, 395, 99, c, t)
        for i in range(fill):
            s.add(R2, 162 + (i * 7) % 162, 99 + i % 3, c, s.desc())
        s.add(R2, 150, 101, c, t)
        s.add(R1, 400, 103, c, t)
        s.add(L1, 404, 103, c, t)
    # (e) the closing search: two L2 features with one descriptor reach the
    # same R2 feature; L1 -> L2 ties and returns the lower, which alone closes
    e = s.desc()
    s.add(L2, 300, 30, 0, e)
    s.add(L2, 310, 31, 0, e)
    s.add(R2, 290, 30, 0, e)
    s.add(R1, 288, 28, 0, e)
    s.add(L1, 299, 28, 0, e)
    s.background(30, rows=(140, 200), distractors=10)
    return s.finish()


def _case_dense(n):
    """Exactly n class-0 candidates in rows 99..101 of bands 2..7 of R2 (the
    window of the L2 query at (400, 100)); the match is the last of row 101 in
    band 7, i.e. the last slot of the concatenated list."""
    s = _Scene(f"dense_{n}", W0, H0, 100 + n, **KW0)
    q = s.desc()
    s.add(L2, QU, QV, 0, s.noisy(q, 2))
    cells = [(u, v) for v in (99, 100, 101) for u in range(108, 432) if (u, v) != (390, 101)]
    for i in s.rng.choice(len(cells), n - 1, replace=False):
        s.add(R2, cells[i][0], cells[i][1], 0, s.desc())
    s.add(R2, 390, 101, 0, s.noisy(q, 2))
    s.add(R1, 395, 110, 0, s.noisy(q, 2))
    s.add(L1, 404, 110, 0, s.noisy(q, 2))
    s.background(20, classes=(1, 2, 3), distractors=10)
    return s.finish()


def _case_bands8():
    """nms_n 8: 48-column bands, disp_max 335 = the widest window svo_check
    admits (8 bands unless it starts on a band edge).  Disparities 1..335 in
    both stereo searches."""
    s = _Scene("bands8", 720, 120, 21, nms_n=8, disp_max=335, max_features=2048)
    disps = (1, 2, 47, 48, 100, 200, 287, 300, 334, 335)
    for i, d2 in enumerate(disps):
        d1 = disps[len(disps) - 1 - i]
        # L2 at 340 + ..: the R2 window starts at column >= 5; L1 = R1 + d1 < 720
        u2 = 345 + 3 * i
        ur1 = u2 - d2 + 4
        if ur1 + d1 >= 720 or abs(d2 - 4 - d1) > 96:
            d1 = int(np.clip(d2 - 4, 1, 335))
        s.track(u2, 10 + 10 * i, i % 4, d2, (4, 2), d1)
    s.background(40, distractors=40)
    return s.finish()


def _case_clamp_left():
    s = _Scene("clamp_left", W0, H0, 31, **KW0)
    for i, (u2, d2) in enumerate(((1, 1), (10, 3), (54, 20), (100, 100), (200, 199), (254, 1), (30, 29))):
        s.track(u2, 20 + 20 * i, i % 4, d2, (3 if u2 - d2 + 3 < W0 else 0, 1), None)
    s.background(20, cols=(0, 300), distractors=20)
    return s.finish()


def _case_clamp_right():
    s = _Scene("clamp_right", W0, H0, 32, **KW0)  # 640 = 11 x 54 + 46: the last band is partial
    for i, (u2, d2) in enumerate(((639, 10), (620, 30), (600, 5), (594, 1), (545, 1), (560, 12))):
        s.track(u2, 20 + 25 * i, i % 4, d2, (2, -1), d2 + 1 if u2 - d2 + 2 + d2 + 1 < W0 else d2 - 2)
    s.background(20, cols=(400, W0), distractors=20)
    return s.finish()


def _case_clamp_rows():
    s = _Scene("clamp_rows", W0, H0, 33, **KW0)
    h = H0
    # (v2, dvr, flow dv): rows 0 / h - 1 in every image in turn
    for i, (v2, dvr, dv) in enumerate(((0, 0, 0), (0, 1, -1), (1, -1, 0), (h - 1, 0, 0), (h - 1, -1, 1),
                                       (h - 2, 1, 0), (50, 0, -50), (150, 0, 49))):
        s.track(100 + 60 * i, v2, i % 4, 10 + i, (3, dv), 12 + i, dvr=dvr)
    s.background(20, distractors=20)
    return s.finish()


def _case_short_image():
    s = _Scene("short_image", W0, 40, 34, **KW0)  # 40 rows < 2 x 96 + 1: both row clamps at once
    for i, v2 in enumerate((0, 1, 20, 38, 39)):
        s.track(150 + 90 * i, v2, i % 4, 15 + i, (-5, 0), 14 + i)
    s.background(30, distractors=20)
    return s.finish()


def _base_scene(name, seed, classes=(0, 1, 2, 3)):
    s = _Scene(name, W0, H0, seed, **KW0)
    s.background(60, classes=classes, distractors=20)
    return s


def _case_class_absent():
    s = _base_scene("class_absent", 41, classes=(0, 2, 3))
    # class-1 queries: L2 (and L1, R1) hold the class, R2 does not
    for i in range(4):
        d = s.desc()
        s.add(L2, 200 + 50 * i, 40 + 30 * i, 1, d)
        s.add(R1, 190 + 50 * i, 40 + 30 * i, 1, d)
        s.add(L1, 200 + 50 * i, 40 + 30 * i, 1, d)
    return s.finish()


def _case_zero_disparity():
    s = _base_scene("zero_disparity_winner", 42)
    # current pair: the SAD winner sits at disparity 0, a worse candidate at 5
    d = np.clip(s.desc(), 0, 200)
    s.add(L2, 300, 50, 0, d)
    s.add(R2, 300, 50, 0, d)
    s.add(R2, 295, 50, 0, _bump(d, 0, 40))
    s.add(R1, 303, 52, 0, d)
    s.add(L1, 310, 52, 0, d)
    # previous pair: the same at R1 -> L1
    d = np.clip(s.desc(), 0, 200)
    s.add(L2, 300, 150, 1, d)
    s.add(R2, 290, 150, 1, d)
    s.add(R1, 292, 148, 1, d)
    s.add(L1, 292, 148, 1, d)
    s.add(L1, 299, 148, 1, _bump(d, 0, 40))
    return s.finish()


def _case_index_32767():
    """R2 holds 32768 features (max_features 32768): fillers in rows 0..190,
    the queried ones in rows 198 / 199; the last feature (index 32767) is the
    unique winner of one query and the tied loser of another."""
    s = _Scene("index_32767", W0, H0, 51, max_features=32768)
    base = np.clip(s.desc(), 0, 200)
    # query 1 (300, 199): window 45..300 holds index 32767 at (290, 199) only
    s.add(L2, 300, 199, 0, base)
    s.add(R1, 292, 197, 0, base)
    s.add(L1, 303, 197, 0, base)
    # query 2 (500, 198): window 245..500 holds (450, 198) [descriptor + 8]
    # and index 32767 [descriptor + 0]; its own descriptor + 4 ties them
    s.add(L2, 500, 198, 0, _bump(base, 0, 4))
    s.add(R2, 450, 198, 0, _bump(base, 0, 8))
    s.add(R1, 452, 196, 0, _bump(base, 0, 8))
    s.add(L1, 500, 196, 0, _bump(base, 0, 8))
    s.background(10, rows=(192, 200), classes=(1, 2, 3))
    n_fill = 32768 - len(s.items[R2]) - 1
    rng = s.rng
    fu, fv = rng.integers(0, W0, n_fill), rng.integers(0, 191, n_fill)
    fc, fd = rng.integers(0, 4, n_fill), rng.integers(0, 256, (n_fill, DESC), dtype=np.int64).astype(np.uint8)
    for i in range(n_fill):
        s.items[R2].append((int(fu[i]), int(fv[i]), int(fc[i]), fd[i]))
    s.add(R2, 290, 199, 0, base)  # added last into the last row: index 32767
    return s.finish()


_match_cache = None


def match_cases():
    """All matching cases (built once, shared, never modified)."""
    global _match_cache
    if _match_cache is None:
        cases = [_case_tie()]
        cases += [_case_dense(n) for n in (64, 65, 128, 129, 256, 257, 400)]
        cases += [_case_bands8(), _case_clamp_left(), _case_clamp_right(), _case_clamp_rows(), _case_short_image()]
        for k in range(4):
            s = _base_scene("empty_" + SET_NAMES[k], 60 + k)
            cases.append(s.finish(empty=k))
        cases += [_case_class_absent(), _case_zero_disparity(), _case_index_32767()]
        _match_cache = cases
    return _match_cache
