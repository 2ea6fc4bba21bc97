"""TEST INFRASTRUCTURE ONLY — inputs for the direct-pose branch tests and a
CPU census of the branches direct_level_kernel (viso_amd/csrc/direct.hip)
takes on them.

The kernel's contract is bit-identity with the oracle; what keeps it is a set
of data-dependent branches (direct_point_rs, sample_cw, win_issue,
direct_tile_pf, prefetch_tile, tile_range).  The census predicts, from the
oracle alone, which branch every good point of a case takes at every pyramid
level, so the tests can prove that their inputs reach each branch and, on a
mismatch, name the branches the failing case populates.

Branch map of one good point at level l (w x h the level's size):

* The 20 x 20 LDS window of the current image is loaded around the point's
  projection (up, vp) under a *predicted* pose — the pose level l + 1 started
  from (the seed for level 3): x0 = clamp(floor(up) - 9, 0, w - 20), likewise
  y0.  A level smaller than 20 px in either direction has no window
  (``win_off``): every sample reads global memory.
* With (uc, vc) the projection under the level's starting pose and
  fu = floor(uc), fv = floor(vc), the patch is ``whole`` in the window when
  fu - 6 >= x0, fu + 5 <= x0 + 18, and the same in v.
  - ``shared``: whole, and uc - 6, uc + 6 (and vc's) lie in one binade: one
    set of bilinear weights, 12 taps per lane.
  - ``straddle``: whole, but uc +- 6 or vc +- 6 straddles a power of two: the
    per-sample LDS form.
* Not whole: sample_cw decides per sample (``per_sample``).  A sample with
  base (ix, iy) = (int(x), int(y)) is served from the window when
  x0 <= ix <= x0 + 18 and y0 <= iy <= y0 + 18; the bases of one point span
  [fu - 5, fu + 4] x [fv - 5, fv + 4].
  - ``edge_lt``: uc < 5 or vc < 5: gradient taps at coordinates in (-1, 0),
    where int() != floor().
  - ``edge_r``: uc >= w - 5: base ix = w - 1, whose tap ix + 1 = w would wrap
    into the next row: sample_px's global path.
  - ``edge_b``: vc >= h - 5: base iy = h - 1, the branch with two zero taps.
  - ``full_miss``: no base is served (the predicted window and the patch are
    disjoint): all 320 samples read global memory.
  - ``partial_miss``: some bases are served and some are not, on a side where
    the window is not clamped to the image border — the prediction, not the
    border, put them outside.
  full_miss and partial_miss need the level above to move the projection by
  more than about 4 px: one large Gauss-Newton step.

The census looks at the first iteration of each level (the tile phase of the
level's launch); later iterations of a level re-centre the windows on the
current pose.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import images, oracle_lib

LEVELS = 4
SCALES = (1.0, 0.5, 0.25, 0.125)
WIN = 20  # direct.hip kCW
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
CLASSES = ("shared", "straddle", "per_sample", "edge_lt", "edge_r", "edge_b", "partial_miss", "full_miss",
           "win_off")

# (w, h, (sx, sy), n, seed, scale, near)
CASES = {
    "gentle": (320, 240, (3, 2), 2465, 0, 12, 0.5),          # every whole-patch and edge class, T = 10
    "small_l3": (320, 152, (16, 0), 4097, 0, 12, 0.5),       # level 3 is 40 x 19: no window; T = 17
    "odd_t64": (333, 251, (20, -12), 16384, 0, 12, 0.5),     # truncated odd level sizes; T = 64
    "big_step": (640, 480, (64, 0), 3321, 0, 128, 0.5),      # prediction misses at levels 0-2; T = 13
    "big_step_far": (640, 480, (64, 0), 3321, 0, 128, 0.0),  # the same pair, every point far
    "near_pts": (320, 240, (56, 0), 3321, 3, 128, 0.05),     # a few near points: the largest misses
    "wide": (1242, 375, (5, -3), 2465, 1, 16, 0.5),          # the 512 and 1024 binade boundaries
}

# Tile sweep: the gentle 320 x 240 pair with n points, T = map_tile(n):
# n_tiles < 256 (3, 12, 13, 255), the T = 1 -> 2 step (256, 257), then per
# T in {9, 10, 12, 13, 16, 17, 18, 19, 63, 64} an n in (256 (T - 1), 256 T]
# that is no multiple of T (a partial last tile), and the full map.
# n = 1 and n = 2 are left out: the oracle's update is finite there (H is
# singular only up to rounding), so there is no NaN revert to pin and the
# result is rounding noise divided by rounding noise.
SWEEP_N = (3, 12, 13, 255, 256, 257, 2300, 2465, 3070, 3321, 4090, 4100, 4600, 4860, 16100, 16300, 16384)
SWEEP_ARGS = (320, 240, (3, 2), 0, 12, 0.5)  # make() without n

# Tolerance mode (precision = FAST) is held to 1e-4 against the fp64 oracle
# only where the oracle's cond(H) (numpy, stats[2:38], the last iteration of
# every level) stays at or below the largest value it takes on the inputs of
# tests/test_track.py::test_gpu_direct_pose, the data that bar was shown on.
# tests/test_direct_cases.py measures the ceiling and checks both lists.
COND_CEILING = 50.93
FAST_CASES = ("gentle", "small_l3", "odd_t64", "big_step", "wide")
FAST_SWEEP_N = tuple(n for n in SWEEP_N if n >= 255)


def level_dims(w: int, h: int):
    """Level sizes of the pyramid (oracle pyramid_dims: int(w * 0.5))."""
    ws, hs = [w], [h]
    for _ in range(1, LEVELS):
        ws.append(int(ws[-1] * 0.5))
        hs.append(int(hs[-1] * 0.5))
    return ws, hs


def map_tile(n: int) -> int:
    """Points per tile of the faithful map tree: min(64, ceil(n / 256))."""
    return max(1, min(64, (n + 255) // 256))


@functools.lru_cache(maxsize=None)
def _pair(w, h, shift, seed, scale):
    sx, sy = shift
    base = images.smooth(h + 160, w + 160, seed=seed, scale=scale)
    last = np.ascontiguousarray(base[80:80 + h, 80:80 + w])
    cur = np.ascontiguousarray(base[80 - sy:80 - sy + h, 80 - sx:80 - sx + w])
    lp, cp = oracle_lib.pyramid(last), oracle_lib.pyramid(cur)
    lp.setflags(write=False)
    cp.setflags(write=False)
    return lp, cp


def make(w, h, shift, n, seed, scale, near):
    """One case: dict(last, cur (pyramids), w, h, K, points (n, 3), pose_last,
    pose_init).  Deterministic in its arguments."""
    last, cur = _pair(w, h, tuple(shift), seed, scale)
    K = (0.8 * w, 0.8 * w, w / 2 - 0.3, h / 2 + 0.2)
    rng = np.random.default_rng(seed + 1000)
    u = rng.uniform(0, w, n)
    v = rng.uniform(0, h, n)
    z = rng.uniform(4, 12, n)
    m = int(near * n)
    z[:m] = rng.uniform(0.5, 1.2, m)
    pts = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
    pts.setflags(write=False)
    return dict(last=last, cur=cur, w=w, h=h, K=K, points=pts, pose_last=IDENTITY, pose_init=IDENTITY)


@functools.lru_cache(maxsize=None)
def case(name: str):
    return make(*CASES[name])


@functools.lru_cache(maxsize=None)
def sweep_case(n: int):
    w, h, shift, seed, scale, near = SWEEP_ARGS
    return make(w, h, shift, n, seed, scale, near)


def get(key):
    """A named case (str) or the tile sweep's case of n points (int)."""
    return sweep_case(key) if isinstance(key, int) else case(key)


@functools.lru_cache(maxsize=None)
def oracle_pose(key) -> np.ndarray:
    """The oracle's pose for get(key): computed once, shared, read-only."""
    c = get(key)
    p = oracle_lib.direct_pose(c["last"], c["cur"], c["w"], c["h"], c["K"], c["points"], c["pose_last"],
                               c["pose_init"])
    p.setflags(write=False)
    return p


def walk_levels(c: dict):
    """Levels 3 -> 0 through the oracle: (start poses [4] indexed by level,
    stats [4][50] indexed by level, final pose)."""
    pose = np.asarray(c["pose_init"], np.float64).copy()
    start = [None] * LEVELS
    stats = [None] * LEVELS
    for lv in range(LEVELS - 1, -1, -1):
        start[lv] = pose
        pose, stats[lv] = oracle_lib.direct_pose_level(c["last"], c["cur"], c["w"], c["h"], c["K"], c["points"],
                                                       c["pose_last"], pose, lv)
    return start, stats, pose


def _project(pose, K, P, scale):
    """oracle project(): mat3_vec's order, then the two quotients."""
    R, t = pose[:9], pose[9:]
    c = [(R[3 * i] * P[:, 0] + R[3 * i + 1] * P[:, 1]) + R[3 * i + 2] * P[:, 2] + t[i] for i in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = scale * (c[0] / c[2] * K[0] + K[2])
        v = scale * (c[1] / c[2] * K[1] + K[3])
    return u, v


def _inside(u, v, w, h):
    return (u >= 0) & (u < w) & (v >= 0) & (v < h)


def _binade(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64) >> 52


def classify_level(c: dict, lv: int, pose_start, pose_pred) -> dict:
    """Boolean masks over the case's points, one per class, plus `good`."""
    ws, hs = level_dims(c["w"], c["h"])
    w, h = ws[lv], hs[lv]
    P = np.asarray(c["points"], np.float64)
    s = SCALES[lv]
    ur, vr = _project(c["pose_last"], c["K"], P, s)
    uc, vc = _project(pose_start, c["K"], P, s)
    up, vp = _project(pose_pred, c["K"], P, s)
    good = (_inside(ur - 4, vr - 4, w, h) & _inside(ur + 4, vr + 4, w, h) &
            _inside(uc - 4, vc - 4, w, h) & _inside(uc + 4, vc + 4, w, h))
    fin = np.isfinite(up) & np.isfinite(vp) & (np.abs(up) < 1e6) & (np.abs(vp) < 1e6)
    on = fin & (w >= WIN) & (h >= WIN)
    upf = np.where(fin, up, 0.0)
    vpf = np.where(fin, vp, 0.0)
    x0 = np.clip(np.floor(upf).astype(np.int64) - (WIN // 2 - 1), 0, max(w - WIN, 0))
    y0 = np.clip(np.floor(vpf).astype(np.int64) - (WIN // 2 - 1), 0, max(h - WIN, 0))
    ucg = np.where(good, uc, 0.0)
    vcg = np.where(good, vc, 0.0)
    fu = np.floor(ucg).astype(np.int64)
    fv = np.floor(vcg).astype(np.int64)
    whole = on & (fu - 6 >= x0) & (fu + 5 <= x0 + WIN - 2) & (fv - 6 >= y0) & (fv + 5 <= y0 + WIN - 2)
    one = (_binade(ucg - 6.0) == _binade(ucg + 6.0)) & (_binade(vcg - 6.0) == _binade(vcg + 6.0))
    per = on & ~whole
    # bases of the point's samples: [fu - 5, fu + 4] x [fv - 5, fv + 4];
    # served from the window: x0 <= ix <= x0 + 18, y0 <= iy <= y0 + 18
    hi = WIN - 2
    full = per & ((fu + 4 < x0) | (fu - 5 > x0 + hi) | (fv + 4 < y0) | (fv - 5 > y0 + hi))
    out_pred = (((fu - 5 < x0) & (x0 > 0)) | ((fu + 4 > x0 + hi) & (x0 < w - WIN)) |
                ((fv - 5 < y0) & (y0 > 0)) | ((fv + 4 > y0 + hi) & (y0 < h - WIN)))
    m = dict(good=good,
             shared=whole & one,
             straddle=whole & ~one,
             per_sample=per,
             edge_lt=per & ((ucg < 5) | (vcg < 5)),
             edge_r=per & (ucg >= w - 5),
             edge_b=per & (vcg >= h - 5),
             partial_miss=per & ~full & out_pred,
             full_miss=full,
             win_off=~on)
    for k in CLASSES:
        m[k] = m[k] & good
    pe = np.hypot(uc - up, vc - vp)
    m["pred_err_max"] = float(pe[good].max()) if good.any() else 0.0
    return m


@functools.lru_cache(maxsize=None)
def census(key) -> dict:
    """Per-class counts of good points per level for get(key):
    {class: [level 0..3]}, plus "good", "pred_err_max", "cond" (cond(H) of
    the oracle's last iteration per level), "update_finite" and "moved"."""
    return census_of(get(key))


def census_of(c: dict) -> dict:
    start, stats, final = walk_levels(c)
    out = {k: [0] * LEVELS for k in ("good",) + CLASSES}
    out["pred_err_max"] = [0.0] * LEVELS
    out["cond"] = [0.0] * LEVELS
    out["update_finite"] = [False] * LEVELS
    for lv in range(LEVELS):
        pred = start[lv + 1] if lv + 1 < LEVELS else np.asarray(c["pose_init"], np.float64)
        m = classify_level(c, lv, start[lv], pred)
        for k in ("good",) + CLASSES:
            out[k][lv] = int(m[k].sum())
        out["pred_err_max"][lv] = m["pred_err_max"]
        H = stats[lv][2:38].reshape(6, 6)
        out["cond"][lv] = float(np.linalg.cond(H)) if np.isfinite(H).all() and H.any() else float("inf")
        out["update_finite"][lv] = bool(np.isfinite(stats[lv][44:50]).all())
    out["moved"] = not np.array_equal(final, np.asarray(c["pose_init"], np.float64))
    out["n"] = len(c["points"])
    out["tile"] = map_tile(len(c["points"]))
    return out


def format_census(cen: dict) -> str:
    rows = [f"n = {cen['n']}, T = {cen['tile']}; good points per class at levels 0, 1, 2, 3"]
    for k in ("good",) + CLASSES:
        rows.append(f"  {k:13s}" + "".join(f"{v:7d}" for v in cen[k]))
    rows.append("  pred_err_max " + "".join(f"{v:7.1f}" for v in cen["pred_err_max"]))
    rows.append("  cond(H)      " + "".join(f" {v:.1e}" for v in cen["cond"]))
    return "\n".join(rows)
