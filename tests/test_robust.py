"""Robust tracking (viso_track_robust, viso_set_robust): the
restatement tests/robust_ref.py against tests/bright_ref.py (the tie), a plain
pixel loop, numpy's solve and a known answer under an occluder; the device
against the restatement, as a stage and in the frame path."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import bright_ref as br, kf_align_ref as ref, oracle_lib, robust_ref as rr, test_brightness as tb
from tests.lk_warp_ref import SCALE, levels, project, sample
from tests.test_relocalise import (ATOL, HS, IDENT, KS, RTOL, SHIFT, WS, ZS, _grid_points, _plane, _random_points,
                                   _shift_pose)

K9 = 9.0
K2 = 6.3          # the second k: no integer, and no multiple of 1/64 (the first pass's residual lattice)
OCC = (112, 208)  # the replaced columns, 30 % of the width
MARGIN = 1e-7     # the least |r - k| of a parity case (device and restatement differ by about 1e-12 relative)


# ------------------------------------------------------------------ the occluded pair
@functools.lru_cache(maxsize=None)
def _occluded(lo=OCC[0], hi=OCC[1]):
    """The pyramid of the base image moved by SHIFT px in x, its columns lo ..
    hi - 1 replaced by the same texture moved the other way."""
    img = np.roll(tb._base(), SHIFT, axis=1).copy()
    img[:, lo:hi] = np.roll(np.roll(tb._base(), -7, axis=1), 11, axis=0)[:, lo:hi]
    p = oracle_lib.pyramid(img)
    p.setflags(write=False)
    return p


# ------------------------------------------------------------------ 1: the tie to bright_ref
@pytest.mark.parametrize("which", ["grid", "random"])
def test_tie_to_the_plain_chain(which):
    """With a k that no residual exceeds the rule is bright_ref's, bit for bit."""
    pts = _grid_points() if which == "grid" else _random_points(257, 5)
    last, cur = tb._pyr_b(0), tb._pyr_b(SHIFT, 0.5, 20.0)
    pose0, rep0 = br.track_affine(last, cur, WS, HS, KS, pts, IDENT, IDENT, 10)
    pose, rep, w = rr.track_robust(last, cur, WS, HS, KS, pts, IDENT, IDENT, 10, 1e300)
    assert np.array_equal(pose, pose0)
    assert np.array_equal(rep[0:23], rep0[0:23])
    assert rep[24] == 64 * rep[2] and rep[25] == 0 and rep[23] == 1e300
    assert set(np.unique(w)) <= {0.0, 64.0} and w.sum() == rep[24]


# ------------------------------------------------------------------ 2: the weighted sums by a plain loop
def test_weighted_terms_against_a_pixel_loop():
    level, g, o, k = 1, 0.9, 3.0, 2.5
    lp, cp = tb._pyr_b(0), _occluded()
    L = [float(x) for x in IDENT]
    T = [float(x) for x in _shift_pose(SHIFT - 0.4)]
    pts = _random_points(5, seed=3, lo_u=60.0, hi_u=WS - 60.0)
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    ll, ws, hs = levels(lp, WS, HS)
    cl, _, _ = levels(cp, WS, HS)
    w, h, s = ws[level], hs[level], SCALE[level]
    good, terms = rr.point_terms(ll[level], cl[level], w, h, L, T, g, o, k, KS, P, level)
    assert good.all()
    J0, J1 = ref.d_pixel_d_xi(T, KS, P, s)
    u0, v0, _ = project(L, KS, P)
    u1, v1, _ = project(T, KS, P)
    one = lambda buf, x, y: float(sample(buf, w, h, np.float64(x), np.float64(y)))
    worst = 0.0
    for i in range(5):
        exp = np.zeros(46)
        for x in range(-4, 4):
            for y in range(-4, 4):
                xc, yc = s * u1[i] + x, s * v1[i] + y
                R = one(ll[level], s * u0[i] + x, s * v0[i] + y)
                C = one(cl[level], xc, yc)
                g0 = 0.5 * (one(cl[level], xc + 1, yc) - one(cl[level], xc - 1, yc))
                g1 = 0.5 * (one(cl[level], xc, yc + 1) - one(cl[level], xc, yc - 1))
                e = g * R + o - C
                r = abs(e)
                wt = k / r if r > k else 1.0
                t = 0
                for a in range(6):
                    ja = g0 * J0[a][i] + g1 * J1[a][i]
                    for b in range(a, 6):
                        exp[t] += wt * ja * (g0 * J0[b][i] + g1 * J1[b][i])
                        t += 1
                    exp[21 + a] += wt * e * ja
                    exp[28 + a] -= wt * ja * R
                    exp[34 + a] -= wt * ja
                exp[27] += k * (2 * r - k) if r > k else e * e
                exp[40] += wt * R * R
                exp[41] += wt * R
                exp[42] -= wt * e * R
                exp[43] -= wt * e
                exp[44] += wt
                exp[45] += r > k
        worst = max(worst, float(np.max(np.abs(terms[i] - exp) / np.abs(exp))))
        assert np.allclose(terms[i], exp, rtol=1e-12, atol=0), (i, terms[i], exp)
    print("down-weighted pixels per point", terms[:, 45], "worst relative difference", worst)
    # both branches of the weight are taken
    assert 0 < terms[:, 45].sum() < 5 * 64 and terms[:, 45].max() > 0


# ------------------------------------------------------------------ 3: the step
def test_weighted_step_against_numpy_solve():
    level, g, o = 0, 0.9, 3.0
    lp, cp = tb._pyr_b(0), _occluded()
    L = [float(x) for x in IDENT]
    T = [float(x) for x in _shift_pose(SHIFT - 0.4)]
    pts = _grid_points()
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    ll, ws, hs = levels(lp, WS, HS)
    cl, _, _ = levels(cp, WS, HS)
    good, terms = rr.point_terms(ll[level], cl[level], ws[level], hs[level], L, T, g, o, K9, KS, P, level)
    S, n = br.map_tree_sum(terms), int(good.sum())
    assert n > 100 and 0 < S[45] < 64 * n and S[44] < 64 * n
    M, rhs = np.zeros((8, 8)), np.zeros(8)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            M[a, b] = M[b, a] = S[k]
            k += 1
    rhs[:6] = S[21:27]
    M[:6, 6] = M[6, :6] = S[28:34]
    M[:6, 7] = M[7, :6] = S[34:40]
    M[6, 6], M[6, 7], M[7, 6], M[7, 7] = S[40], S[41], S[41], S[44]
    rhs[6:] = S[42:44]
    exp = np.linalg.solve(M, rhs)
    xi, dg, do = rr.step([float(x) for x in S])
    got = np.array(list(xi) + [dg, do])
    print("cond", np.linalg.cond(M), "\ngot", got, "\nexp", exp, "\nrelative", np.abs(got - exp) / np.abs(exp))
    assert np.all(np.abs(got - exp) <= 1e-9 * np.abs(exp))


# ------------------------------------------------------------------ 4: the known answer
def test_known_translation_under_an_occluder():
    """The occluded pair, unmodified brightness, the grid points, 10
    iterations, k = 9 (DESIGN.md §23 records the printed values)."""
    want = np.array([SHIFT * ZS / KS[0], 0.0, 0.0])
    pts = _grid_points()
    pose0, rep0 = br.track_affine(tb._pyr_b(0), _occluded(), WS, HS, KS, pts, IDENT, IDENT, 10)
    pose, rep, w = rr.track_robust(tb._pyr_b(0), _occluded(), WS, HS, KS, pts, IDENT, IDENT, 10, K9)
    e0, e1 = np.linalg.norm(pose0[9:] - want), np.linalg.norm(pose[9:] - want)
    # the level-0 patch columns of a point in the last image, and in the current one (moved by SHIFT)
    u = pts[:, 0] / pts[:, 2] * KS[0] + KS[2]
    lo, hi = u - 4, u + 3 + SHIFT
    outside = (hi < OCC[0]) | (lo > OCC[1] - 1)
    inside = (lo >= OCC[0]) & (hi <= OCC[1] - 1)
    good = w > 0
    print("plain", e0, "robust", e1, "factor", e0 / e1, "\nreport", rep)
    print("outside", int((outside & good).sum()), "least mass / 64", (w[outside & good] / 64).min())
    print("inside", int((inside & good).sum()), "largest mass / 64", (w[inside & good] / 64).max(), "mean",
          (w[inside & good] / 64).mean())
    assert rep[0] == 0 and rep[1] == 130 and rep[2] == 130 and good.all()
    assert e1 <= 0.25 * e0
    assert (outside & good).sum() >= 60 and (inside & good).sum() >= 20
    assert np.all(w[outside & good] / 64 >= 0.95)
    assert np.all(w[inside & good] / 64 <= 0.85)


# ------------------------------------------------------------------ 5: the ABI
NAMES = ("viso_track_robust", "viso_set_robust", "viso_get_robust", "viso_get_robust_report",
         "viso_get_robust_weights", "viso_get_robust_log")


def _lib():
    from viso_amd import _lib
    return _lib


def test_abi_exports_and_null_context():
    import ctypes
    L = _lib()
    lib = L.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert L.SIGNATURES["viso_track_robust"][10] is ctypes.c_double
    assert L.SIGNATURES["viso_set_robust"][1] is ctypes.c_double
    assert L.kernel_id("bright") == 19
    info, n, buf = np.zeros(8, np.int64), np.zeros(1, np.uint64), np.zeros(16 * 28)
    assert lib.viso_set_robust(None, 9.0) == -1
    assert lib.viso_get_robust(None, info.ctypes.data) == -1
    assert lib.viso_get_robust_report(None, buf.ctypes.data) == -1
    assert lib.viso_get_robust_weights(None, buf.ctypes.data, 16, n.ctypes.data) == -1
    assert lib.viso_get_robust_log(None, buf.ctypes.data, 16, n.ctypes.data) == -1
    assert lib.viso_track_robust(None, buf.ctypes.data, buf.ctypes.data, WS, HS, buf.ctypes.data, 1, buf.ctypes.data,
                                 buf.ctypes.data, 10, 9.0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == -1
    from viso_amd import api, frontend
    for name in ("track_robust", "set_robust", "get_robust", "robust_report", "robust_weights", "robust_log"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "track_robust") and hasattr(frontend.Viso, "set_robust")


# ------------------------------------------------------------------ GPU: the stage (6)
@functools.lru_cache(maxsize=None)
def _ctx():
    from viso_amd import api
    fx, fy, cx, cy = KS
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=WS, height=HS))


@pytest.fixture(scope="module", autouse=True)
def _close_stage_context():
    """The stage context's streams go back when the module is done."""
    yield
    if _ctx.cache_info().currsize:
        _ctx().close()
        _ctx.cache_clear()


def _expect(last, cur, points, seed=None, iterations=10, k=K9):
    """The restatement's (pose, report, weights) and its margins."""
    mg = {}
    seed = IDENT if seed is None else seed
    pose, rep, w = rr.track_robust(last, cur, WS, HS, KS, points, IDENT, seed, iterations, k, margins=mg)
    return pose, rep, w, mg


def _stage(last, cur, points, seed=None, iterations=10, k=K9, weights=True):
    exp = _expect(last, cur, points, seed, iterations, k)
    got = _ctx().track_robust(last, cur, WS, HS, points, IDENT, IDENT if seed is None else seed, iterations, k, weights)
    return got, exp


INT_COLS = [c for c in tb.INT_COLS if c != 23] + [25]
REAL_COLS = tb.REAL_COLS + [23, 24]


def _same_report(rep, erep):
    assert np.array_equal(rep[INT_COLS], erep[INT_COLS])
    assert np.allclose(rep[REAL_COLS], erep[REAL_COLS], rtol=RTOL, atol=ATOL, equal_nan=True)
    assert rep[26] == 0 and rep[27] == 0


def _same(got, exp, label=""):
    """test_brightness._same's rule, on the 28 columns and the weights; the
    case's Huber margin first."""
    (pose, rep, w), (epose, erep, ew, mg) = got, exp
    print(label, "margins", mg)
    print("gpu", pose, "\n", rep, "\nref", epose, "\n", erep)
    print("bit-equal:", np.array_equal(rep, erep, equal_nan=True) and np.array_equal(pose, epose) and
          (w is None or np.array_equal(w, ew)))
    assert mg.get("huber", np.inf) >= MARGIN, mg
    _same_report(rep, erep)
    assert np.allclose(pose, epose, rtol=RTOL, atol=ATOL)
    if w is not None:
        assert w.shape == ew.shape and np.allclose(w, ew, rtol=RTOL, atol=ATOL)
        assert np.array_equal(w == 0, ew == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 5, 6, 63, 64, 65, 256, 257, 513, 1025])
def test_gpu_stage_point_counts(n):
    """test_brightness's counts on the occluded pair, k = 9; the weights are
    not asked for once (n = 64)."""
    got, exp = _stage(tb._pyr_b(0), _occluded(), _random_points(n), weights=n != 64)
    assert exp[1][1] == n and exp[1][0] == (2 if n < 6 else 0) and (n < 6 or 0 < exp[1][25] < 64 * n)
    assert (got[2] is None) == (n == 64)
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_device_tie():
    """k = 1e300: the plain chain's bits from the robust kernel."""
    pts, last, cur = _random_points(257, 5), tb._pyr_b(0), tb._pyr_b(SHIFT, *tb.GAIN)
    pose0, rep0 = _ctx().track_affine(last, cur, WS, HS, pts, IDENT, IDENT, 10)
    pose, rep, w = _ctx().track_robust(last, cur, WS, HS, pts, IDENT, IDENT, 10, 1e300)
    print("plain", pose0, rep0, "\nrobust", pose, rep)
    assert np.array_equal(pose, pose0) and np.array_equal(rep[0:23], rep0[0:23], equal_nan=True)
    assert rep[23] == 1e300 and rep[24] == 64 * rep[2] and rep[25] == 0 and rep0[23] == 0
    assert set(np.unique(w)) <= {0.0, 64.0} and w.sum() == rep[24]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 20])
def test_gpu_stage_iterations(iterations):
    got, exp = _stage(tb._pyr_b(0), _occluded(), _random_points(257, 5), iterations=iterations)
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_second_k():
    got, exp = _stage(tb._pyr_b(0), _occluded(), _random_points(257, 5), k=K2)
    assert exp[1][23] == K2
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_tiny_k():
    """k = 1e-3 down-weights nearly every pixel."""
    got, exp = _stage(tb._pyr_b(0), _occluded(), _grid_points(), k=1e-3)
    print("down-weighted", exp[1][25], "of", 64 * exp[1][2])
    assert exp[1][25] >= 0.98 * 64 * exp[1][2]
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_far_seed():
    """A seed 5 px off: exits 0 (the last pass) and 1 or 2 both occur."""
    got, exp = _stage(tb._pyr_b(0), _occluded(), _random_points(120, 7), _shift_pose(SHIFT + 5.0), iterations=2)
    ex = tb._exits(exp[1])
    assert 0 in ex and (1 in ex or 2 in ex), ex
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_exits_and_statuses():
    cur, pts = _occluded(), _random_points(120, 7)
    # a flat current image: no gradient, A' = 0 and a non-finite step
    got, exp = _stage(tb._pyr_b(0), tb._pyr_b(0, flat=100), pts)
    assert 3 in tb._exits(exp[1]), exp[1]
    _same(got, exp, "flat current")
    # points whose patches leave level 3 only: exit 4 there, then a fit below
    # (no whole-pixel coordinates: level 3's first pass would have residuals of exactly 9)
    edge = _plane(np.linspace(18.3, 30.1, 40), np.linspace(40.7, 200.2, 40))
    got, exp = _stage(tb._pyr_b(0), cur, edge)
    assert exp[1][4] == 4 and np.isnan(exp[1][7]) and exp[1][0] == 0 and exp[1][16] != 4
    _same(got, exp, "outside level 3")
    # too few good points at every level: status 2
    far = _plane(np.linspace(0.5, 3.5, 8), np.linspace(40.0, 200.0, 8))
    got, exp = _stage(tb._pyr_b(0), cur, far)
    assert exp[1][0] == 2 and tb._exits(exp[1]) == [4, 4, 4, 4] and exp[1][24] == 0
    _same(got, exp, "no good point")


@pytest.mark.gpu
def test_gpu_stage_constant_last_image():
    """R is the same everywhere: det = d00 d11 - d01 d01 = 0 up to rounding;
    the level ends as the restatement's does."""
    got, exp = _stage(tb._pyr_b(0, flat=100), _occluded(), _random_points(120, 7))
    print("exits", tb._exits(exp[1]))
    _same(got, exp, "constant last")


@pytest.mark.gpu
def test_gpu_argument_codes():
    lib, h = _lib().load(), _ctx().h
    pts = np.ascontiguousarray(_random_points(20, 9))
    lp, cp = np.ascontiguousarray(tb._pyr_b(0)), np.ascontiguousarray(_occluded())
    pose, seed, out, rep, wts = IDENT.copy(), _shift_pose(1.0), np.zeros(12), np.zeros(28), np.zeros(20)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(n=20, it=10, k=9.0, last=lp, cur=cp, p=pts, pl=pose, sd=seed, po=out, rp=rep, wt=wts, wd=WS, ht=HS):
        return lib.viso_track_robust(h, ptr(last), ptr(cur), wd, ht, ptr(p), n, ptr(pl), ptr(sd), it, k, ptr(po),
                                     ptr(rp), ptr(wt))

    assert call() == 0 and call(n=0, p=None) == 0 and call(it=1) == 0 and call(it=20) == 0 and call(wt=None) == 0
    assert call(k=1e300) == 0 and call(k=5e-324) == 0
    for kw in ({"n": -1}, {"n": 16385}, {"it": 0}, {"it": 21}, {"last": None}, {"cur": None}, {"p": None}, {"pl": None},
               {"sd": None}, {"po": None}, {"rp": None}, {"wd": 0}, {"ht": -3}, {"k": 0.0}, {"k": -1.0},
               {"k": float("nan")}, {"k": float("inf")}, {"k": -float("inf")}, {"k": 1.1e300}):
        assert call(**kw) == -1, kw
    info, n = np.zeros(8, np.int64), np.zeros(1, np.uint64)
    for k in (-1.0, float("nan"), float("inf"), 1.1e300):
        assert lib.viso_set_robust(h, k) == -1
    # the brightness mode is off: nothing is allocated and the getters say so
    assert lib.viso_set_robust(h, 9.0) == 0
    assert lib.viso_get_robust(h, info.ctypes.data) == 0 and list(info) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert lib.viso_get_robust_report(h, rep.ctypes.data) == -4  # VISO_ERR_STATE
    assert lib.viso_get_robust_weights(h, None, 0, n.ctypes.data) == -4
    assert lib.viso_get_robust_log(h, None, 0, n.ctypes.data) == -4
    assert lib.viso_get_robust(h, None) == -1
    assert lib.viso_set_brightness(h, 10) == 0
    assert lib.viso_get_robust_report(h, rep.ctypes.data) == 0 and not rep.any()
    assert lib.viso_get_robust_report(h, None) == -1
    assert lib.viso_get_robust_weights(h, None, 0, n.ctypes.data) == 0 and n[0] == 0
    assert lib.viso_get_robust_log(h, None, 0, n.ctypes.data) == 0 and n[0] == 0
    assert lib.viso_set_robust(h, 0.0) == 0 and lib.viso_set_brightness(h, 0) == 0
    assert lib.viso_get_robust(h, info.ctypes.data) == 0 and list(info) == [0] * 8


# ------------------------------------------------------------------ GPU: the frame path (7)
WQ, HQ, N_FRAMES, ITER = tb.WQ, tb.HQ, tb.N_FRAMES, tb.ITER
# The first tracked frame has the identity as its last pose and map points on
# whole pixels: level 3's first pass samples both images on eighths of a pixel,
# its residuals are multiples of 1/64 and some are exactly 9.  The parity run
# therefore tracks frame 1 by the direct pose, with both modes off, and frames
# 2..9 (eight) with them on; test_gpu_set_while_tracking covers frame 1 under
# the plain brightness chain.
FIRST, LAST = 2, N_FRAMES + 1
BLOCK = (slice(24, 104), slice(150, 250))  # the replaced block of every frame behind the first


@functools.lru_cache(maxsize=None)
def _frame(k):
    """The renderer's frame k; behind frame 0 with a block replaced by the
    frame's own texture from elsewhere."""
    img = tb._seq().image(k).copy()
    if k > 0:
        img[BLOCK] = np.roll(np.roll(img, -9, axis=1), 6, axis=0)[BLOCK]
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _fpyr(k):
    return oracle_lib.pyramid(_frame(k))


def _start(gv):
    gv.process(_frame(0), tb._seq().image(0, 1))
    assert gv.state == 1
    return gv.GetPoints()


_models = {}


def _model(pts, first, last_frame, pose, k=K9):
    """The frame path with both modes on from frame `first` to `last_frame`,
    from `pose`: the restatement frame by frame.  Returns poses, brightness rows, robust rows,
    reports, the last weights, the margins."""
    key = (pts.tobytes(), first, last_frame, np.asarray(pose).tobytes(), k)
    if key not in _models:
        last = np.asarray(pose, np.float64)
        poses, rows, rrows, reps, mg = [], [], [], [], {}
        for f in range(first, last_frame + 1):
            last, rep, w = rr.track_robust(_fpyr(f - 1), _fpyr(f), WQ, HQ, tb._seq().K, pts, last, last, ITER, k,
                                           margins=mg)
            poses.append(last)
            rows.append([rep[20], rep[21], rep[16], rep[22]])
            with np.errstate(all="ignore"):
                rrows.append([rep[24] / (64.0 * rep[2]), rep[25]])
            reps.append(rep)
        _models[key] = (np.array(poses), np.array(rows), np.array(rrows), np.array(reps), w, mg)
    return _models[key]


def _run(gv, pts, stats):
    """Everything a run with both modes on from frame FIRST leaves, against
    the model; returns it for the comparison of the two ingest paths."""
    poses, rows, rrows, reps, w, mg = _model(pts, FIRST, LAST, gv.poses[FIRST - 2])
    got = dict(poses=gv.poses, blog=gv.brightness_log(), rlog=gv.robust_log(), rep=gv.robust_report(),
               brep=gv.brightness_report(), w=gv.robust_weights(), binfo=gv.brightness(), info=gv.robust(),
               stats=np.asarray(stats, np.float64), flog=gv.frame_log())
    print("margins", mg, "\ngpu poses", got["poses"], "\nmodel", poses, "\ngpu robust log", got["rlog"], "\nmodel",
          rrows, "\ninfo", list(got["info"]), list(got["binfo"]), "\nreport", got["rep"], "\nmodel", reps[-1])
    print("bit-equal:", np.array_equal(got["poses"], poses) and np.array_equal(got["rlog"], rrows) and
          np.array_equal(got["w"], w))
    assert mg["huber"] >= MARGIN, mg
    assert 0 < rrows[:, 1].min() and rrows[:, 0].max() < 1  # the block is down-weighted in every frame
    p = FIRST - 1  # the poses ahead of the modes: NaN rows in both logs
    assert len(got["poses"]) == LAST and np.isnan(got["blog"][:p]).all() and np.isnan(got["rlog"][:p]).all()
    assert np.allclose(got["poses"][p:], poses, rtol=RTOL, atol=ATOL)
    assert np.array_equal(got["blog"][p:, 2:], rows[:, 2:])
    assert np.allclose(got["blog"][p:, :2], rows[:, :2], rtol=RTOL, atol=ATOL)
    assert np.array_equal(got["rlog"][p:, 1], rrows[:, 1])
    assert np.allclose(got["rlog"][p:, 0], rrows[:, 0], rtol=RTOL, atol=ATOL)
    _same_report(got["rep"], reps[-1])
    assert np.array_equal(got["brep"][tb.INT_COLS], np.append(reps[-1][:23], 0.0)[tb.INT_COLS])
    assert np.allclose(got["brep"][tb.REAL_COLS], reps[-1][tb.REAL_COLS], rtol=RTOL, atol=ATOL, equal_nan=True)
    assert got["w"].shape == w.shape and np.allclose(got["w"], w, rtol=RTOL, atol=ATOL)
    assert list(got["binfo"]) == tb._info(reps)
    assert list(got["info"]) == [1, len(reps), int(reps[-1][25]), int(reps[-1][2]), 0, 0, 0, 0]
    assert stats[9] == reps[-1][2] and np.isclose(stats[10], reps[-1][3], rtol=RTOL, atol=ATOL)
    assert np.array_equal(got["flog"][p:, 0], reps[:, 2])
    assert np.allclose(got["flog"][p:, 1], reps[:, 3], rtol=RTOL, atol=ATOL)
    return got


@pytest.mark.gpu
def test_gpu_frame_path_both_ingest_paths():
    """Eight frames with brightness (10) and robust (9) on, through host frames
    and through one device chunk: each against the chained restatement, and
    the two against each other bit for bit."""
    import torch

    def begin():
        gv = tb._viso()
        pts = _start(gv)
        gv.OnNewFrame(_frame(1))
        gv.set_brightness(ITER)
        gv.set_robust(K9)
        return gv, pts

    gv, pts = begin()
    for f in range(FIRST, LAST + 1):
        gv.OnNewFrame(_frame(f))
    host = _run(gv, pts, gv.stats())
    gv.close()
    gv, pts_d = begin()
    assert np.array_equal(pts, pts_d)
    dl = torch.from_numpy(np.stack([_frame(f) for f in range(FIRST, LAST + 1)])).cuda()
    torch.cuda.synchronize()
    gv.process_device(dl.data_ptr(), None, N_FRAMES, WQ * HQ)
    gv.synchronize()
    dev = _run(gv, pts_d, gv.stats())
    gv.close()
    for key in host:
        assert np.array_equal(host[key], dev[key], equal_nan=True), key


@pytest.mark.gpu
def test_gpu_off_is_off():
    # with the brightness mode on: never set, and set to 0
    runs = []
    for mode in ("never", "cleared"):
        gv = tb._viso(brightness=(ITER,))
        if mode == "cleared":
            gv.set_robust(0)
        _start(gv)
        for f in range(1, N_FRAMES + 1):
            gv.OnNewFrame(_frame(f))
        assert list(gv.robust()) == [0] * 8
        with pytest.raises(_lib().VisoError) as e:
            gv.robust_log()
        assert e.value.rc == -4
        runs.append((gv.poses, gv.GetPoints(), gv.brightness_log(), gv.brightness_report(), gv.frame_log(),
                     gv.brightness(), gv.config()))
        gv.close()
    a, b = runs
    assert a[6] == b[6] and len(a[0]) == N_FRAMES
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:6], b[:6]))
    # with the brightness mode off: k = 9 against a context that never heard of either
    runs = []
    for mode in ("plain", "robust"):
        gv = tb._viso(**({"robust": (K9,)} if mode == "robust" else {}))
        gv.ctx.timing_enable(True)
        _start(gv)
        for f in range(1, N_FRAMES + 1):
            gv.OnNewFrame(_frame(f))
        assert gv.ctx.timing("bright")[0] == 0
        assert list(gv.robust()) == [1 if mode == "robust" else 0] + [0] * 7
        for getter in (gv.robust_log, gv.robust_report, gv.robust_weights):
            with pytest.raises(_lib().VisoError) as e:
                getter()
            assert e.value.rc == -4
        runs.append((gv.poses, gv.GetPoints(), gv.frame_log(), gv.alignment(), gv.config()))
        gv.close()
    a, b = runs
    assert a[4] == b[4]  # viso_get_config
    assert len(a[0]) == N_FRAMES and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:3], b[:3]))
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


@pytest.mark.gpu
def test_gpu_set_while_tracking():
    """Frames 1..3 by the plain brightness chain, the rest robustly: the rows
    before the switch read NaN, the rest follow the model from the pose the
    plain chain left."""
    gv = tb._viso(brightness=(ITER,))
    pts = _start(gv)
    for f in range(1, 4):
        gv.OnNewFrame(_frame(f))
    gv.set_robust(K9)
    for f in range(4, N_FRAMES + 1):
        gv.OnNewFrame(_frame(f))
    got, rows = gv.poses, gv.robust_log()
    poses, _, erows, reps, w, mg = _model(pts, 4, N_FRAMES, got[2])
    print("margins", mg, "\nlog", rows, "\nmodel", erows)
    assert mg["huber"] >= MARGIN, mg
    assert rows.shape == (N_FRAMES, 2) and np.isnan(rows[:3]).all()
    assert np.array_equal(rows[3:, 1], erows[:, 1]) and np.allclose(rows[3:, 0], erows[:, 0], rtol=RTOL, atol=ATOL)
    assert np.allclose(got[3:], poses, rtol=RTOL, atol=ATOL)
    assert not np.isnan(gv.brightness_log()).any()
    assert list(gv.robust()) == [1, len(reps), int(reps[-1][25]), int(reps[-1][2]), 0, 0, 0, 0]
    assert np.allclose(gv.robust_weights(), w, rtol=RTOL, atol=ATOL)
    gv.close()
