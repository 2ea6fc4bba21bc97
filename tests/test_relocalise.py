"""Relocalisation (viso_kf_align, viso_set_relocalise): the
restatement tests/kf_align_ref.py against the oracle's arithmetic, a known
answer and the renderer; a Python model of the frame path over an occlusion;
the device against both."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import images, kf_align_ref as ref, oracle_lib
from tests.pose_refine_ref import quat_from_matrix, quat_to_matrix

IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
RTOL, ATOL = 1e-9, 1e-12  # the bar of §17's pipeline test

# ------------------------------------------------------------------ the small scene (tests 1, 2, 6)
WS, HS = 320, 240
KS = (517.3, 516.5, 325.1, 249.7)  # the context's default intrinsics
ZS = 10.0
SHIFT = 3


@functools.lru_cache(maxsize=None)
def _img():
    img = images.smooth(HS, WS)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _pyr_small(shift, offset=0, flat=False):
    """The pyramid of the scene's image moved by `shift` pixels in x, `offset`
    grey levels brighter (flat: a uniform image instead)."""
    if flat:
        img = np.full((HS, WS), 100, np.uint8)
    else:
        img = np.clip(np.roll(_img(), shift, axis=1).astype(np.int32) + offset, 0, 255).astype(np.uint8)
    p = oracle_lib.pyramid(img)
    p.setflags(write=False)
    return p


def _plane(u, v):
    """World points of the pixels (u, v) of the unmoved image on z = ZS."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return np.stack([(u - KS[2]) / KS[0] * ZS, (v - KS[3]) / KS[1] * ZS, np.full(u.shape, ZS)], 1)


def _shift_pose(px):
    """The pose whose image is the unmoved one moved by px pixels in x."""
    p = IDENT.copy()
    p[9] = px * ZS / KS[0]
    return p


def _grid_points():
    us, vs = np.meshgrid(np.arange(12, WS, 24.0), np.arange(12, HS, 24.0))
    return _plane(us.ravel(), vs.ravel())


def _random_points(n, seed=1, lo_u=16.3, hi_u=WS - 16.3):
    rng = np.random.default_rng(seed)
    return _plane(rng.uniform(lo_u, hi_u, n), rng.uniform(16.3, HS - 16.3, n))


# ------------------------------------------------------------------ 1: the oracle's arithmetic
def _roundtrip(pose):
    """The pose as the oracle holds it: through a quaternion and back."""
    return np.array(quat_to_matrix(quat_from_matrix([float(x) for x in pose[:9]])) + [float(x) for x in pose[9:]])


def _rot_pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    return np.concatenate([R.ravel(), np.asarray(t, np.float64)])


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_point_terms_equal_the_oracles(level):
    """The 28 terms of one point are the H, b and cost * nGood the oracle's
    level reports for that point alone (the reference's level stops behind its
    first pass: 1 - cost / lastCost with lastCost = 0 is below delta_thresh)."""
    kp, cp = _pyr_small(0), _pyr_small(SHIFT)
    kf_pose = _roundtrip(_rot_pose(0.004, -0.003, 0.002, (0.01, -0.02, 0.015)))
    T = _roundtrip(_rot_pose(-0.002, 0.005, 0.001, (0.05, 0.01, -0.01)))
    pts = _random_points(8, seed=11, lo_u=60.0, hi_u=WS - 60.0)
    pts[:, 1] = np.clip(pts[:, 1], -3.5, -1.0)  # rows 69..198: inside level 3 too
    kl, ws, hs = ref.levels(kp, WS, HS)
    cl, _, _ = ref.levels(cp, WS, HS)
    seen = 0
    for P in pts:
        Pt = (P[0:1], P[1:2], P[2:3])
        good, terms = ref.point_terms(kl[level], cl[level], ws[level], hs[level], kf_pose, [float(x) for x in T], KS,
                                      Pt, level)
        _, stats = oracle_lib.direct_pose_level(kp, cp, WS, HS, KS, P[None], kf_pose, T, level)
        assert good[0] and stats[0] == 1
        H = stats[2:38].reshape(6, 6)
        exp = [H[a, b] for a in range(6) for b in range(a, 6)] + list(stats[38:44]) + [stats[1] * stats[0]]
        assert np.array_equal(terms[0], np.array(exp)), (level, P)
        seen += 1
    assert seen == 8


# ------------------------------------------------------------------ 2: a small known answer
def test_known_translation():
    """The current image is the keyframe's moved by 3 px in x: on the plane
    z = 10 that is t_x = 3 z / fx.  The restatement gives it to 1e-12
    relative, so the 5 % of the issue stands."""
    mg = {}
    r = ref.kf_align([_pyr_small(0)], [IDENT], _pyr_small(SHIFT), WS, HS, KS, _grid_points(), iterations=10,
                     max_points=512, margins=mg)
    rep, pose = r["report"][0], r["poses"][0]
    want = SHIFT * ZS / KS[0]
    got = float(np.linalg.norm(pose[9:12]))
    print("report", rep, "\nt", pose[9:12], "expected length", want, "margins", mg)
    assert r["winner"] == 0 and rep[0] == 0 and rep[1] == 130
    assert abs(got - want) <= 0.05 * want
    assert abs(abs(pose[9]) - want) <= 0.05 * want


# ------------------------------------------------------------------ 3: the renderer
W, H = 1242, 375
MAX_COST = 4 * 14400.0  # 4 x photometric_error_thresh, §18's max_score
PARAMS = dict(iterations=10, max_points=512, max_cost=MAX_COST, min_good_permille=500)
FOREIGN = (5, 6, 7)


@functools.lru_cache(maxsize=None)
def _seq(seed=0):
    from viso_amd.synth import Sequence
    return Sequence(W, H, seed=seed)


@functools.lru_cache(maxsize=None)
def _image(f, cam=0):
    img = _seq().image(f, cam)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _scene_image(f):
    """The occlusion scenario: frames 5-7 show another scene."""
    if f in FOREIGN:
        img = _seq(7).image(40 + f)
        img.setflags(write=False)
        return img
    return _image(f)


@functools.lru_cache(maxsize=None)
def _pyr(f, scene=False):
    p = oracle_lib.pyramid(_scene_image(f) if scene else _image(f))
    p.setflags(write=False)
    return p


def _truth(f):
    """The renderer's pose of frame f in the map's frame (camera 0's)."""
    a, b = _seq().pose(f), _seq().pose(0)
    R = a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T
    return np.concatenate([R.ravel(), a[9:] - R @ b[9:]])


def _terr(pose, f):
    return float(np.linalg.norm(np.asarray(pose)[9:12] - _truth(f)[9:12]))


@functools.lru_cache(maxsize=None)
def _stereo_map():
    seq = _seq()
    ov = oracle_lib.Viso(seq.K, W, H, enable_tracking=1)
    ov.set_stereo(seq.p.baseline, 128, 1)
    ov.on_new_stereo(_image(0), _image(0, 1))
    assert ov.state == 1
    pts = ov.points()
    for f in range(1, 5):
        ov.on_new_frame(_image(f))
    poses = ov.poses()
    E = max(_terr(poses[f - 1], f) for f in range(1, 5))
    pts.setflags(write=False)
    return pts, E


def _align(f, extra=None, pyr=None):
    pts, _ = _stereo_map()
    return ref.kf_align([_pyr(0)], [IDENT], _pyr(f) if pyr is None else pyr, W, H, _seq().K, pts, extra_seed=extra,
                        **PARAMS)


@pytest.mark.parametrize("f,extra", [(2, None), (4, None), (6, None), (8, 4), (10, 4)])
def test_renderer_accepts(f, extra):
    pts, E = _stereo_map()
    r = _align(f, None if extra is None else _truth(extra))
    w = r["winner"]
    print("frame", f, "winner", w, "report", r["report"], "E", E)
    assert len(pts) == 2465 and w == (0 if extra is None else 1)
    assert r["report"][w][0] == 0 and r["report"][w][3] <= MAX_COST
    err = _terr(r["poses"][w], f)
    print("translation error", err, "bound", 2 * E)
    assert err <= 2 * E


def test_renderer_rejects():
    r = _align(8)
    print("frame 8 from the keyframe's pose", r["report"])
    assert r["winner"] == -1 and r["report"][0][0] == 4
    r = _align(0, pyr=oracle_lib.pyramid(_seq(7).image(45)))
    print("foreign frame", r["report"])
    assert r["winner"] == -1 and r["report"][0][0] != 0
    r = _align(0, pyr=oracle_lib.pyramid(np.full((H, W), 128, np.uint8)))
    print("grey frame", r["report"])
    assert r["winner"] == -1 and r["report"][0][0] != 0


# ------------------------------------------------------------------ 4: the frame path's model
_track_cache = {}


def _track(f, last_pose):
    """A tracking frame f from frame f - 1 at last_pose, by the oracle: the
    direct pose, the level-0 verdict numbers, the LK counts at the pose."""
    key = (f, np.asarray(last_pose, np.float64).tobytes())
    if key not in _track_cache:
        pts, _ = _stereo_map()
        K = _seq().K
        lp, cp = _pyr(f - 1, True), _pyr(f, True)
        X = oracle_lib.direct_pose(lp, cp, W, H, K, pts, last_pose, last_pose)
        T = np.asarray(last_pose, np.float64)
        for level in (3, 2, 1, 0):
            T, st = oracle_lib.direct_pose_level(lp, cp, W, H, K, pts, last_pose, T, level)
        pk, sc, _, _ = oracle_lib.lk_align([_pyr(0)], [IDENT], cp, X, W, H, K, pts)
        _track_cache[key] = (X, float(st[0]), float(st[1]), int((pk >= 0).sum()), int(sc.sum()))
    return _track_cache[key]


@functools.lru_cache(maxsize=None)
def _model(lost_after, lk_permille=0, n_frames=11):
    """DESIGN.md §19's frame path over frames 1 .. n_frames - 1 of the
    scenario (lost_after 0: the mode off).  Returns poses, statuses, the info
    of viso_get_relocalise and the last attempt."""
    pts, _ = _stereo_map()
    n_map = len(pts)
    last = good = IDENT.copy()
    lost, bad_run = False, 0
    poses, status, attempt = [], [], None
    losses = attempts = recoveries = 0
    last_frame, last_winner, last_cands = -1, -1, 0
    for f in range(1, n_frames):
        if lost:
            st = None
        else:
            if lost_after and bad_run == 0:
                good = last
            X, n_good, cost, pairs, succ = _track(f, last)
            pose, st = X, 0
            if lost_after:
                bad = (not cost <= MAX_COST) or n_good * 1000 < PARAMS["min_good_permille"] * n_map or \
                      (lk_permille > 0 and succ * 1000 < lk_permille * pairs)
                bad_run = bad_run + 1 if bad else 0
                st = 1 if bad else 0
                if bad and bad_run >= lost_after:
                    lost, st = True, None
                    losses += 1
        if st is None:
            attempt = ref.kf_align([_pyr(0)], [IDENT], _pyr(f, True), W, H, _seq().K, pts, extra_seed=good, **PARAMS)
            attempts += 1
            last_frame, last_winner, last_cands = f, attempt["winner"], 2
            if attempt["winner"] >= 0:
                pose = good = attempt["poses"][attempt["winner"]]
                st, lost, bad_run = 3, False, 0
                recoveries += 1
            else:
                pose, st = good, 2
        poses.append(np.asarray(pose, np.float64))
        status.append(st)
        last = poses[-1]
    info = [lost_after, int(lost), losses, attempts, recoveries, last_frame, last_winner, last_cands]
    return {"poses": np.array(poses), "status": status, "info": info, "attempt": attempt}


def test_frame_path_model_recovers():
    _, E = _stereo_map()
    m = _model(1)
    err = [_terr(p, f + 1) for f, p in enumerate(m["poses"])]
    print("statuses", m["status"], "\nerrors", err, "E", E, "info", m["info"])
    assert m["status"] == [0, 0, 0, 0, 2, 2, 2, 3, 0, 0]
    for f in (5, 6, 7):
        assert np.array_equal(m["poses"][f - 1], m["poses"][3])
    assert max(err[7:10]) <= 2 * E
    assert m["info"] == [1, 0, 1, 4, 1, 8, 1, 2]
    off = _model(0)
    err_off = [_terr(p, f + 1) for f, p in enumerate(off["poses"])]
    print("mode off", err_off)
    assert off["status"] == [0] * 10 and err_off[-1] > 0.1
    assert np.array_equal(off["poses"][:4], m["poses"][:4])


LK_PERMILLE = 500  # tracked frames align four fifths of their pairs, foreign ones one in a hundred


def test_frame_path_model_lost_after_two():
    """The direct pose compares the last frame with the current one, so the
    second foreign frame has a low cost and only its LK row tells: the case
    runs with the LK test on."""
    m = _model(2, LK_PERMILLE)
    print("statuses", m["status"], "info", m["info"])
    assert m["status"] == [0, 0, 0, 0, 1, 2, 2, 3, 0, 0]
    # frame 5 is tracked at a wrong pose and is no good frame: the held pose is frame 4's
    assert not np.array_equal(m["poses"][4], m["poses"][3])
    assert np.array_equal(m["poses"][5], m["poses"][3])


# ------------------------------------------------------------------ 5: arguments
def _lib():
    from viso_amd import _lib
    return _lib


def test_abi_exports_and_null_context():
    L = _lib()
    lib = L.load()
    for name in ("viso_kf_align", "viso_set_relocalise", "viso_get_relocalise", "viso_get_relocalise_report",
                 "viso_get_frame_status"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert L.KERNEL_IDS["reloc"] == 15
    info, n = np.zeros(8, np.int64), np.zeros(1, np.uint64)
    buf = np.zeros(16 * 20)
    assert lib.viso_get_relocalise(None, info.ctypes.data) == -1
    assert lib.viso_get_relocalise_report(None, buf.ctypes.data, buf.ctypes.data, 16, n.ctypes.data) == -1
    assert lib.viso_get_frame_status(None, buf.ctypes.data, 16, n.ctypes.data) == -1
    assert lib.viso_set_relocalise(None, 1, MAX_COST, 500, 0, 10, 512) == -1
    w = np.zeros(1, np.int32)
    assert lib.viso_kf_align(None, buf.ctypes.data, buf.ctypes.data, 1, buf.ctypes.data, WS, HS, buf.ctypes.data, 1,
                             None, 0, 10, 512, MAX_COST, 500, buf.ctypes.data, buf.ctypes.data, w.ctypes.data) == -1


SETTER_BAD = [(-1, MAX_COST, 500, 0, 10, 512), (1001, MAX_COST, 500, 0, 10, 512), (1, 0.0, 500, 0, 10, 512),
              (1, -1.0, 500, 0, 10, 512), (1, float("nan"), 500, 0, 10, 512), (1, float("inf"), 500, 0, 10, 512),
              (1, MAX_COST, 0, 0, 10, 512), (1, MAX_COST, 1001, 0, 10, 512), (1, MAX_COST, 500, -1, 10, 512),
              (1, MAX_COST, 500, 1001, 10, 512), (1, MAX_COST, 500, 0, 0, 512), (1, MAX_COST, 500, 0, 21, 512),
              (1, MAX_COST, 500, 0, 10, 63), (1, MAX_COST, 500, 0, 10, 1025)]
SETTER_GOOD = [(1, MAX_COST, 500, 0, 10, 512), (1000, 1.0, 1, 1000, 1, 64), (3, 1e9, 1000, 500, 20, 1024),
               (0, 0.0, 0, -5, 0, 0)]


# ------------------------------------------------------------------ GPU: the stage (6)
@functools.lru_cache(maxsize=None)
def _ctx():
    from viso_amd import api
    fx, fy, cx, cy = KS
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=WS, height=HS))


def _stage(kf, cur, points, extra=None, **kw):
    """(device result, restatement, margins) of one attempt on the small
    scene: kf = [(shift, offset)], cur a pyramid."""
    par = dict(iterations=10, max_points=512, max_cost=MAX_COST, min_good_permille=500)
    par.update(kw)
    kf_pyrs = [_pyr_small(s, o) for s, o in kf]
    kf_poses = [_shift_pose(s) for s, _ in kf]
    mg = {}
    exp = ref.kf_align(kf_pyrs, kf_poses, cur, WS, HS, KS, points, extra_seed=extra, margins=mg, **par)
    got = _ctx().kf_align(kf_pyrs, kf_poses, cur, WS, HS, points, extra, **par)
    return got, exp, mg


INT_COLS = [0, 1, 2] + [4 + 4 * q + k for q in range(4) for k in range(3)]
COST_COLS = [3, 7, 11, 15, 19]


def _same(got, exp, mg, label=""):
    print(label, "margins", mg)
    print("gpu winner", got["winner"], "\n", got["report"], "\nref winner", exp["winner"], "\n", exp["report"])
    bit = np.array_equal(got["report"], exp["report"], equal_nan=True) and np.array_equal(got["poses"], exp["poses"])
    print("bit-equal:", bit)
    assert got["report"].shape == exp["report"].shape
    assert np.array_equal(got["report"][:, INT_COLS], exp["report"][:, INT_COLS])
    assert got["winner"] == exp["winner"]
    assert np.allclose(got["report"][:, COST_COLS], exp["report"][:, COST_COLS], rtol=RTOL, atol=ATOL, equal_nan=True)
    assert np.allclose(got["poses"], exp["poses"], rtol=RTOL, atol=ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 5, 6, 15, 16, 17, 64, 65, 257])
def test_gpu_stage_point_counts(n):
    """Nothing, the threshold of 6, one round of the 16 accumulators +-1, one
    wave's share +-1 and every wave with an unequal share."""
    got, exp, mg = _stage([(0, 2)], _pyr_small(SHIFT), _random_points(n))
    assert exp["report"][0][1] == n and exp["report"][0][0] == (1 if n < 6 else 0)
    _same(got, exp, mg)


@pytest.mark.gpu
@pytest.mark.parametrize("max_points", [64, 1024])
def test_gpu_stage_reaches_the_cap(max_points):
    pts = np.concatenate([_random_points(700, 2), _plane([-50.0] * 60, [20.0] * 60), _random_points(740, 3)])
    got, exp, mg = _stage([(0, 2)], _pyr_small(SHIFT), pts, max_points=max_points)
    assert len(pts) == 1500 and exp["report"][0][1] == max_points and exp["report"][0][0] == 0
    _same(got, exp, mg)


KF8 = [(0, 9), (1, 6), (-1, 4), (2, 1), (4, 7), (5, 3), (3, 5), (-2, 8)]  # (shift, brightness offset)


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,n_extra,iterations", [(1, 1, 10), (2, 0, 1), (2, 1, 10), (8, 0, 10), (8, 1, 1),
                                                      (8, 1, 10)])
def test_gpu_stage_candidates(n_kf, n_extra, iterations):
    """Keyframes that are copies moved by different amounts, of different
    brightness (the cost at the fit is about the offset squared): the
    candidate of the darkest offset wins."""
    kf = KF8[:n_kf]
    extra = _shift_pose(SHIFT + 0.6) if n_extra else None
    got, exp, mg = _stage(kf, _pyr_small(SHIFT), _random_points(257, 5), extra, iterations=iterations)
    assert len(exp["report"]) == n_kf * (1 + n_extra)
    if iterations == 10:
        best = min(range(n_kf), key=lambda k: kf[k][1])
        assert exp["winner"] // (1 + n_extra) == best
    _same(got, exp, mg)


@pytest.mark.gpu
def test_gpu_stage_exits_and_statuses():
    cur = _pyr_small(SHIFT)
    pts = _random_points(120, 7)
    # a flat current image: no gradient, H = 0 and a non-finite step at once (at level 3 the taps
    # that read 0 outside the buffer give a gradient to a few border points, so a step is made first)
    got, exp, mg = _stage([(0, 0)], _pyr_small(0, flat=True), pts)
    assert list(exp["report"][0][8::4]) == [3, 3, 3] and exp["report"][0][4] in (3, 5)
    assert exp["report"][0][0] == 4 and exp["winner"] == -1
    _same(got, exp, mg, "flat")
    # points whose patches leave level 3 only: exit 4 there, then a fit below
    edge = _plane(np.linspace(18.0, 30.0, 40), np.linspace(40.0, 200.0, 40))
    got, exp, mg = _stage([(0, 2)], cur, edge)
    assert exp["report"][0][4] == 4 and np.isnan(exp["report"][0][7]) and exp["report"][0][0] == 0
    _same(got, exp, mg, "outside level 3")
    # too few good points at every level: status 2
    far = _plane(np.linspace(0.5, 3.5, 8), np.linspace(40.0, 200.0, 8))
    got, exp, mg = _stage([(0, 2)], cur, far)
    assert exp["report"][0][0] == 2 and exp["report"][0][16] == 4
    _same(got, exp, mg, "no good point")
    # some points leave the current image at the result: status 3 at 1000 permille
    leaving = np.concatenate([pts, _plane(np.linspace(313.6, 315.4, 10), np.linspace(40.0, 200.0, 10))])
    got, exp, mg = _stage([(0, 2)], cur, leaving, min_good_permille=1000)
    assert exp["report"][0][0] == 3 and exp["report"][0][2] < exp["report"][0][1]
    _same(got, exp, mg, "points leaving")
    got, exp, mg = _stage([(0, 2)], cur, leaving, min_good_permille=900)
    assert exp["report"][0][0] == 0
    _same(got, exp, mg, "points leaving, 900 permille")
    # max_cost below the fit: status 4
    got, exp, mg = _stage([(0, 2)], cur, pts, max_cost=100.0)
    assert exp["report"][0][0] == 4 and exp["report"][0][3] > 100.0 and exp["winner"] == -1
    _same(got, exp, mg, "max_cost")
    # two identical keyframes tie: the lower index wins
    got, exp, mg = _stage([(1, 5), (0, 2), (0, 2), (2, 6)], cur, pts)
    assert exp["winner"] == 1 and exp["report"][1][3] == exp["report"][2][3]
    _same(got, exp, mg, "tie")
    # exits 0 (the last pass) and 1 or 2 together, from a far seed
    got, exp, mg = _stage([(0, 2)], cur, pts, _shift_pose(SHIFT + 5.0), iterations=2)
    assert 0 in list(exp["report"][:, 4::4].ravel())
    _same(got, exp, mg, "iterations 2")


@pytest.mark.gpu
def test_gpu_argument_codes():
    lib, h = _lib().load(), _ctx().h
    pts = np.ascontiguousarray(_random_points(20, 9))
    kp, cp = np.ascontiguousarray(_pyr_small(0)), np.ascontiguousarray(_pyr_small(SHIFT))
    pose, seed = IDENT.copy(), _shift_pose(1.0)
    po, rp, w = np.zeros((2, 12)), np.zeros((2, 20)), np.zeros(1, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(n_kf=1, n=20, n_extra=0, it=10, mp=512, mc=MAX_COST, pm=500, kfp=kp, kpo=pose, cur=cp, p=pts, sd=None,
             out=po, rep=rp, win=w, wd=WS, ht=HS):
        return lib.viso_kf_align(h, ptr(kfp), ptr(kpo), n_kf, ptr(cur), wd, ht, ptr(p), n, ptr(sd), n_extra, it, mp,
                                 mc, pm, ptr(out), ptr(rep), ptr(win))

    assert call() == 0 and call(n=0, p=None) == 0 and call(n_extra=1, sd=seed) == 0
    for kw in ({"n_kf": 0}, {"n_kf": 9}, {"n": -1}, {"n": 16385}, {"n_extra": -1}, {"n_extra": 2}, {"n_extra": 1},
               {"it": 0}, {"it": 21}, {"mp": 63}, {"mp": 1025}, {"mc": 0.0}, {"mc": -1.0}, {"mc": float("nan")},
               {"pm": 0}, {"pm": 1001}, {"kfp": None}, {"kpo": None}, {"cur": None}, {"p": None}, {"out": None},
               {"rep": None}, {"win": None}, {"wd": 0}, {"ht": -3}):
        assert call(**kw) == -1, kw
    for args in SETTER_BAD:
        assert lib.viso_set_relocalise(h, *args) == -1, args
    info, n = np.zeros(8, np.int64), np.zeros(1, np.uint64)
    assert lib.viso_get_relocalise_report(h, None, None, 0, n.ctypes.data) == -4  # off: VISO_ERR_STATE
    for args in SETTER_GOOD:
        assert lib.viso_set_relocalise(h, *args) == 0, args
        assert lib.viso_get_relocalise(h, info.ctypes.data) == 0 and info[0] == args[0]
    assert lib.viso_get_relocalise(h, None) == -1
    assert list(info) == [0, 0, 0, 0, 0, -1, -1, 0]


# ------------------------------------------------------------------ GPU: the frame path (7)
N_SCENE = 11


def _viso(w=W, h=H, seq=None, reloc=None, **modes):
    import viso_amd
    seq = seq or _seq()
    gv = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    gv.set_stereo(seq.p.baseline, 128, 1)
    gv.set_frame_log(True)
    for name, args in modes.items():
        getattr(gv, "set_" + name)(*args)
    if reloc is not None:
        gv.set_relocalise(*reloc)
    return gv


_scene_runs = {}


def _scene_run(lost_after, batched=False, lk_permille=0):
    key = (lost_after, batched, lk_permille)
    if key not in _scene_runs:
        gv = _viso(reloc=(lost_after, MAX_COST, 500, lk_permille, 10, 512) if lost_after else None)
        gv.process(_image(0), _image(0, 1))
        assert gv.state == 1
        pts = gv.GetPoints()
        if batched:
            import torch
            dl = torch.from_numpy(np.stack([_scene_image(f) for f in range(1, N_SCENE)])).cuda()
            torch.cuda.synchronize()
            gv.process_device(dl.data_ptr(), None, N_SCENE - 1, W * H)
            gv.synchronize()
        else:
            for f in range(1, N_SCENE):
                gv.OnNewFrame(_scene_image(f))
        res = {"points": pts, "poses": gv.poses, "status": gv.frame_status(), "info": gv.relocalise(),
               "flog": gv.frame_log(), "state": gv.state}
        if lost_after:
            res["report"] = gv.relocalise_report()
            res["launches"] = gv.ctx.timing("reloc")[0]
        _scene_runs[key] = res
        gv.close()
    return _scene_runs[key]


def _check_scene(res, m):
    _, E = _stereo_map()
    print("statuses", list(res["status"]), "info", list(res["info"]))
    err = [_terr(p, f + 1) for f, p in enumerate(res["poses"])]
    print("errors", err, "E", E)
    assert res["points"].shape == _stereo_map()[0].shape and np.allclose(res["points"], _stereo_map()[0], rtol=RTOL)
    assert list(res["status"]) == m["status"] and res["state"] == 1
    assert list(res["info"]) == m["info"]
    for f, st in enumerate(m["status"]):
        if st == 2:
            assert np.array_equal(res["poses"][f], res["poses"][3]), f  # the held pose: frame 4's
            assert np.isnan(res["flog"][f]).all(), f
    assert np.allclose(res["poses"], m["poses"], rtol=RTOL, atol=ATOL)
    poses, report = res["report"]
    exp = m["attempt"]
    assert np.array_equal(report[:, INT_COLS], exp["report"][:, INT_COLS])
    assert np.allclose(report[:, COST_COLS], exp["report"][:, COST_COLS], rtol=RTOL, atol=ATOL, equal_nan=True)
    assert np.allclose(poses, exp["poses"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(poses[m["info"][6]], res["poses"][m["info"][5] - 1])  # the recovered frame's pose
    assert max(err[7:10]) <= 2 * E


@pytest.mark.gpu
def test_gpu_frame_path_matches_the_model():
    res, off = _scene_run(1), _scene_run(0)
    _check_scene(res, _model(1))
    assert np.array_equal(res["poses"][:4], off["poses"][:4])  # frames 1-4: the same bits as with the mode off
    assert list(off["status"]) == [0] * 10 and _terr(off["poses"][-1], 10) > 0.1


@pytest.mark.gpu
def test_gpu_frame_path_device_ingest():
    res = _scene_run(1, batched=True)
    _check_scene(res, _model(1))
    assert np.array_equal(res["poses"], _scene_run(1)["poses"])


@pytest.mark.gpu
def test_gpu_frame_path_lost_after_two():
    res, m = _scene_run(2, lk_permille=LK_PERMILLE), _model(2, LK_PERMILLE)
    print("statuses", list(res["status"]), "model", m["status"], "info", list(res["info"]), m["info"])
    assert list(res["status"]) == m["status"] and list(res["info"]) == m["info"]
    assert np.allclose(res["poses"], m["poses"], rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ GPU: off is off (8)
WQ, HQ = 416, 128  # the smallest synthetic size whose stereo initialisation makes a map


@functools.lru_cache(maxsize=None)
def _seq_small():
    from viso_amd.synth import Sequence
    return Sequence(WQ, HQ, seed=0, z_amp=20.0, z_period=1000.0)


@pytest.mark.gpu
def test_gpu_off_is_off():
    seq = _seq_small()
    runs = []
    for mode in ("never", "cleared"):
        gv = _viso(WQ, HQ, seq)
        if mode == "cleared":
            gv.set_relocalise(1, MAX_COST, 500, 0, 10, 512)
            gv.set_relocalise(0)
        gv.ctx.timing_enable(True)
        gv.process(seq.image(0), seq.image(0, 1))
        assert gv.state == 1
        for f in range(1, 13):
            gv.OnNewFrame(seq.image(f))
        assert gv.ctx.timing("reloc")[0] == 0
        assert list(gv.frame_status()) == [0] * 12 and list(gv.relocalise()) == [0, 0, 0, 0, 0, -1, -1, 0]
        runs.append((gv.poses, gv.GetPoints(), gv.alignment(), gv.frame_log()))
        gv.close()
    a, b = runs
    assert len(a[0]) == 12 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    assert np.array_equal(a[3], b[3], equal_nan=True)


# ------------------------------------------------------------------ GPU: with its neighbours (9)
@pytest.mark.gpu
def test_gpu_lost_frames_feed_nothing():
    """Culling, pose and point refinement and depth seeds on, over the
    occlusion: the lost and the recovered frame leave the track records, the
    observation ring's schedule and the seeds alone, and the map after frame 10
    is as large as without an occlusion at the same count of tracking frames.
    Every schedule has the interval 4: at 6 tracking frames each has fired once,
    on frames 1-4, which both runs share; a lost frame that counted as a
    tracking frame would fire them again at frame 8, on records and seeds that
    the foreign frames had fed."""
    modes = dict(pose_refine=(5, 1.0, 8.0), point_cull=(4, 3, 2.0, 50), point_refine=(4, 5, 3, 1.0, 8.0, 3, 0.05),
                 depth_seeds=(4,))

    def run(frames, reloc):
        gv = _viso(reloc=reloc, **modes)
        gv.process(_image(0), _image(0, 1))
        snaps = {}
        for f in frames:
            gv.OnNewFrame(_scene_image(f) if reloc else _image(f))
            snaps[f] = (gv.point_tracks(), int(gv.point_refine()[2]), gv.depth_seeds().copy(), len(gv.GetPoints()))
        out = (snaps, list(gv.frame_status()), len(gv.GetPoints()), gv.point_cull().copy())
        gv.close()
        return out

    snaps, status, n_end, cull = run(range(1, 11), (1, MAX_COST, 500, 0, 10, 512))
    print("statuses", status, "map", n_end, "cull", list(cull))
    assert status == [0, 0, 0, 0, 2, 2, 2, 3, 0, 0]
    for f in (5, 6, 7, 8):
        assert np.array_equal(snaps[f][0], snaps[4][0]), f  # no record moved: no fail_run grew
        assert snaps[f][1] == snaps[4][1] and snaps[f][3] == snaps[4][3], f
        assert np.array_equal(snaps[f][2], snaps[4][2]), f
    plain, pstatus, p_end, pcull = run(range(1, 7), None)
    print("without an occlusion: map", p_end, "cull", list(pcull))
    assert pstatus == [0] * 6
    assert snaps[10][1] == plain[6][1] == 1  # as many point refinements at 6 tracking frames
    assert list(cull[2:5]) == list(pcull[2:5]) and cull[2] == 1 and cull[3] > 0  # one cull each, of as many points
    assert n_end == p_end
