"""Brightness-compensated tracking (viso_track_affine, viso_set_brightness;
DESIGN.md §22): the restatement tests/bright_ref.py against the keyframe
alignment's oracle-pinned terms, a plain pixel loop, numpy's solve and a known
answer; the device against the restatement, as a stage and in the frame path."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import bright_ref as br, kf_align_ref as ref, oracle_lib
from tests.lk_warp_ref import SCALE, levels, project, sample
from tests.test_relocalise import (ATOL, HS, IDENT, KS, RTOL, SHIFT, WS, ZS, _grid_points, _img, _plane, _random_points,
                                   _rot_pose, _roundtrip, _shift_pose)


# ------------------------------------------------------------------ the small scene
@functools.lru_cache(maxsize=None)
def _base():
    """The scene's image in even bytes 40..166: every gain and offset below
    maps it to exact bytes without clipping."""
    img = ((_img() // 4) * 2 + 40).astype(np.uint8)
    img.setflags(write=False)
    return img


def _affine_image(img, g, o):
    """g img + o as bytes; asserts that the bytes are exact and none clips."""
    v = img.astype(np.float64) * g + o
    assert np.array_equal(v, np.rint(v)) and v.min() > 0 and v.max() < 255, (g, o, v.min(), v.max())
    return v.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pyr_b(shift, g=1.0, o=0.0, flat=-1):
    """The pyramid of the base image moved by `shift` pixels in x and mapped
    to g I + o (flat >= 0: a uniform image of that grey value instead)."""
    img = np.full((HS, WS), flat, np.uint8) if flat >= 0 else _affine_image(np.roll(_base(), shift, axis=1), g, o)
    p = oracle_lib.pyramid(img)
    p.setflags(write=False)
    return p


# ------------------------------------------------------------------ 1: the oracle-pinned terms
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_terms_equal_the_keyframe_alignments(level):
    """At g = 1, o = 0 the first 28 terms are kf_align_ref's, bit for bit
    (those are the oracle's: test_relocalise.test_point_terms_equal_the_oracles)."""
    lp, cp = _pyr_b(0), _pyr_b(SHIFT, 0.5, 20)
    L = _roundtrip(_rot_pose(0.004, -0.003, 0.002, (0.01, -0.02, 0.015)))
    T = [float(x) for x in _roundtrip(_rot_pose(-0.002, 0.005, 0.001, (0.05, 0.01, -0.01)))]
    pts = _random_points(40, seed=11)
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    ll, ws, hs = levels(lp, WS, HS)
    cl, _, _ = levels(cp, WS, HS)
    good, terms = br.point_terms(ll[level], cl[level], ws[level], hs[level], L, T, 1.0, 0.0, KS, P, level)
    good_k, terms_k = ref.point_terms(ll[level], cl[level], ws[level], hs[level], L, T, KS, P, level)
    assert good.sum() >= 8 and np.array_equal(good, good_k)
    assert np.array_equal(terms[:, :28], terms_k)
    assert np.abs(terms[good][:, 28:]).min() > 0


# ------------------------------------------------------------------ 2: B, d, c by a plain loop
def test_brightness_terms_against_a_pixel_loop():
    level, g, o = 1, 0.9, 3.0
    lp, cp = _pyr_b(0), _pyr_b(SHIFT, 0.5, 20)
    L = [float(x) for x in IDENT]
    T = [float(x) for x in _shift_pose(SHIFT - 0.4)]
    pts = _random_points(5, seed=3, lo_u=60.0, hi_u=WS - 60.0)
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    ll, ws, hs = levels(lp, WS, HS)
    cl, _, _ = levels(cp, WS, HS)
    w, h, s = ws[level], hs[level], SCALE[level]
    good, terms = br.point_terms(ll[level], cl[level], w, h, L, T, g, o, KS, P, level)
    assert good.all()
    J0, J1 = ref.d_pixel_d_xi(T, KS, P, s)
    u0, v0, _ = project(L, KS, P)
    u1, v1, _ = project(T, KS, P)
    one = lambda buf, x, y: float(sample(buf, w, h, np.float64(x), np.float64(y)))
    for i in range(5):
        exp = np.zeros(16)
        for x in range(-4, 4):
            for y in range(-4, 4):
                xc, yc = s * u1[i] + x, s * v1[i] + y
                R = one(ll[level], s * u0[i] + x, s * v0[i] + y)
                C = one(cl[level], xc, yc)
                g0 = 0.5 * (one(cl[level], xc + 1, yc) - one(cl[level], xc - 1, yc))
                g1 = 0.5 * (one(cl[level], xc, yc + 1) - one(cl[level], xc, yc - 1))
                e = g * R + o - C
                for a in range(6):
                    exp[a] -= (g0 * J0[a][i] + g1 * J1[a][i]) * R
                    exp[6 + a] -= g0 * J0[a][i] + g1 * J1[a][i]
                exp[12] += R * R
                exp[13] += R
                exp[14] -= e * R
                exp[15] -= e
        assert np.allclose(terms[i, 28:], exp, rtol=1e-12, atol=0), (i, terms[i, 28:], exp)


# ------------------------------------------------------------------ 3: the Schur step
def test_schur_step_against_numpy_solve():
    level, g, o = 0, 0.9, 3.0
    lp, cp = _pyr_b(0), _pyr_b(SHIFT, 0.5, 20)
    L = [float(x) for x in IDENT]
    T = [float(x) for x in _shift_pose(SHIFT - 0.4)]
    pts = _grid_points()
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    ll, ws, hs = levels(lp, WS, HS)
    cl, _, _ = levels(cp, WS, HS)
    good, terms = br.point_terms(ll[level], cl[level], ws[level], hs[level], L, T, g, o, KS, P, level)
    S, n = br.map_tree_sum(terms), int(good.sum())
    assert n > 100
    M, rhs = np.zeros((8, 8)), np.zeros(8)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            M[a, b] = M[b, a] = S[k]
            k += 1
    rhs[:6] = S[21:27]
    M[:6, 6] = M[6, :6] = S[28:34]
    M[:6, 7] = M[7, :6] = S[34:40]
    M[6, 6], M[6, 7], M[7, 6], M[7, 7] = S[40], S[41], S[41], 64.0 * n
    rhs[6:] = S[42:44]
    exp = np.linalg.solve(M, rhs)
    xi, dg, do = br.step([float(x) for x in S], n)
    got = np.array(list(xi) + [dg, do])
    print("cond", np.linalg.cond(M), "\ngot", got, "\nexp", exp, "\nrelative", np.abs(got - exp) / np.abs(exp))
    assert np.all(np.abs(got - exp) <= 1e-9 * np.abs(exp))


# ------------------------------------------------------------------ 4: the known answer
# three times the errors the restatement attains (1.7e-16 and 2.2e-14; 8.9e-16 and 9.6e-14)
G_O_BOUND = {(0.5, 20.0): (5.1e-16, 6.6e-14), (1.0, -9.0): (2.7e-15, 2.9e-13)}


@functools.lru_cache(maxsize=None)
def _known(g, o):
    return br.track_affine(_pyr_b(0), _pyr_b(SHIFT, g, o), WS, HS, KS, _grid_points(), IDENT, IDENT, 10)


@pytest.mark.parametrize("g,o", [(0.5, 20.0), (1.0, -9.0)])
def test_known_translation_gain_offset(g, o):
    """The current image is the last one moved by 3 px in x (t_x = 3 z / fx
    on the plane z = 10) and mapped to g I + o in exact bytes."""
    want = np.array([SHIFT * ZS / KS[0], 0.0, 0.0])
    pose0, rep0 = _known(1.0, 0.0)
    pose, rep = _known(g, o)
    plain = ref.kf_align([_pyr_b(0)], [IDENT], _pyr_b(SHIFT, g, o), WS, HS, KS, _grid_points(), iterations=10,
                         max_points=512)
    e0, e1 = np.linalg.norm(pose0[9:] - want), np.linalg.norm(pose[9:] - want)
    ep = np.linalg.norm(plain["poses"][0][9:] - want)
    print("unmodified", e0, rep0, "\nmodified", e1, rep, "\nplain 6-DoF", ep, plain["report"][0])
    print("g error", abs(rep[20] - g), "o error", abs(rep[21] - o))
    assert rep0[0] == 0 and rep[0] == 0 and rep[1] == 130
    assert e1 <= 2 * e0 + 1e-6
    assert ep > e1
    assert abs(rep[20] - g) <= G_O_BOUND[(g, o)][0] and abs(rep[21] - o) <= G_O_BOUND[(g, o)][1]


# ------------------------------------------------------------------ 5: the ABI
def _lib():
    from viso_amd import _lib
    return _lib


def test_abi_exports_and_null_context():
    L = _lib()
    lib = L.load()
    for name in ("viso_track_affine", "viso_set_brightness", "viso_get_brightness", "viso_get_brightness_log",
                 "viso_get_brightness_report"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert L.kernel_id("bright") == 19 and L.kernel_id("direct") == 5
    info, n, buf = np.zeros(8, np.int64), np.zeros(1, np.uint64), np.zeros(16 * 24)
    assert lib.viso_set_brightness(None, 10) == -1
    assert lib.viso_get_brightness(None, info.ctypes.data) == -1
    assert lib.viso_get_brightness_log(None, buf.ctypes.data, 16, n.ctypes.data) == -1
    assert lib.viso_get_brightness_report(None, buf.ctypes.data) == -1
    assert lib.viso_track_affine(None, buf.ctypes.data, buf.ctypes.data, WS, HS, buf.ctypes.data, 1, buf.ctypes.data,
                                 buf.ctypes.data, 10, buf.ctypes.data, buf.ctypes.data) == -1


# ------------------------------------------------------------------ GPU: the stage (6)
@functools.lru_cache(maxsize=None)
def _ctx():
    from viso_amd import api
    fx, fy, cx, cy = KS
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=WS, height=HS))


@pytest.fixture(scope="module", autouse=True)
def _close_stage_context():
    """The stage context's streams go back when the module is done: the files
    that run behind this one count on the process's hardware queues."""
    yield
    if _ctx.cache_info().currsize:
        _ctx().close()
        _ctx.cache_clear()


GAIN = (0.5, 20.0)


def _expect(last, cur, points, seed=None, iterations=10):
    """The restatement's (pose, report), its margins and its trace."""
    mg, trace = {}, []
    seed = IDENT if seed is None else seed
    pose, rep = br.track_affine(last, cur, WS, HS, KS, points, IDENT, seed, iterations, margins=mg, trace=trace)
    return pose, rep, mg, trace


def _stage(last, cur, points, seed=None, iterations=10):
    exp = _expect(last, cur, points, seed, iterations)
    got = _ctx().track_affine(last, cur, WS, HS, points, IDENT, IDENT if seed is None else seed, iterations)
    return got, exp


INT_COLS = [0, 1, 2, 22, 23] + [4 + 4 * q + k for q in range(4) for k in range(3)]
REAL_COLS = [3, 7, 11, 15, 19, 20, 21]


def _same(got, exp, label=""):
    """test_relocalise._same's rule."""
    (pose, rep), (epose, erep, mg, _) = got, exp
    print(label, "margins", mg)
    print("gpu", pose, "\n", rep, "\nref", epose, "\n", erep)
    print("bit-equal:", np.array_equal(rep, erep, equal_nan=True) and np.array_equal(pose, epose))
    assert np.array_equal(rep[INT_COLS], erep[INT_COLS])
    assert np.allclose(rep[REAL_COLS], erep[REAL_COLS], rtol=RTOL, atol=ATOL, equal_nan=True)
    assert np.allclose(pose, epose, rtol=RTOL, atol=ATOL)


def _exits(rep):
    return [int(x) for x in rep[4::4][:4]]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 5, 6, 63, 64, 65, 256, 257, 513, 1025])
def test_gpu_stage_point_counts(n):
    """Nothing, the threshold of 6, one tile's most points +-1 of a workgroup's
    waves, and map-tree tiles of 1, 2, 3 and 5 points with a ragged last tile."""
    got, exp = _stage(_pyr_b(0), _pyr_b(SHIFT, *GAIN), _random_points(n))
    assert exp[1][1] == n and exp[1][0] == (2 if n < 6 else 0)
    _same(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 20])
def test_gpu_stage_iterations(iterations):
    got, exp = _stage(_pyr_b(0), _pyr_b(SHIFT, *GAIN), _random_points(257, 5), iterations=iterations)
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_far_seed():
    """A seed 5 px off: exits 0 (the last pass) and 1 or 2 both occur."""
    got, exp = _stage(_pyr_b(0), _pyr_b(SHIFT, *GAIN), _random_points(120, 7), _shift_pose(SHIFT + 5.0), iterations=2)
    ex = _exits(exp[1])
    assert 0 in ex and (1 in ex or 2 in ex), ex
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_exits_and_statuses():
    cur, pts = _pyr_b(SHIFT, *GAIN), _random_points(120, 7)
    # a flat current image: no gradient, A' = 0 and a non-finite step
    got, exp = _stage(_pyr_b(0), _pyr_b(0, flat=100), pts)
    assert 3 in _exits(exp[1]), exp[1]
    _same(got, exp, "flat current")
    # points whose patches leave level 3 only: exit 4 there, then a fit below
    edge = _plane(np.linspace(18.0, 30.0, 40), np.linspace(40.0, 200.0, 40))
    got, exp = _stage(_pyr_b(0), cur, edge)
    assert exp[1][4] == 4 and np.isnan(exp[1][7]) and exp[1][0] == 0 and exp[1][16] != 4
    _same(got, exp, "outside level 3")
    # too few good points at every level: status 2
    far = _plane(np.linspace(0.5, 3.5, 8), np.linspace(40.0, 200.0, 8))
    got, exp = _stage(_pyr_b(0), cur, far)
    assert exp[1][0] == 2 and _exits(exp[1]) == [4, 4, 4, 4]
    _same(got, exp, "no good point")


@pytest.mark.gpu
def test_gpu_stage_constant_last_image():
    """R is the same everywhere: det = d00 d11 - d01 d01 = 0, dg is not finite
    and the level ends with exit 3."""
    got, exp = _stage(_pyr_b(0, flat=100), _pyr_b(SHIFT, *GAIN), _random_points(120, 7))
    assert 3 in _exits(exp[1]), exp[1]
    _same(got, exp, "constant last")


@pytest.mark.gpu
def test_gpu_argument_codes():
    lib, h = _lib().load(), _ctx().h
    pts = np.ascontiguousarray(_random_points(20, 9))
    lp, cp = np.ascontiguousarray(_pyr_b(0)), np.ascontiguousarray(_pyr_b(SHIFT, *GAIN))
    pose, seed, out, rep = IDENT.copy(), _shift_pose(1.0), np.zeros(12), np.zeros(24)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(n=20, it=10, last=lp, cur=cp, p=pts, pl=pose, sd=seed, po=out, rp=rep, wd=WS, ht=HS):
        return lib.viso_track_affine(h, ptr(last), ptr(cur), wd, ht, ptr(p), n, ptr(pl), ptr(sd), it, ptr(po), ptr(rp))

    assert call() == 0 and call(n=0, p=None) == 0 and call(it=1) == 0 and call(it=20) == 0
    for kw in ({"n": -1}, {"n": 16385}, {"it": 0}, {"it": 21}, {"last": None}, {"cur": None}, {"p": None}, {"pl": None},
               {"sd": None}, {"po": None}, {"rp": None}, {"wd": 0}, {"ht": -3}):
        assert call(**kw) == -1, kw
    info, n = np.zeros(8, np.int64), np.zeros(1, np.uint64)
    for it in (-1, 21):
        assert lib.viso_set_brightness(h, it) == -1
    assert lib.viso_get_brightness_log(h, None, 0, n.ctypes.data) == -4  # off: VISO_ERR_STATE
    assert lib.viso_get_brightness_report(h, rep.ctypes.data) == -4
    for it in (1, 20, 10, 0):
        assert lib.viso_set_brightness(h, it) == 0
        assert lib.viso_get_brightness(h, info.ctypes.data) == 0 and list(info) == [it, 0, 0, 0, 0, 0, 0, 0]
    assert lib.viso_get_brightness(h, None) == -1
    assert lib.viso_set_brightness(h, 10) == 0 and lib.viso_get_brightness_report(h, None) == -1
    assert lib.viso_set_brightness(h, 0) == 0


# ------------------------------------------------------------------ GPU: the frame path (7)
WQ, HQ = 416, 128  # test_relocalise's small synthetic size
N_FRAMES = 8
# frame k's (gain, offset) on bytes that are multiples of 4: exact, and inside 1..254 (asserted)
FRAME_GO = [None, (1.0, 10.0), (0.75, 30.0), (0.5, 100.0), (1.0, -3.0), (0.75, -2.0), (0.5, 0.0), (1.0, 15.0),
            (0.5, 130.0)]
ITER = 10


@functools.lru_cache(maxsize=None)
def _seq():
    from viso_amd.synth import Sequence
    return Sequence(WQ, HQ, seed=0, z_amp=20.0, z_period=1000.0)


@functools.lru_cache(maxsize=None)
def _frame(k, plain=False):
    img = _seq().image(k)
    if k > 0 and not plain:
        img = _affine_image(img & np.uint8(0xFC), *FRAME_GO[k])
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _fpyr(k):
    return oracle_lib.pyramid(_frame(k))


def _viso(**modes):
    import viso_amd
    seq = _seq()
    gv = viso_amd.Viso(*seq.K, width=WQ, height=HQ, enable_tracking=1, batch_frames=32)
    gv.set_stereo(seq.p.baseline, 128, 1)
    gv.set_frame_log(True)
    for name, args in modes.items():
        getattr(gv, "set_" + name)(*args)
    return gv


def _start(gv):
    gv.process(_frame(0), _seq().image(0, 1))
    assert gv.state == 1
    return gv.GetPoints()


_models = {}


def _model(pts, first=1, pose=None):
    """The frame path with the mode on from frame `first`, from `pose`:
    the restatement frame by frame.  Returns poses, log rows, reports."""
    key = (pts.tobytes(), first, None if pose is None else np.asarray(pose).tobytes())
    if key not in _models:
        last = IDENT.copy() if pose is None else np.asarray(pose, np.float64)
        poses, rows, reps = [], [], []
        for k in range(first, N_FRAMES + 1):
            last, rep = br.track_affine(_fpyr(k - 1), _fpyr(k), WQ, HQ, _seq().K, pts, last, last, ITER)
            poses.append(last)
            rows.append([rep[20], rep[21], rep[16], rep[22]])
            reps.append(rep)
        _models[key] = (np.array(poses), np.array(rows), np.array(reps))
    return _models[key]


def _info(reps):
    return [ITER, len(reps), int(reps[:, 22].sum()), int((reps[:, 0] == 2).sum()), int(reps[-1][16]), int(reps[-1][22]),
            int(reps[-1][2]), 0]


def _check_run(gv, pts, stats):
    poses, rows, reps = _model(pts)
    got_rows, info = gv.brightness_log(), list(gv.brightness())
    print("gpu poses", gv.poses, "\nmodel", poses, "\ngpu log", got_rows, "\nmodel", rows, "\ninfo", info)
    print("bit-equal:", np.array_equal(gv.poses, poses) and np.array_equal(got_rows, rows))
    assert np.allclose(gv.poses, poses, rtol=RTOL, atol=ATOL)
    assert np.array_equal(got_rows[:, 2:], rows[:, 2:])
    assert np.allclose(got_rows[:, :2], rows[:, :2], rtol=RTOL, atol=ATOL)
    assert info == _info(reps)
    rep = gv.brightness_report()
    assert np.array_equal(rep[INT_COLS], reps[-1][INT_COLS])
    assert np.allclose(rep[REAL_COLS], reps[-1][REAL_COLS], rtol=RTOL, atol=ATOL, equal_nan=True)
    flog = gv.frame_log()
    assert np.array_equal(flog[:, 0], reps[:, 2]) and np.allclose(flog[:, 1], reps[:, 3], rtol=RTOL, atol=ATOL)
    assert stats[9] == reps[-1][2] and np.isclose(stats[10], reps[-1][3], rtol=RTOL, atol=ATOL)
    # the estimated maps are the frames' own: g_k / g_{k-1} from frame 2 on (frame 1's includes the rounding to
    # multiples of 4)
    for k in range(2, N_FRAMES + 1):
        assert abs(rows[k - 1][0] * FRAME_GO[k - 1][0] / FRAME_GO[k][0] - 1) < 0.05, (k, rows[k - 1])


@pytest.mark.gpu
def test_gpu_frame_path_host_frames():
    gv = _viso(brightness=(ITER,))
    pts = _start(gv)
    for k in range(1, N_FRAMES + 1):
        gv.OnNewFrame(_frame(k))
    _check_run(gv, pts, gv.stats())
    gv.close()


@pytest.mark.gpu
def test_gpu_frame_path_device_ingest():
    import torch
    gv = _viso(brightness=(ITER,))
    pts = _start(gv)
    dl = torch.from_numpy(np.stack([_frame(k) for k in range(1, N_FRAMES + 1)])).cuda()
    torch.cuda.synchronize()
    gv.process_device(dl.data_ptr(), None, N_FRAMES, WQ * HQ)
    gv.synchronize()
    _check_run(gv, pts, gv.stats())
    gv.close()


@pytest.mark.gpu
def test_gpu_off_is_off():
    runs = []
    for mode in ("never", "cleared"):
        gv = _viso()
        if mode == "cleared":
            gv.set_brightness(0)
        gv.ctx.timing_enable(True)
        _start(gv)
        for k in range(1, N_FRAMES + 1):
            gv.OnNewFrame(_frame(k, plain=True))
        assert gv.ctx.timing("bright")[0] == 0 and list(gv.brightness()) == [0] * 8
        with pytest.raises(_lib().VisoError) as e:
            gv.brightness_log()
        assert e.value.rc == -4
        runs.append((gv.poses, gv.GetPoints(), gv.alignment(), gv.frame_log(), gv.config()))
        gv.close()
    a, b = runs
    assert a[4] == b[4]  # viso_get_config
    assert len(a[0]) == N_FRAMES and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    assert np.array_equal(a[3], b[3], equal_nan=True)


@pytest.mark.gpu
def test_gpu_set_while_tracking():
    """Frames 1..3 with the mode off (unmodified frames), the rest with it on:
    the rows before the switch read NaN, the rest follow the model from the
    pose the direct path left."""
    gv = _viso()
    pts = _start(gv)
    for k in range(1, 4):
        gv.OnNewFrame(_frame(k))
    gv.set_brightness(ITER)
    for k in range(4, N_FRAMES + 1):
        gv.OnNewFrame(_frame(k))
    got, rows = gv.poses, gv.brightness_log()
    poses, erows, reps = _model(pts, 4, got[2])
    print("log", rows, "\nmodel", erows)
    assert rows.shape == (N_FRAMES, 4) and np.isnan(rows[:3]).all()
    assert np.array_equal(rows[3:, 2:], erows[:, 2:]) and np.allclose(rows[3:, :2], erows[:, :2], rtol=RTOL, atol=ATOL)
    assert np.allclose(got[3:], poses, rtol=RTOL, atol=ATOL)
    assert list(gv.brightness()) == _info(reps)
    gv.close()


MAX_COST = 9000.0  # between the compensated and the plain level-0 costs of the gained frames (asserted)


@pytest.mark.gpu
def test_gpu_relocalise_keeps_gained_frames():
    """The verdict of viso_set_relocalise on the compensated cost: with a
    max_cost that the plain path's level-0 cost exceeds on the gained frames, no
    frame is lost with the mode on."""
    reloc = (1, MAX_COST, 100, 0, 10, 512)
    gv = _viso(brightness=(ITER,), relocalise=reloc)
    pts = _start(gv)
    poses, _, reps = _model(pts)
    # the plain path (the oracle's direct pose) from the same poses
    K = _seq().K
    plain = []
    for k in range(1, N_FRAMES + 1):
        last = IDENT if k == 1 else poses[k - 2]
        T = np.asarray(last, np.float64)
        for level in (3, 2, 1, 0):
            T, st = oracle_lib.direct_pose_level(_fpyr(k - 1), _fpyr(k), WQ, HQ, K, pts, last, T, level)
        plain.append(float(st[1]))
    print("compensated", reps[:, 3], "n", reps[:, 2], "of", len(pts), "\nplain", plain)
    assert reps[:, 3].max() <= 0.8 * MAX_COST and min(plain) > 1.2 * MAX_COST
    assert np.all(reps[:, 2] * 1000 >= 2 * reloc[2] * len(pts))
    for k in range(1, N_FRAMES + 1):
        gv.OnNewFrame(_frame(k))
    print("status", list(gv.frame_status()), "info", list(gv.relocalise()))
    assert list(gv.frame_status()) == [0] * N_FRAMES and list(gv.relocalise())[1:5] == [0, 0, 0, 0]
    assert np.allclose(gv.poses, poses, rtol=RTOL, atol=ATOL)
    gv.close()
    # and without the mode the same frames are lost at once
    gv = _viso(relocalise=reloc)
    _start(gv)
    gv.OnNewFrame(_frame(1))
    assert list(gv.relocalise())[2] == 1
    gv.close()
