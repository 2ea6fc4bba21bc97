"""Relocalisation with an affine brightness map per candidate
(viso_kf_align_illum, viso_set_reloc_illum): the restatement
tests/kf_align_illum_ref.py against the oracle-pinned keyframe alignment, a
plain pixel loop, known answers and the renderer; Python models of the frame
path over an occlusion whose end is exposed differently; the device against
all of them."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

from tests import bright_ref as br, kf_align_illum_ref as ref, kf_align_ref as ka, oracle_lib
from tests import test_brightness as tb, test_relocalise as tr, test_reloc_seed as ts
from tests.lk_warp_ref import SCALE, levels, project, sample

IDENT, KS, WS, HS, SHIFT, ZS = tr.IDENT, tr.KS, tr.WS, tr.HS, tr.SHIFT, tr.ZS
W, H = tr.W, tr.H
RTOL, ATOL = tr.RTOL, tr.ATOL
MAX_COST = tr.MAX_COST
MAX_GAIN = 4.0
PARAMS = dict(tr.PARAMS, max_gain=MAX_GAIN)
GAINS = [(1.0, -30.0), (1.0, 40.0), (0.5, 20.0), (0.5, 100.0), (1.5, -20.0)]
MAP_G, MAP_O = 0.6, 30.0  # the renderer's frames behind the occlusion


def _exits(rep):
    return [int(x) for x in rep[4::4][:4]]


# ------------------------------------------------------------------ 1: the oracle-pinned terms
def _pixel_loop(kf_buf, cur_buf, w, h, s, L, T, g, o, P, good):
    """Terms 28..43 summed over the good points by a plain double loop over
    the patch pixels (vectors over the points; math.fsum across them)."""
    J0, J1 = ka.d_pixel_d_xi(T, KS, P, s)
    u0, v0, _ = project(L, KS, P)
    u1, v1, _ = project(T, KS, P)
    exp = np.zeros((16, len(P[0])))
    with np.errstate(all="ignore"):
        for x in range(-4, 4):
            for y in range(-4, 4):
                xc, yc = s * u1 + x, s * v1 + y
                R = sample(kf_buf, w, h, s * u0 + x, s * v0 + y)
                C = sample(cur_buf, w, h, xc, yc)
                g0 = 0.5 * (sample(cur_buf, w, h, xc + 1, yc) - sample(cur_buf, w, h, xc - 1, yc))
                g1 = 0.5 * (sample(cur_buf, w, h, xc, yc + 1) - sample(cur_buf, w, h, xc, yc - 1))
                e = g * R + o - C
                for a in range(6):
                    exp[a] -= (g0 * J0[a] + g1 * J1[a]) * R
                    exp[6 + a] -= g0 * J0[a] + g1 * J1[a]
                exp[12] += R * R
                exp[13] += R
                exp[14] -= e * R
                exp[15] -= e
    return np.array([math.fsum(row[good]) for row in exp])


@pytest.mark.parametrize("n", [17, 130])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_pass_sums_equal_the_keyframe_alignments(level, n):
    """At g = 1, o = 0 the first 28 sums of a pass are kf_align_ref's, bit for
    bit (its terms are the oracle's and its order is the rule's: tests 1 of
    test_relocalise and test_brightness); the other 16 agree with a pixel loop."""
    kp, cp = tb._pyr_b(0), tb._pyr_b(SHIFT, 0.5, 20)
    L = [float(x) for x in tr._roundtrip(tr._rot_pose(0.004, -0.003, 0.002, (0.01, -0.02, 0.015)))]
    T = [float(x) for x in tr._roundtrip(tr._rot_pose(-0.002, 0.005, 0.001, (0.05, 0.01, -0.01)))]
    pts = tr._grid_points()[::130 // n][:n]  # spread over the image: the border rows leave the upper levels
    P = (pts[:, 0], pts[:, 1], pts[:, 2])
    kl, ws, hs = levels(kp, WS, HS)
    cl, _, _ = levels(cp, WS, HS)
    w, h = ws[level], hs[level]
    good, terms = br.point_terms(kl[level], cl[level], w, h, L, T, 1.0, 0.0, KS, P, level)
    good_k, terms_k = ka.point_terms(kl[level], cl[level], w, h, np.array(L), T, KS, P, level)
    S, cnt = ref.pass_sums(good, terms)
    Sk, cnt_k = ka.pass_sums(good_k, terms_k)
    assert len(pts) == n and cnt == cnt_k and cnt >= 6
    assert len(S) == 44 and S[:28] == Sk
    for g, o in ((1.0, 0.0), (0.9, 3.0)):
        good, terms = br.point_terms(kl[level], cl[level], w, h, L, T, g, o, KS, P, level)
        S, _ = ref.pass_sums(good, terms)
        exp = _pixel_loop(kl[level], cl[level], w, h, SCALE[level], L, T, g, o, P, good)
        rel = np.abs(np.array(S[28:]) - exp) / np.abs(exp)
        print("level", level, "n", n, "(g, o)", (g, o), "largest relative difference", rel.max())
        assert np.all(rel <= 1e-12), (S[28:], exp)


# ------------------------------------------------------------------ 2: the known answer
WANT = np.array([SHIFT * ZS / KS[0], 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def _known(g, o, illum=True):
    fn = ref.kf_align_illum if illum else ka.kf_align
    kw = dict(max_gain=MAX_GAIN) if illum else {}
    return fn([tb._pyr_b(0)], [IDENT], tb._pyr_b(SHIFT, g, o), WS, HS, KS, tr._grid_points(), iterations=10,
              max_points=512, max_cost=MAX_COST, min_good_permille=500, **kw)


@pytest.mark.parametrize("g,o", GAINS)
def test_known_translation_gain_offset(g, o):
    """The current image is the keyframe's moved by 3 px in x (t_x = 3 z / fx
    on the plane z = 10) and mapped to g I + o in exact bytes.  The plain
    alignment accepts (1, -30) at three times the motion and rejects the rest."""
    e0 = np.linalg.norm(_known(1.0, 0.0)["poses"][0][9:] - WANT)
    r, plain = _known(g, o), _known(g, o, False)
    e1, ep = np.linalg.norm(r["poses"][0][9:] - WANT), np.linalg.norm(plain["poses"][0][9:] - WANT)
    go = r["gain_offset"][0]
    print("unmodified", e0, "\nthis form", e1, r["report"][0], go, "\nplain", ep, plain["report"][0])
    print("g error", abs(go[0] - g), "o error", abs(go[1] - o))
    assert r["winner"] == 0 and r["report"][0][0] == 0 and r["report"][0][1] == 130
    assert e1 <= 2 * e0 + 1e-6
    assert abs(go[0] - g) <= 1e-9 and abs(go[1] - o) <= 1e-7
    if (g, o) == GAINS[0]:
        assert plain["report"][0][0] == 0 and ep > 0.5 * WANT[0]
    else:
        assert plain["report"][0][0] == 4 and plain["winner"] == -1


# ------------------------------------------------------------------ 3: the gain bound
@functools.lru_cache(maxsize=None)
def _pyr_of(kind):
    base = tb._base()
    img = {"flipud": lambda: np.flipud(base), "fliplr": lambda: np.fliplr(base),
           "roll": lambda: np.roll(base, (97, 53), axis=(0, 1)),
           "noise": lambda: np.random.default_rng(5).integers(0, 256, base.shape).astype(np.uint8),
           "flat": lambda: np.full(base.shape, 100, np.uint8)}[kind]()
    p = oracle_lib.pyramid(np.ascontiguousarray(img))
    p.setflags(write=False)
    return p


def _small(kf, cur, points=None, **kw):
    par = dict(iterations=10, max_points=512, max_cost=MAX_COST, min_good_permille=500, max_gain=MAX_GAIN)
    par.update(kw)
    return ref.kf_align_illum([kf], [IDENT], cur, WS, HS, KS, tr._grid_points() if points is None else points, **par)


@pytest.mark.parametrize("kind", ["flipud", "fliplr", "roll"])
def test_gain_bound_rejects_a_foreign_frame(kind):
    """A foreign frame is explained by g -> 0 at a cost below max_cost: the
    bound, not the cost, rejects it."""
    r = _small(tb._pyr_b(0), _pyr_of(kind))
    print(kind, r["report"][0], r["gain_offset"][0])
    assert r["report"][0][0] == 5 and r["winner"] == -1
    assert r["report"][0][3] <= MAX_COST and abs(r["gain_offset"][0][0]) < 1 / MAX_GAIN


def test_gain_bound_noise_and_uniform_images():
    r = _small(tb._pyr_b(0), _pyr_of("noise"))
    print("noise", r["report"][0], r["gain_offset"][0])
    assert r["report"][0][0] in (4, 5) and r["winner"] == -1
    # a uniform current image: no gradient, A' = 0, the step is not finite, the state stays (seed, 1, 0)
    r = _small(tb._pyr_b(0), _pyr_of("flat"))
    print("uniform current", r["report"][0], r["gain_offset"][0])
    assert _exits(r["report"][0]) == [3, 3, 3, 3] and list(r["gain_offset"][0]) == [1.0, 0.0]
    assert np.array_equal(r["poses"][0], IDENT)  # (the status is the plain form's: its cost at the seed)
    # a uniform keyframe: R is the same everywhere, det = d00 d11 - d01 d01 = 0
    r = _small(_pyr_of("flat"), tb._pyr_b(SHIFT, 0.5, 20))
    print("uniform keyframe", r["report"][0], r["gain_offset"][0])
    assert _exits(r["report"][0]) == [3, 3, 3, 3] and list(r["gain_offset"][0]) == [1.0, 0.0]


# ------------------------------------------------------------------ 4: the renderer
def _map_image(img):
    """0.6 I + 30, rounded and clipped."""
    out = np.clip(np.rint(MAP_G * img.astype(np.float64) + MAP_O), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _foreign_pyr(mapped):
    img = tr._seq(7).image(45)
    return oracle_lib.pyramid(_map_image(img) if mapped else img)


@functools.lru_cache(maxsize=None)
def _mapped_pyr(f):
    p = oracle_lib.pyramid(_map_image(tr._image(f)))
    p.setflags(write=False)
    return p


def _attempt(cur, extra, illum):
    pts, _ = tr._stereo_map()
    if illum:
        return ref.kf_align_illum([tr._pyr(0)], [IDENT], cur, W, H, tr._seq().K, pts, extra_seed=extra, **PARAMS)
    return ka.kf_align([tr._pyr(0)], [IDENT], cur, W, H, tr._seq().K, pts, extra_seed=extra, **tr.PARAMS)


def test_renderer_mapped_frame():
    """Frame 8 at another exposure, from frame 4's truth: the plain alignment
    has no winner, this form recovers the pose."""
    _, E = tr._stereo_map()
    plain, r = _attempt(_mapped_pyr(8), tr._truth(4), False), _attempt(_mapped_pyr(8), tr._truth(4), True)
    err = tr._terr(r["poses"][1], 8)
    print("plain", plain["report"][:, :4], "\nthis form", r["report"][:, :4], r["gain_offset"], "error", err, "2 E", 2 * E)
    assert plain["winner"] == -1
    assert r["winner"] == 1 and err <= 2 * E and 0.25 <= r["gain_offset"][1][0] <= 4
    for mapped in (False, True):
        f = _attempt(_foreign_pyr(mapped), tr._truth(4), True)
        print("foreign frame, mapped" if mapped else "foreign frame", f["report"][:, :4], f["gain_offset"])
        assert f["winner"] == -1


# ------------------------------------------------------------------ 5, 6: the frame path's models
_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


@functools.lru_cache(maxsize=None)
def _scene_image(f, gap):
    """The occlusion: frames 5 .. gap - 1 show another scene, and the frames
    from the return on are exposed differently (0.6 I + 30)."""
    if 5 <= f < gap:
        img = tr._seq(7).image(40 + f)
        img.setflags(write=False)
        return img
    return _map_image(tr._image(f)) if f >= gap else tr._image(f)


@functools.lru_cache(maxsize=None)
def _scene_pyr(f, gap):
    p = oracle_lib.pyramid(_scene_image(f, gap))
    p.setflags(write=False)
    return p


def _track(f, gap, last_pose):
    """A tracking frame by the oracle: the direct pose and the level-0 verdict
    numbers (lk_permille is 0 here)."""
    def run():
        pts, _ = tr._stereo_map()
        K = tr._seq().K
        lp, cp = _scene_pyr(f - 1, gap), _scene_pyr(f, gap)
        X = oracle_lib.direct_pose(lp, cp, W, H, K, pts, last_pose, last_pose)
        T = np.asarray(last_pose, np.float64)
        for level in (3, 2, 1, 0):
            T, st = oracle_lib.direct_pose_level(lp, cp, W, H, K, pts, last_pose, T, level)
        return X, float(st[0]), float(st[1])
    return _cached(("track", f, gap, np.asarray(last_pose, np.float64).tobytes()), run)


@functools.lru_cache(maxsize=None)
def _model(gap, n_frames, illum, seed_on=False, illum_from=1):
    """§19's frame path (lost_after 1, lk_permille 0) with §21's seed stage and
    this mode (on from frame illum_from) over frames 1 .. n_frames - 1."""
    pts, _ = tr._stereo_map()
    n_map, K = len(pts), tr._seq().K
    last = good = IDENT.copy()
    lost = False
    poses, status, attempt, stage = [], [], None, None
    losses = attempts = recoveries = runs = ok = seed_rec = 0
    il_attempts = il_recoveries = 0
    last_frame, last_winner, il_winner = -1, -1, -1
    for f in range(1, n_frames):
        st = None
        on = illum and f >= illum_from
        if not lost:
            good = last
            X, n_good, cost = _track(f, gap, last)
            pose, st = X, 0
            if (not cost <= MAX_COST) or n_good * 1000 < PARAMS["min_good_permille"] * n_map:
                lost, st = True, None
                losses += 1
        if st is None:
            cur, gb = _scene_pyr(f, gap), good.tobytes()
            attempt = _cached(("attempt", f, gap, gb, on), lambda: _attempt(cur, good, on))
            attempts += 1
            il_attempts += on
            if attempt["winner"] < 0 and seed_on:
                stage = _cached(("seed", f, gap, gb), lambda: ts._seed_stage(cur, ts._corners(_scene_image(f, gap)), good))
                runs += 1
                if stage["report"][0] == 0:
                    ok += 1
                    assert stage["report"][10] == 0
                    attempt = _attempt(cur, stage["pose"], on)
                    attempts += 1
                    il_attempts += on
                    seed_rec += 1 if attempt["winner"] >= 0 else 0
            last_frame, last_winner = f, attempt["winner"]
            if on:
                il_winner = attempt["winner"]
            if attempt["winner"] >= 0:
                pose = good = attempt["poses"][attempt["winner"]]
                st, lost = 3, False
                recoveries += 1
                il_recoveries += on
            else:
                pose, st = good, 2
        poses.append(np.asarray(pose, np.float64))
        status.append(st)
        last = poses[-1]
    info = [1, int(lost), losses, attempts, recoveries, last_frame, last_winner, 2]
    sinfo = [int(seed_on), runs, ok, seed_rec] + ([0, 0, -1, -1] if stage is None else
                                                  [int(stage["report"][k]) for k in (3, 6, 10, 0)])
    return {"poses": np.array(poses), "status": status, "info": info, "seed_info": sinfo, "attempt": attempt,
            "stage": stage, "illum_info": [int(illum), il_attempts, il_recoveries, il_winner, 0, 0, 0, 0]}


GAP, N_SCENE = 8, 11  # test_relocalise's occlusion: frames 5-7 foreign, frames 0..10


def test_frame_path_model_recovers_at_another_exposure():
    """Frames 9 and 10 are tracked by the plain direct pose between two equally
    mapped frames, so no other mode is needed."""
    _, E = tr._stereo_map()
    off, on = _model(GAP, N_SCENE, False), _model(GAP, N_SCENE, True)
    err = [tr._terr(p, f + 1) for f, p in enumerate(on["poses"])]
    print("off", off["status"], off["info"], "\non ", on["status"], on["info"], on["illum_info"])
    print("errors", err, "2 E", 2 * E, "\nlast attempt", on["attempt"]["report"][:, :4], on["attempt"]["gain_offset"])
    assert off["status"] == [0, 0, 0, 0, 2, 2, 2, 2, 2, 2]
    assert on["status"] == [0, 0, 0, 0, 2, 2, 2, 3, 0, 0]
    assert max(err[7:10]) <= 2 * E
    assert on["info"] == [1, 0, 1, 4, 1, 8, 1, 2] and on["illum_info"][:4] == [1, 4, 1, 1]
    assert off["info"] == [1, 1, 1, 6, 0, 10, -1, 2]
    assert np.array_equal(off["poses"][:4], on["poses"][:4])


def test_seed_path_model_recovers_at_another_exposure():
    """test_reloc_seed's long occlusion: the seed stage finds the place (BRIEF
    bits survive an affine map), the plain second attempt throws it away."""
    _, E = tr._stereo_map()
    g = ts._gap()
    n = g + 4
    off, on = _model(g, n, False, True), _model(g, n, True, True)
    err = [tr._terr(p, f + 1) for f, p in enumerate(on["poses"])]
    print("g", g, "seed only", off["status"], off["info"], off["seed_info"], "\nboth", on["status"], on["info"],
          on["seed_info"], on["illum_info"], "\nerrors", err[g - 1:], "2 E", 2 * E)
    assert off["status"] == [0] * 4 + [2] * (g - 1)
    assert off["seed_info"][2] >= 1 and off["seed_info"][3] == 0 and off["stage"]["report"][0] == 0
    assert off["attempt"]["winner"] == -1
    assert on["status"] == [0] * 4 + [2] * (g - 5) + [3, 0, 0, 0]
    assert on["seed_info"][:4] == [1, g - 4, 1, 1] and on["info"][4] == 1 and on["illum_info"][2] == 1
    assert max(err[g - 1:g + 3]) <= 2 * E


# ------------------------------------------------------------------ 10a: the exports (no device needed)
def _lib():
    from viso_amd import _lib
    return _lib


NEW_ABI = ("viso_kf_align_illum", "viso_set_reloc_illum", "viso_get_reloc_illum", "viso_get_reloc_illum_rows")


def test_abi_exports_and_null_context():
    L = _lib()
    lib = L.load()
    for name in NEW_ABI:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert L.KERNEL_IDS["reloc"] == 15  # no new timing id
    from viso_amd import api
    for name in ("kf_align_illum", "set_reloc_illum", "get_reloc_illum", "reloc_illum_rows"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "kf_align_illum")
    info, n, buf, w = np.zeros(8, np.int64), np.zeros(1, np.uint64), np.zeros(16 * 20), np.zeros(1, np.int32)
    b = buf.ctypes.data
    assert lib.viso_set_reloc_illum(None, 1, MAX_GAIN) == -1
    assert lib.viso_get_reloc_illum(None, info.ctypes.data) == -1
    assert lib.viso_get_reloc_illum_rows(None, b, 16, n.ctypes.data) == -1
    assert lib.viso_kf_align_illum(None, b, b, 1, b, WS, HS, b, 1, None, 0, 10, 512, MAX_COST, 500, MAX_GAIN, b, b, b,
                                   w.ctypes.data) == -1


# ------------------------------------------------------------------ GPU: the stage (7-9)
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


CUR = (SHIFT, 0.5, 20.0)  # the gained current image of the stage tests


def _stage(kf_pyrs, kf_poses, cur, points, extra=None, **kw):
    """(device result, restatement, margins) of one attempt on the small scene."""
    par = dict(iterations=10, max_points=512, max_cost=MAX_COST, min_good_permille=500, max_gain=MAX_GAIN)
    par.update(kw)
    mg = {}
    exp = ref.kf_align_illum(kf_pyrs, kf_poses, cur, WS, HS, KS, points, extra_seed=extra, margins=mg, **par)
    got = _ctx().kf_align_illum(kf_pyrs, kf_poses, cur, WS, HS, points, extra, **par)
    return got, exp, mg


def _same(got, exp, mg, label=""):
    """Every integer equal, every cost, pose, g and o bit-equal; the margins
    guard the decisions."""
    print(label, "margins", mg)
    print("gpu winner", got["winner"], "\n", got["report"], "\n", got["gain_offset"], "\nref winner", exp["winner"], "\n",
          exp["report"], "\n", exp["gain_offset"])
    assert got["report"].shape == exp["report"].shape and got["gain_offset"].shape == exp["gain_offset"].shape
    assert np.array_equal(got["report"][:, tr.INT_COLS], exp["report"][:, tr.INT_COLS])
    assert got["winner"] == exp["winner"]
    assert np.array_equal(got["report"][:, tr.COST_COLS], exp["report"][:, tr.COST_COLS], equal_nan=True)
    assert np.array_equal(got["poses"], exp["poses"])
    assert np.array_equal(got["gain_offset"], exp["gain_offset"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 5, 6, 15, 16, 17, 65])
def test_gpu_stage_point_counts(n):
    """Nothing, the threshold of 6, one round of the 16 accumulators +-1 and an
    accumulator that wraps four times."""
    got, exp, mg = _stage([tb._pyr_b(0)], [IDENT], tb._pyr_b(*CUR), tr._random_points(n))
    assert exp["report"][0][1] == n and exp["report"][0][0] == (1 if n < 6 else 0)
    if n >= 6:
        assert np.allclose(exp["gain_offset"][0], CUR[1:], rtol=1e-9)
    _same(got, exp, mg)


@pytest.mark.gpu
@pytest.mark.parametrize("n,max_points", [(200, 64), (1025, 1024)])
def test_gpu_stage_reaches_the_cap(n, max_points):
    """The cap inside one ranking round, and a second round of one point."""
    got, exp, mg = _stage([tb._pyr_b(0)], [IDENT], tb._pyr_b(*CUR), tr._random_points(n, 2), max_points=max_points)
    assert exp["report"][0][1] == max_points and exp["report"][0][0] == 0
    _same(got, exp, mg)


# (shift, gain, offset) of eight keyframes, each with the same one-grey-level texture added in its own
# units: against the exact current image the compensated residual is that texture times 1 / gain, so the
# cost falls with the keyframe's gain and the one keyframe of gain 1.5 wins
KF8 = [(0, 1.0, 0.0), (1, 1.0, 10.0), (-1, 0.5, 20.0), (2, 0.5, 100.0), (4, 1.5, -20.0), (5, 1.0, -30.0),
       (3, 0.5, 60.0), (-2, 1.0, 40.0)]


@functools.lru_cache(maxsize=None)
def _pyr_kf8(k):
    s, g, o = KF8[k]
    tex = np.random.default_rng(17).integers(0, 2, (HS, WS))
    v = np.roll(tb._base(), s, axis=1).astype(np.float64) * g + o + tex
    assert np.array_equal(v, np.rint(v)) and v.min() > 0 and v.max() < 255
    p = oracle_lib.pyramid(v.astype(np.uint8))
    p.setflags(write=False)
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,n_extra,iterations", [(1, 1, 10), (2, 0, 1), (8, 1, 10)])
def test_gpu_stage_candidates(n_kf, n_extra, iterations):
    extra = tr._shift_pose(SHIFT + 0.6) if n_extra else None
    got, exp, mg = _stage([_pyr_kf8(k) for k in range(n_kf)], [tr._shift_pose(KF8[k][0]) for k in range(n_kf)],
                          tb._pyr_b(SHIFT), tr._random_points(257, 5), extra, iterations=iterations)
    n_cand = n_kf * (1 + n_extra)
    assert len(exp["report"]) == n_cand and len(np.unique(exp["gain_offset"], axis=0)) == n_cand
    if n_kf == 8:
        cost = exp["report"][:, 3]
        assert (exp["report"][:, 0] == 0).all() and exp["winner"] // 2 == 4
        assert np.delete(cost, [8, 9]).min() > 2 * cost[8:10].max()  # 1 / 1.5^2 against 1 and 4
        for k in range(8):  # the map from keyframe k to the current image is the inverse of k's own
            assert abs(exp["gain_offset"][2 * k][0] * KF8[k][1] - 1) < 0.02, (k, exp["gain_offset"][2 * k])
    _same(got, exp, mg)


@pytest.mark.gpu
def test_gpu_stage_exits_and_statuses():
    kf, cur, pts = tb._pyr_b(0), tb._pyr_b(*CUR), tr._random_points(120, 7)
    # a uniform current image: no gradient, A' = 0 and a non-finite step; the state stays (seed, 1, 0)
    got, exp, mg = _stage([kf], [IDENT], _pyr_of("flat"), pts)
    assert 3 in _exits(exp["report"][0]) and exp["report"][0][16] == 3
    _same(got, exp, mg, "uniform current")
    # a uniform keyframe: det = 0, dg is not finite
    got, exp, mg = _stage([_pyr_of("flat")], [IDENT], cur, pts)
    assert _exits(exp["report"][0]) == [3, 3, 3, 3] and list(exp["gain_offset"][0]) == [1.0, 0.0]
    _same(got, exp, mg, "uniform keyframe")
    # points whose patches leave level 3 only: exit 4 there, then a fit below
    edge = tr._plane(np.linspace(18.0, 30.0, 40), np.linspace(40.0, 200.0, 40))
    got, exp, mg = _stage([kf], [IDENT], cur, edge)
    assert exp["report"][0][4] == 4 and np.isnan(exp["report"][0][7]) and exp["report"][0][0] == 0
    _same(got, exp, mg, "outside level 3")
    # too few good points at every level: status 2
    far = tr._plane(np.linspace(0.5, 3.5, 8), np.linspace(40.0, 200.0, 8))
    got, exp, mg = _stage([kf], [IDENT], cur, far)
    assert exp["report"][0][0] == 2 and exp["report"][0][16] == 4 and list(exp["gain_offset"][0]) == [1.0, 0.0]
    _same(got, exp, mg, "no good point")
    # some points leave the current image at the result: status 3 at 1000 permille
    leaving = np.concatenate([pts, tr._plane(np.linspace(313.6, 315.4, 10), np.linspace(40.0, 200.0, 10))])
    got, exp, mg = _stage([kf], [IDENT], cur, leaving, min_good_permille=1000)
    assert exp["report"][0][0] == 3 and exp["report"][0][2] < exp["report"][0][1]
    _same(got, exp, mg, "points leaving")
    # a foreign frame: the gain bound rejects it at a cost below max_cost
    got, exp, mg = _stage([kf], [IDENT], _pyr_of("flipud"), tr._grid_points())
    assert exp["report"][0][0] == 5 and exp["report"][0][3] <= MAX_COST and exp["winner"] == -1
    _same(got, exp, mg, "flipud")
    # max_cost below the fit (the keyframe's added texture leaves a residual): status 4
    got, exp, mg = _stage([_pyr_kf8(0)], [IDENT], tb._pyr_b(SHIFT), pts, max_cost=1.0)
    assert exp["report"][0][0] == 4 and exp["report"][0][3] > 1.0 and exp["winner"] == -1
    _same(got, exp, mg, "max_cost")
    # exits 0 (the last pass) and 1 or 2 together, from a far seed
    got, exp, mg = _stage([kf], [IDENT], cur, pts, tr._shift_pose(SHIFT + 5.0), iterations=2)
    ex = [int(x) for x in exp["report"][:, 4::4].ravel()]
    assert 0 in ex and (1 in ex or 2 in ex)
    _same(got, exp, mg, "iterations 2")
    # m < 6: status 1, the row (1, 0), the pose out is the seed
    got, exp, mg = _stage([kf], [IDENT], cur, pts[:5], tr._shift_pose(1.0))
    assert list(exp["report"][:, 0]) == [1, 1] and np.array_equal(exp["gain_offset"], [[1.0, 0.0]] * 2)
    assert np.array_equal(exp["poses"][1], tr._shift_pose(1.0))
    _same(got, exp, mg, "m < 6")


# ------------------------------------------------------------------ GPU: argument codes (10)
@pytest.mark.gpu
def test_gpu_argument_codes():
    lib, h = _lib().load(), _ctx().h
    pts = np.ascontiguousarray(tr._random_points(20, 9))
    kp, cp = np.ascontiguousarray(tb._pyr_b(0)), np.ascontiguousarray(tb._pyr_b(*CUR))
    pose, seed = IDENT.copy(), tr._shift_pose(1.0)
    po, rp, go, w = np.zeros((2, 12)), np.zeros((2, 20)), np.zeros((2, 2)), np.zeros(1, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(n_kf=1, n=20, n_extra=0, it=10, mp=512, mc=MAX_COST, pm=500, mg=MAX_GAIN, kfp=kp, kpo=pose, cur=cp, p=pts,
             sd=None, out=po, rep=rp, gof=go, win=w, wd=WS, ht=HS):
        return lib.viso_kf_align_illum(h, ptr(kfp), ptr(kpo), n_kf, ptr(cur), wd, ht, ptr(p), n, ptr(sd), n_extra, it,
                                       mp, mc, pm, mg, ptr(out), ptr(rep), ptr(gof), ptr(win))

    assert call() == 0 and call(n=0, p=None) == 0 and call(n_extra=1, sd=seed) == 0 and call(mg=1.0 + 1e-9) == 0
    for kw in ({"mg": 1.0}, {"mg": 0.5}, {"mg": -4.0}, {"mg": float("nan")}, {"mg": float("inf")}, {"gof": None},
               {"n_kf": 0}, {"n_kf": 9}, {"n": -1}, {"n": 16385}, {"n_extra": -1}, {"n_extra": 2}, {"n_extra": 1},
               {"it": 0}, {"it": 21}, {"mp": 63}, {"mp": 1025}, {"mc": 0.0}, {"mc": -1.0}, {"mc": float("nan")},
               {"pm": 0}, {"pm": 1001}, {"kfp": None}, {"kpo": None}, {"cur": None}, {"p": None}, {"out": None},
               {"rep": None}, {"win": None}, {"wd": 0}, {"ht": -3}):
        assert call(**kw) == -1, kw
    info, n = np.zeros(8, np.int64), np.zeros(1, np.uint64)
    for args in ((-1, MAX_GAIN), (2, MAX_GAIN), (1, 1.0), (1, 0.0), (1, float("nan")), (1, float("inf"))):
        assert lib.viso_set_reloc_illum(h, *args) == -1, args
    assert lib.viso_get_reloc_illum_rows(h, None, 0, n.ctypes.data) == -4  # off: VISO_ERR_STATE
    assert lib.viso_get_reloc_illum_rows(h, go.ctypes.data, 2, n.ctypes.data) == -4
    assert lib.viso_get_reloc_illum(h, info.ctypes.data) == 0 and list(info) == [0, 0, 0, -1, 0, 0, 0, 0]
    for args in ((1, MAX_GAIN), (1, 1.5), (0, float("nan")), (1, 1e6), (0, 0.0)):
        assert lib.viso_set_reloc_illum(h, *args) == 0, args
        assert lib.viso_get_reloc_illum(h, info.ctypes.data) == 0 and list(info) == [args[0], 0, 0, -1, 0, 0, 0, 0]
        assert lib.viso_get_reloc_illum_rows(h, go.ctypes.data, 2, n.ctypes.data) == (0 if args[0] else -4)
        assert n[0] == 0  # no attempt has run
    assert lib.viso_get_reloc_illum(h, None) == -1


# ------------------------------------------------------------------ GPU: the frame path (11-13)
RELOC = (1, MAX_COST, 500, 0, 10, 512)
_runs = {}


def _run(gap, n_frames, illum, seed_on=False, batched=False, illum_from=1):
    """The scenario through the frame path.  illum: None (the setter is never
    called), 0 (called with mode 0) or 1, set before frame illum_from."""
    key = (gap, n_frames, illum, seed_on, batched, illum_from)
    if key not in _runs:
        gv = tr._viso(reloc=RELOC)
        if seed_on:
            gv.set_reloc_seed()
        if illum is not None and illum_from == 1:
            gv.set_reloc_illum(illum, MAX_GAIN if illum else float("nan"))
        gv.ctx.timing_enable(True)
        gv.process(tr._image(0), tr._image(0, 1))
        assert gv.state == 1
        pts = gv.GetPoints()
        if batched:
            import torch
            dl = torch.from_numpy(np.stack([_scene_image(f, gap) for f in range(1, n_frames)])).cuda()
            torch.cuda.synchronize()
            gv.process_device(dl.data_ptr(), None, n_frames - 1, W * H)
            gv.synchronize()
        else:
            for f in range(1, n_frames):
                if f == illum_from and f > 1:
                    gv.set_reloc_illum(illum, MAX_GAIN)
                gv.OnNewFrame(_scene_image(f, gap))
        res = {"points": pts, "poses": gv.poses, "status": list(gv.frame_status()), "info": list(gv.relocalise()),
               "seed_info": list(gv.reloc_seed()), "illum_info": list(gv.reloc_illum()), "flog": gv.frame_log(),
               "report": gv.relocalise_report(), "alignment": gv.alignment(), "state": gv.state,
               "launches": gv.ctx.timing("reloc")[0], "rows": gv.reloc_illum_rows() if illum else None}
        gv.close()
        _runs[key] = res
    return _runs[key]


def _check_run(res, m, first_back):
    _, E = tr._stereo_map()
    print("statuses", res["status"], "info", res["info"], "seed info", res["seed_info"], "illum", res["illum_info"])
    err = [tr._terr(p, f + 1) for f, p in enumerate(res["poses"])]
    print("errors", err, "2 E", 2 * E, "\nrows", res["rows"], "model", m["attempt"]["gain_offset"])
    assert res["status"] == m["status"] and res["state"] == 1
    assert res["info"] == m["info"] and res["seed_info"] == m["seed_info"] and res["illum_info"] == m["illum_info"]
    assert np.allclose(res["poses"], m["poses"], rtol=RTOL, atol=ATOL)
    poses, report = res["report"]
    exp = m["attempt"]
    assert np.array_equal(report[:, tr.INT_COLS], exp["report"][:, tr.INT_COLS])
    assert np.allclose(report[:, tr.COST_COLS], exp["report"][:, tr.COST_COLS], rtol=RTOL, atol=ATOL, equal_nan=True)
    assert np.allclose(poses, exp["poses"], rtol=RTOL, atol=ATOL)
    win = m["info"][6]
    assert res["rows"].shape == exp["gain_offset"].shape
    assert np.allclose(res["rows"][win], exp["gain_offset"][win], rtol=RTOL, atol=ATOL)
    assert np.array_equal(poses[win], res["poses"][m["info"][5] - 1])  # the recovered frame's pose
    assert max(err[first_back - 1:first_back + 2]) <= 2 * E


@pytest.mark.gpu
def test_gpu_frame_path_matches_the_model():
    res, off = _run(GAP, N_SCENE, 1), _run(GAP, N_SCENE, None)
    _check_run(res, _model(GAP, N_SCENE, True), GAP)
    m_off = _model(GAP, N_SCENE, False)
    assert off["status"] == m_off["status"] and off["info"] == m_off["info"]
    assert off["illum_info"] == [0, 0, 0, -1, 0, 0, 0, 0]
    assert np.array_equal(res["poses"][:4], off["poses"][:4])  # frames 1-4: the same bits as with the mode off
    assert res["launches"] == 4 and off["launches"] == 6  # one timed region per attempt, under VISO_KERNEL_RELOC


@pytest.mark.gpu
def test_gpu_frame_path_device_ingest():
    res = _run(GAP, N_SCENE, 1, batched=True)
    _check_run(res, _model(GAP, N_SCENE, True), GAP)
    assert np.array_equal(res["poses"], _run(GAP, N_SCENE, 1)["poses"])


@pytest.mark.gpu
def test_gpu_seed_path_matches_the_model():
    g = ts._gap()
    res, m = _run(g, g + 4, 1, seed_on=True), _model(g, g + 4, True, True)
    _check_run(res, m, g)
    assert res["seed_info"][3] == 1  # recoveries through a seed
    off, m_off = _run(g, g + 4, None, seed_on=True), _model(g, g + 4, False, True)
    print("seed only", off["status"], off["info"], off["seed_info"])
    assert off["status"] == m_off["status"] and off["info"] == m_off["info"] and off["seed_info"] == m_off["seed_info"]


@pytest.mark.gpu
def test_gpu_off_is_off():
    a, b = _run(GAP, N_SCENE, None), _run(GAP, N_SCENE, 0)
    assert a["status"] == [0, 0, 0, 0, 2, 2, 2, 2, 2, 2] and a["status"] == b["status"]
    assert a["info"] == b["info"] and a["illum_info"] == b["illum_info"] == [0, 0, 0, -1, 0, 0, 0, 0]
    assert a["launches"] == b["launches"] == a["info"][3] == 6
    assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"])
    assert all(np.array_equal(x, y) for x, y in zip(a["alignment"], b["alignment"]))
    assert np.array_equal(a["flog"], b["flog"], equal_nan=True)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["report"], b["report"]))
    # set on while tracking, between frames 3 and 4: the result of the run with the mode on from the start
    late, on = _run(GAP, N_SCENE, 1, illum_from=4), _run(GAP, N_SCENE, 1)
    assert late["status"] == on["status"] and late["info"] == on["info"] and late["illum_info"] == on["illum_info"]
    assert np.array_equal(late["poses"], on["poses"]) and np.array_equal(late["rows"], on["rows"])
