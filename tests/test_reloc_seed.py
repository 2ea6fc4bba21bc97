"""Relocalisation seed (viso_reloc_seed, viso_set_reloc_seed):
the restatement tests/reloc_seed_ref.py on the renderer (is the seed inside the
basin of the keyframe alignment?), a Python model of the frame path over a long
occlusion, and the device against both."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import images, kf_align_ref as ka, oracle_lib, reloc_seed_ref as ref
from tests import test_relocalise as tr

IDENT = tr.IDENT
RTOL, ATOL = 1e-9, 1e-12  # the frame path's bar (§19)
W, H = tr.W, tr.H
FAST_THRESH = 50  # the context's default (include/viso.h:21)
DEFAULTS = dict(hypotheses=256, max_hamming=48, ratio_permille=800, inlier_px=2.0, min_inliers=30, seed=0)
INT_COLS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]


def _corners(img):
    xs, ys, _ = oracle_lib.fast(np.ascontiguousarray(img), FAST_THRESH)
    return xs, ys


# ------------------------------------------------------------------ 1: the rule's pieces
def test_offsets_and_draws():
    off = ref.offsets()
    assert off.shape == (256, 4) and off.min() >= -6 and off.max() <= 6
    assert ref.mix64(0) == 0xE220A8397B1DCDAF  # splitmix64's first output from state 0
    assert len(np.unique(off, axis=0)) > 200  # (no table is committed: the formula is the table)
    for M in (3, 4, 7, 1000):
        for h in range(200):
            t = ref.draw(5, h, M)
            assert len(set(t)) == 3 and all(0 <= i < M for i in t)
    seen = {ref.draw(0, h, 3) for h in range(400)}
    assert len(seen) == 6  # every ordered triple of three matches is drawn


def _ramp_bits(gx, gy):
    """The descriptor of I1 = gx x + gy y + c written down from the offsets."""
    off = ref.offsets()
    return (gx * off[:, 0] + gy * off[:, 1]) < (gx * off[:, 2] + gy * off[:, 3])


RAMPS = [(7, 1), (1, 7), (-7, 1), (3, -4), (0, 5)]


def _ramp(gx, gy):
    ys, xs = np.mgrid[0:32, 0:32]
    v = gx * xs + gy * ys
    v = v - v.min()
    assert v.max() <= 255
    return v.astype(np.uint8)


@pytest.mark.parametrize("gx,gy", RAMPS)
def test_descriptor_known_answer(gx, gy):
    bits = _ramp_bits(gx, gy)
    for x, y in ((32, 32), (12, 13), (51, 50)):
        val, words = ref.describe(_ramp(gx, gy), 32, 32, [x], [y])
        got = np.unpackbits(words.view(np.uint8), bitorder="little")
        assert val[0] and np.array_equal(got.astype(bool), bits)
    val, _ = ref.describe(_ramp(gx, gy), 32, 32, [11, 52, 32, 32], [32, 32, 11, 52])
    assert not val.any()  # x1 = 5, x1 = 26 = w1 - 6, and the same in y


# ------------------------------------------------------------------ 2: the renderer
@functools.lru_cache(maxsize=None)
def _frame_corners(f, scene_g=0):
    return _corners(_scene_image(f, scene_g) if scene_g else tr._image(f))


def _seed_stage(cur_pyr, corners, start, **kw):
    pts, _ = tr._stereo_map()
    par = dict(DEFAULTS)
    par.update(kw)
    return ref.reloc_seed([tr._pyr(0)], [IDENT], pts, np.zeros(len(pts), np.int64), cur_pyr, W, H, tr._seq().K, start,
                          corners[0], corners[1], **par)


@functools.lru_cache(maxsize=None)
def _renderer_seed(f, start_frame):
    return _seed_stage(tr._pyr(f), _frame_corners(f), IDENT if start_frame == 0 else tr._truth(start_frame))


@pytest.mark.parametrize("f,start_frame", [(8, 0), (10, 0), (24, 4)])
def test_renderer_seed_is_inside_the_basin(f, start_frame):
    """The bound 0.02 sits 4x below the 0.08 from which §19 shows the
    alignment converging; the prototype's worst was 0.0071."""
    r = _renderer_seed(f, start_frame)
    rep, err = r["report"], tr._terr(r["pose"], f)
    print("frame", f, "report", rep, "translation error", err)
    assert rep[0] == 0 and rep[6] >= DEFAULTS["min_inliers"] and rep[10] == 0
    assert rep[3] == len(r["matches"]) and rep[6] == r["inliers"].sum()
    assert err <= 0.02


@pytest.mark.parametrize("f", [8, 10])
def test_alignment_from_the_seed_is_accepted(f):
    """The two rows §19 lists as rejected from the keyframe's pose."""
    pts, E = tr._stereo_map()
    r = _renderer_seed(f, 0)
    a = ka.kf_align([tr._pyr(0)], [IDENT], tr._pyr(f), W, H, tr._seq().K, pts, extra_seed=r["pose"], **tr.PARAMS)
    err = tr._terr(a["poses"][1], f)
    print("frame", f, "report", a["report"][:, :4], "error", err, "2 E", 2 * E)
    assert a["report"][0][0] == 4 and a["winner"] == 1 and a["report"][1][0] == 0
    assert err <= 2 * E


def test_foreign_frame_gives_no_seed():
    img = tr._seq(7).image(45)
    r = _seed_stage(oracle_lib.pyramid(img), _corners(img), IDENT)
    print("foreign frame", r["report"])
    assert r["report"][0] in (1, 2) and np.array_equal(r["pose"], IDENT)


# ------------------------------------------------------------------ 3: the model of the long occlusion
def _first_attempt(f, good):
    pts, _ = tr._stereo_map()
    return ka.kf_align([tr._pyr(0)], [IDENT], tr._pyr(f), W, H, tr._seq().K, pts, extra_seed=good, **tr.PARAMS)


@functools.lru_cache(maxsize=None)
def _tracked4():
    """Frames 1..4 tracked by the oracle: the poses (the last is the held pose)."""
    last, poses = IDENT.copy(), []
    for f in range(1, 5):
        last = tr._track(f, last)[0]
        poses.append(last)
    return poses


@functools.lru_cache(maxsize=None)
def _gap():
    """g: the smallest multiple of 4 >= 12 whose first attempt from frame 4's
    pose has no winner."""
    good = _tracked4()[-1]
    for g in range(12, 41, 4):
        if _first_attempt(g, good)["winner"] < 0:
            return g
    raise AssertionError("every first attempt up to frame 40 has a winner")


@functools.lru_cache(maxsize=None)
def _scene_image(f, g):
    """Frames 5 .. g - 1 show another scene."""
    if 5 <= f < g:
        img = tr._seq(7).image(40 + f)
        img.setflags(write=False)
        return img
    return tr._image(f)


@functools.lru_cache(maxsize=None)
def _scene_pyr(f, g):
    p = oracle_lib.pyramid(_scene_image(f, g))
    p.setflags(write=False)
    return p


_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _track(f, g, last_pose):
    """tests/test_relocalise.py _track on this scenario's images."""
    def run():
        pts, _ = tr._stereo_map()
        K = tr._seq().K
        lp, cp = _scene_pyr(f - 1, g), _scene_pyr(f, g)
        X = oracle_lib.direct_pose(lp, cp, W, H, K, pts, last_pose, last_pose)
        T = np.asarray(last_pose, np.float64)
        for level in (3, 2, 1, 0):
            T, st = oracle_lib.direct_pose_level(lp, cp, W, H, K, pts, last_pose, T, level)
        pk, sc, _, _ = oracle_lib.lk_align([tr._pyr(0)], [IDENT], cp, X, W, H, K, pts)
        return X, float(st[0]), float(st[1]), int((pk >= 0).sum()), int(sc.sum())
    return _cached(("track", f, g, np.asarray(last_pose, np.float64).tobytes()), run)


@functools.lru_cache(maxsize=None)
def _model(seed_on, n_frames=None):
    """§19's frame path with §21's seed over frames 1 .. g + 3 (lost_after 1,
    lk_permille 0)."""
    g = _gap()
    n_frames = n_frames or g + 4
    pts, _ = tr._stereo_map()
    n_map, K = len(pts), tr._seq().K
    last = good = IDENT.copy()
    lost = False
    poses, status, attempt, stage = [], [], None, None
    losses = attempts = recoveries = runs = ok = seed_rec = 0
    last_frame, last_winner = -1, -1
    for f in range(1, n_frames):
        st = None
        if not lost:
            good = last
            X, n_good, cost, pairs, succ = _track(f, g, last)
            pose, st = X, 0
            if (not cost <= tr.MAX_COST) or n_good * 1000 < tr.PARAMS["min_good_permille"] * n_map:
                lost, st = True, None
                losses += 1
        if st is None:
            cur = _scene_pyr(f, g)
            gb = good.tobytes()
            attempt = _cached(("attempt", f, g, gb), lambda: ka.kf_align([tr._pyr(0)], [IDENT], cur, W, H, K, pts,
                                                                       extra_seed=good, **tr.PARAMS))
            attempts += 1
            if attempt["winner"] < 0 and seed_on:
                stage = _cached(("seed", f, g, gb), lambda: _seed_stage(cur, _frame_corners(f, g), good))
                runs += 1
                if stage["report"][0] == 0:
                    ok += 1
                    assert stage["report"][10] == 0
                    attempt = ka.kf_align([tr._pyr(0)], [IDENT], cur, W, H, K, pts, extra_seed=stage["pose"],
                                          **tr.PARAMS)
                    attempts += 1
                    seed_rec += 1 if attempt["winner"] >= 0 else 0
            last_frame, last_winner = f, attempt["winner"]
            if attempt["winner"] >= 0:
                pose = good = attempt["poses"][attempt["winner"]]
                st, lost = 3, False
                recoveries += 1
            else:
                pose, st = good, 2
        poses.append(np.asarray(pose, np.float64))
        status.append(st)
        last = poses[-1]
    info = [1, int(lost), losses, attempts, recoveries, last_frame, last_winner, 2]
    sinfo = [int(seed_on), runs, ok, seed_rec] + ([0, 0, -1, -1] if stage is None else
                                                  [int(stage["report"][k]) for k in (3, 6, 10, 0)])
    return {"poses": np.array(poses), "status": status, "info": info, "seed_info": sinfo, "attempt": attempt,
            "stage": stage, "g": g}


def test_first_attempt_fails_at_the_gap():
    g, good = _gap(), _tracked4()[-1]
    a = _first_attempt(g, good)
    print("g", g, "first attempt", a["report"][:, :4])
    assert g % 4 == 0 and g >= 12 and a["winner"] == -1
    for q in range(12, g, 4):
        assert _first_attempt(q, good)["winner"] >= 0


def test_model_long_occlusion():
    _, E = tr._stereo_map()
    off, on = _model(False), _model(True)
    g = on["g"]
    err = [tr._terr(p, f + 1) for f, p in enumerate(on["poses"])]
    print("g", g, "off", off["status"], "\non ", on["status"], "\nerrors", err[g - 1:], "2 E", 2 * E)
    print("info", on["info"], "seed info", on["seed_info"], "stage", on["stage"]["report"])
    assert off["status"] == [0] * 4 + [2] * (g - 1)
    assert on["status"] == [0] * 4 + [2] * (g - 5) + [3, 0, 0, 0]
    assert max(err[g:g + 3]) <= 2 * E
    assert on["seed_info"][:4] == [1, g - 4, 1, 1] and on["info"][3] == g - 3 and on["info"][4] == 1
    assert np.array_equal(off["poses"][:4], on["poses"][:4])


# ------------------------------------------------------------------ 4: arguments without a device
def _lib():
    from viso_amd import _lib
    return _lib


def test_abi_exports_and_null_context():
    L = _lib()
    lib = L.load()
    for name in ("viso_reloc_seed", "viso_set_reloc_seed", "viso_get_reloc_seed", "viso_get_reloc_seed_report"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert L.KERNEL_IDS["reloc_seed"] == 18 and max(L.KERNEL_IDS.values()) == 18
    buf, info, n = np.zeros(64), np.zeros(8, np.int64), np.zeros(1, np.uint64)
    b = buf.ctypes.data
    assert lib.viso_set_reloc_seed(None, 256, 48, 800, 2.0, 30, 0) == -1
    assert lib.viso_get_reloc_seed(None, info.ctypes.data) == -1
    assert lib.viso_get_reloc_seed_report(None, b, b) == -1
    assert lib.viso_reloc_seed(None, b, b, 1, b, 320, 240, b, b, 1, b, 256, 48, 800, 2.0, 30, 0, b, b, b, b, 1,
                               n.ctypes.data) == -1


# ------------------------------------------------------------------ GPU: the stage at 320x240 (5)
WS, HS, KS, ZS, SHIFT = tr.WS, tr.HS, tr.KS, tr.ZS, tr.SHIFT
_plane = tr._plane


@functools.lru_cache(maxsize=None)
def _ctx(max_features=0):
    from viso_amd import api
    fx, fy, cx, cy = KS
    kw = dict(max_features=max_features) if max_features else {}
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=WS, height=HS, **kw))


@functools.lru_cache(maxsize=None)
def _tex(shift=0, seed=3):
    img = np.roll(images.mixed(HS, WS, seed), shift, axis=1)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _dots(k):
    """A grey image with k single bright pixels: exactly k FAST corners."""
    img = np.full((HS, WS), 100, np.uint8)
    for i in range(k):
        img[30 + 16 * (i // 17), 24 + 16 * (i % 17)] = 255
    return img


@functools.lru_cache(maxsize=None)
def _pyr_of(kind, arg=0, flat_level1=False):
    img = _tex(arg) if kind == "tex" else _dots(arg) if kind == "dots" else np.full((HS, WS), 100, np.uint8)
    p = oracle_lib.pyramid(img).copy()
    if flat_level1:  # (the stage takes the pyramid as data: every descriptor on it is 0)
        p[WS * HS:WS * HS + (WS // 2) * (HS // 2)] = 100
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _tex_points():
    """World points on z = ZS at the interior FAST corners of the unmoved
    texture, then random ones: 1,025."""
    xs, ys = _corners(_tex())
    keep = (xs >= 20) & (xs < WS - 20) & (ys >= 20) & (ys < HS - 20)
    rng = np.random.default_rng(4)
    n_fill = 1025 - int(keep.sum())
    assert n_fill > 0
    pts = np.concatenate([_plane(xs[keep], ys[keep]), _plane(rng.uniform(14.0, WS - 14.0, n_fill),
                                                              rng.uniform(14.0, HS - 14.0, n_fill))])
    pts.setflags(write=False)
    return pts


def _stage(kf_pyrs, kf_poses, cur_pyr, points, hosts=None, start=IDENT, ctx=None, **kw):
    """(device result, restatement) of one stage."""
    ctx = ctx or _ctx()
    par = dict(DEFAULTS, min_inliers=6)
    par.update(kw)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    hosts = np.zeros(len(points), np.int32) if hosts is None else np.asarray(hosts, np.int32)
    xs, ys = _corners(np.asarray(cur_pyr[:WS * HS]).reshape(HS, WS))
    exp = ref.reloc_seed(kf_pyrs, kf_poses, points, hosts, cur_pyr, WS, HS, KS, start, xs, ys, **par)
    got = ctx.reloc_seed(kf_pyrs, kf_poses, cur_pyr, WS, HS, points, hosts, start, **par)
    return got, exp


def _same(got, exp, label=""):
    """Integers and the match list array_equal; the cost and the pose bit-equal
    (printed), asserted within rtol 1e-12: libm's sin / cos / sqrt in the
    restatement against the device's in se3_exp."""
    print(label, "gpu", got["report"], "\nref", exp["report"])
    bit = np.array_equal(got["pose"], exp["pose"]) and np.array_equal(got["report"], exp["report"], equal_nan=True)
    print("bit-equal:", bit)
    assert np.array_equal(got["report"][INT_COLS], exp["report"][INT_COLS])
    assert np.array_equal(got["matches"], exp["matches"])
    assert np.array_equal(got["inliers"], exp["inliers"])
    assert np.allclose(got["report"][8], exp["report"][8], rtol=1e-12, atol=0, equal_nan=True)
    assert np.allclose(got["pose"], exp["pose"], rtol=1e-12, atol=1e-15)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 1025])
def test_gpu_stage_map_sizes(n):
    """Nothing, below three matches, one match workgroup +-1 and seventeen of
    them (two rounds of the one-workgroup compaction)."""
    got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), _tex_points()[:n])
    assert exp["report"][1] == n  # every point is described
    assert exp["report"][0] == (1 if n <= 3 else 0)  # (two of the first three points are matched)
    if n == 1025:
        want = SHIFT * ZS / KS[0]
        assert exp["report"][0] == 0 and abs(exp["pose"][9] - want) <= 0.1 * want
    _same(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 64, 65])
def test_gpu_stage_corner_counts(k):
    """k bright pixels are k corners; the 65 map points sit on the keyframe's
    65.  The corners' surroundings are alike, so equal distances abound."""
    i = np.arange(65)
    pts = _plane(24.0 + 16 * (i % 17), 30.0 + 16 * (i // 17))
    got, exp = _stage([_pyr_of("dots", 65)], [IDENT], _pyr_of("dots", k), pts, max_hamming=256, ratio_permille=1000)
    assert exp["report"][2] == k and exp["report"][1] == 65
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_more_corners_than_max_features():
    ctx = _ctx(64)
    xs, _ = _corners(_tex(SHIFT))
    assert len(xs) > 64
    par = dict(DEFAULTS, min_inliers=6)
    pts = _tex_points()[:300]
    hosts = np.zeros(300, np.int32)
    cur = _pyr_of("tex", SHIFT)
    xs, ys = _corners(_tex(SHIFT))
    exp = ref.reloc_seed([_pyr_of("tex")], [IDENT], pts, hosts, cur, WS, HS, KS, IDENT, xs, ys, max_features=64, **par)
    got = ctx.reloc_seed([_pyr_of("tex")], [IDENT], cur, WS, HS, pts, hosts, IDENT, **par)
    assert 0 < exp["report"][2] <= 64
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_flat_level_ties():
    """Every descriptor is 0 and every distance 0.  One corner: second = 257,
    every point's best is that corner, the corner's best point is the lowest
    index: exactly point 0 is matched.  Three corners: best = second = 0 fails
    the ratio test for every point."""
    pts = _tex_points()[:70]
    kf = _pyr_of("tex", 0, True)
    got, exp = _stage([kf], [IDENT], _pyr_of("dots", 1, True), pts)
    assert exp["report"][3] == 1 and exp["matches"].tolist() == [[0, 0, 0]] and exp["report"][0] == 1
    assert (exp["per_point"][:, 2] == 0).all()
    _same(got, exp, "one corner")
    got, exp = _stage([kf], [IDENT], _pyr_of("dots", 3, True), pts)
    assert exp["report"][3] == 0 and exp["report"][2] == 3 and (exp["per_point"][:, :2] == 0).all()
    _same(got, exp, "three corners")


@pytest.mark.gpu
def test_gpu_stage_border_and_behind():
    """Points in the 6-pixel border of level 1 (level-0 pixel below 12 or from
    w - 12), outside the image and behind the camera are not described."""
    good = _tex_points()[:40]
    border = _plane([11.4, 3.0, WS - 12.0, 100.0, 100.0, 11.6], [100.0, 100.0, 100.0, 11.4, HS - 12.0, 100.0])
    outside = _plane([-5.0, WS + 4.0], [100.0, 100.0])
    behind = good[:5] * np.array([1.0, 1.0, -1.0])
    pts = np.concatenate([good[:20], border, outside, behind, good[20:]])
    got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), pts)
    # 11.6 rounds to the level-0 pixel 12, level-1 pixel 6: the only border point described
    assert exp["report"][1] == 41
    _same(got, exp)


@functools.lru_cache(maxsize=None)
def _full():
    """The restatement on the 300 first texture points: the pool the crafted
    cases take their matches from."""
    pts = _tex_points()[:300]
    xs, ys = _corners(_tex(SHIFT))
    r = ref.reloc_seed([_pyr_of("tex")], [IDENT], pts, np.zeros(300, np.int32), _pyr_of("tex", SHIFT), WS, HS, KS,
                       IDENT, xs, ys, **dict(DEFAULTS, min_inliers=6))
    assert r["report"][0] == 0 and r["report"][3] >= 40
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3])
def test_gpu_stage_two_and_three_matches(m):
    pts = _tex_points()[:300][_full()["matches"][:m, 0]]
    got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), pts)
    assert exp["report"][3] == m and exp["report"][0] == (1 if m == 2 else 2)  # 3 inliers at most: below min_inliers
    assert m == 2 or exp["report"][4] > 0
    _same(got, exp)


@functools.lru_cache(maxsize=None)
def _collinear():
    """Three matched points of the pool on one image row: on the plane z = ZS
    they lie on one world line."""
    full, pts = _full(), _tex_points()[:300]
    rows = {}
    for p, c, _ in full["matches"]:
        rows.setdefault(int(full["kept"][c][1]), []).append(int(p))
    row = min(y for y, v in rows.items() if len(v) >= 3)
    return pts[sorted(rows[row])[:3]]


@pytest.mark.gpu
def test_gpu_stage_collinear_matches():
    """Three collinear matches: a rotation about their line moves no
    projection, so H has rank 5.  In fp64 its last pivot is rounding, not 0, so
    inverse6 returns large finite numbers: whether a hypothesis ends unsolved
    (a step overflows or a depth turns negative) is decided by that rounding.
    Both sides must decide alike in every one of the 256 hypotheses (the six
    ordered triples), which is what parity asserts (both solve all 256: the
    points on the line do not move under the spurious rotation); the exactly
    singular H is test_gpu_stage_unsolved's second case."""
    got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), _collinear())
    print("collinear: solved", exp["report"][4], "of", DEFAULTS["hypotheses"])
    assert exp["report"][3] == 3 and exp["report"][0] == 2
    _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_unsolved():
    """S behind the points: a depth <= 0 in the first pass.  S at an infinite
    depth: every Jacobian entry but two is 0, H is exactly singular, the step
    is not finite.  No hypothesis is solved: status 2, the pose out is S."""
    pts = _tex_points()[:300]
    behind, far = IDENT.copy(), IDENT.copy()
    behind[11], far[11] = -2 * ZS, np.inf
    for S in (behind, far):
        got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), pts, start=S)
        assert exp["report"][3] >= 40 and exp["report"][4] == 0 and exp["report"][0] == 2 and exp["report"][5] == -1
        assert np.array_equal(exp["pose"], S)
        _same(got, exp)


@pytest.mark.gpu
def test_gpu_stage_min_inliers_above_the_best_score():
    pts = _tex_points()[:300]
    best = int(_full()["report"][6])
    got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), pts, min_inliers=best + 1)
    assert exp["report"][0] == 2 and exp["report"][6] == best and np.array_equal(exp["pose"], IDENT)
    _same(got, exp, "above")
    got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), pts, min_inliers=best)
    assert exp["report"][0] == 0
    _same(got, exp, "at")


@pytest.mark.gpu
@pytest.mark.parametrize("hyp", [1, 4096])
def test_gpu_stage_hypothesis_counts(hyp):
    """4,096 hypotheses on seven matches: 210 ordered triples, each computed
    once by the restatement.  The seven are spread over the match list, which
    is in row order: seven neighbours in the list lie in two or three image
    rows, their triples are close to collinear, and the solve then amplifies a
    last-bit difference of sin / cos (the device's against libm's) into the
    pose — the first run of this test on the device showed that, at equal
    integers, in the refinement's cost."""
    m = _full()["matches"]
    pts = _tex_points()[:300][m[np.linspace(0, len(m) - 1, 7).astype(int), 0]]
    got, exp = _stage([_pyr_of("tex")], [IDENT], _pyr_of("tex", SHIFT), pts, hypotheses=hyp, seed=11)
    assert exp["report"][3] == 7 and exp["report"][4] <= hyp
    if hyp == 4096:
        assert exp["report"][0] == 0 and exp["report"][6] == 7
    _same(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,mode", [(1, "all"), (2, "mixed"), (2, "second"), (8, "tie"), (8, "mixed")])
def test_gpu_stage_keyframes_and_hosts(n_kf, mode):
    """The keyframes are copies, so the matches do not depend on the hosts and
    the hosts of the inliers can be dealt to make k* and its tie."""
    pts = _tex_points()[:300]
    full = _full()
    inl = full["matches"][full["inliers"] != 0, 0]
    hosts = (np.arange(300) % n_kf).astype(np.int32)
    if mode == "tie":  # keyframes 3 and 5 share the lead (an odd inlier is keyframe 7's): the lower wins
        k = len(inl) & ~1
        hosts[inl] = 7
        hosts[inl[:k:2]], hosts[inl[1:k:2]] = 5, 3
        want = 3
    elif mode == "second":
        hosts[inl] = 1
        want = 1
    else:
        want = None
    got, exp = _stage([_pyr_of("tex")] * n_kf, [IDENT] * n_kf, _pyr_of("tex", SHIFT), pts, hosts)
    assert np.array_equal(exp["matches"], full["matches"]) and exp["report"][0] == 0
    if want is not None:
        assert exp["report"][10] == want
    _same(got, exp)


# ------------------------------------------------------------------ GPU: the descriptor's known answer (6)
@pytest.mark.gpu
@pytest.mark.parametrize("gx,gy", RAMPS)
def test_gpu_descriptor_known_answer(gx, gy):
    """64x64: level 1 is 32x32.  The keyframe's level 1 is a ramp, the current
    frame's is flat (descriptor 0), one point meets one corner: the distance
    of the one match is the ramp descriptor's popcount, written down from the
    offsets."""
    from viso_amd import api
    ctx = api.Context(api.default_params(fx=100.0, fy=100.0, cx=32.0, cy=32.0, width=64, height=64))
    img = np.full((64, 64), 100, np.uint8)
    img[32, 32] = 255
    xs, ys = _corners(img)
    assert list(xs) == [32] and list(ys) == [32]
    cur = oracle_lib.pyramid(img).copy()
    cur[4096:4096 + 1024] = 100
    kf = cur.copy()
    kf[4096:4096 + 1024] = _ramp(gx, gy).ravel()
    pts = np.array([[0.0, 0.0, 5.0]])
    try:
        got = ctx.reloc_seed([kf], [IDENT], cur, 64, 64, pts, [0], IDENT, max_hamming=256, ratio_permille=1000)
    finally:
        ctx.close()
    want = int(_ramp_bits(gx, gy).sum())
    print("distance", got["matches"], "expected", want)
    assert got["matches"].tolist() == [[0, 0, want]] and list(got["report"][:4]) == [1, 1, 1, 1]
    exp = ref.reloc_seed([kf], [IDENT], pts, [0], cur, 64, 64, (100.0, 100.0, 32.0, 32.0), IDENT, xs, ys,
                         max_hamming=256, ratio_permille=1000)
    assert np.array_equal(got["matches"], exp["matches"])


# ------------------------------------------------------------------ GPU: the frame path (7)
RELOC = (1, tr.MAX_COST, 500, 0, 10, 512)
_runs = {}


def _run(seed_on, batched=False):
    key = (seed_on, batched)
    if key not in _runs:
        g = _gap()
        n = g + 4
        gv = tr._viso(reloc=RELOC)
        if seed_on:
            gv.set_reloc_seed()
        gv.ctx.timing_enable(True)
        gv.process(tr._image(0), tr._image(0, 1))
        assert gv.state == 1
        if batched:
            import torch
            dl = torch.from_numpy(np.stack([_scene_image(f, g) for f in range(1, n)])).cuda()
            torch.cuda.synchronize()
            gv.process_device(dl.data_ptr(), None, n - 1, W * H)
            gv.synchronize()
        else:
            for f in range(1, n):
                gv.OnNewFrame(_scene_image(f, g))
        _runs[key] = {"poses": gv.poses, "status": list(gv.frame_status()), "info": list(gv.relocalise()),
                      "seed_info": list(gv.reloc_seed()), "report": gv.relocalise_report(),
                      "seed_report": gv.reloc_seed_report() if seed_on else None,
                      "launches": gv.ctx.timing("reloc_seed")[0], "state": gv.state}
        gv.close()
    return _runs[key]


def _check_run(res, m):
    _, E = tr._stereo_map()
    g = m["g"]
    print("statuses", res["status"], "info", res["info"], "seed info", res["seed_info"])
    assert res["status"] == m["status"] and res["state"] == 1
    assert res["info"] == m["info"] and res["seed_info"] == m["seed_info"]
    assert res["launches"] == m["seed_info"][1]
    assert np.allclose(res["poses"], m["poses"], rtol=RTOL, atol=ATOL)
    poses, report = res["report"]
    exp = m["attempt"]
    assert np.array_equal(report[:, tr.INT_COLS], exp["report"][:, tr.INT_COLS])
    assert np.allclose(poses, exp["poses"], rtol=RTOL, atol=ATOL)
    if res["seed_report"] is not None:
        rep, pose = res["seed_report"]
        assert np.array_equal(rep[INT_COLS], m["stage"]["report"][INT_COLS])
        assert np.allclose(pose, m["stage"]["pose"], rtol=RTOL, atol=ATOL)
        err = [tr._terr(p, f + 1) for f, p in enumerate(res["poses"])]
        print("errors", err[g - 1:], "2 E", 2 * E)
        assert max(err[g:g + 3]) <= 2 * E


@pytest.mark.gpu
def test_gpu_frame_path_matches_the_model():
    _check_run(_run(True), _model(True))
    _check_run(_run(False), _model(False))
    assert np.array_equal(_run(True)["poses"][:4], _run(False)["poses"][:4])


@pytest.mark.gpu
def test_gpu_frame_path_device_ingest():
    res = _run(True, batched=True)
    _check_run(res, _model(True))
    assert np.array_equal(res["poses"], _run(True)["poses"])


# ------------------------------------------------------------------ GPU: off is off (8)
@pytest.mark.gpu
def test_gpu_off_is_off():
    """12 frames with an occlusion (frames 5-7 of another scene at 416x128),
    the relocalisation on: never set, and set then cleared."""
    seq = tr._seq_small()
    from viso_amd.synth import Sequence
    other = Sequence(tr.WQ, tr.HQ, seed=7, z_amp=20.0, z_period=1000.0)
    runs = []
    for mode in ("never", "cleared"):
        gv = tr._viso(tr.WQ, tr.HQ, seq, reloc=RELOC)
        if mode == "cleared":
            gv.set_reloc_seed(256, 48, 800, 2.0, 30, 5)
            gv.set_reloc_seed(0)
        gv.ctx.timing_enable(True)
        gv.process(seq.image(0), seq.image(0, 1))
        assert gv.state == 1
        for f in range(1, 13):
            gv.OnNewFrame(other.image(40 + f) if f in (5, 6, 7) else seq.image(f))
        assert gv.ctx.timing("reloc_seed")[0] == 0
        assert list(gv.reloc_seed()) == [0, 0, 0, 0, 0, 0, -1, -1]
        runs.append((gv.poses, gv.GetPoints(), gv.alignment(), gv.frame_log(), gv.relocalise_report(),
                     list(gv.frame_status()), list(gv.relocalise())))
        gv.close()
    a, b = runs
    print("statuses", a[5], "info", a[6])
    assert 2 in a[5]  # the occlusion loses the context: attempts ran
    assert len(a[0]) == 12 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    assert np.array_equal(a[3], b[3], equal_nan=True)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[4], b[4]))
    assert a[5] == b[5] and a[6] == b[6]


# ------------------------------------------------------------------ GPU: ARG and STATE codes (9)
@pytest.mark.gpu
def test_gpu_argument_codes():
    lib, h = _lib().load(), _ctx().h
    pts = np.ascontiguousarray(_tex_points()[:20])
    hosts = np.zeros(20, np.int32)
    kp, cp = np.ascontiguousarray(_pyr_of("tex")), np.ascontiguousarray(_pyr_of("tex", SHIFT))
    pose = IDENT.copy()
    rep, out, mt, fl, n = np.zeros(12), np.zeros(12), np.zeros((20, 3), np.int32), np.zeros(20, np.uint8), \
        np.zeros(1, np.uint64)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(n_kf=1, npt=20, hyp=16, mh=48, rp=800, px=2.0, mi=6, kfp=kp, kpo=pose, cur=cp, p=pts, hs=hosts, st=pose,
             r=rep, o=out, m=mt, f=fl, cap=20, nm=n, wd=WS, ht=HS):
        return lib.viso_reloc_seed(h, ptr(kfp), ptr(kpo), n_kf, ptr(cur), wd, ht, ptr(p), ptr(hs), npt, ptr(st), hyp,
                                   mh, rp, px, mi, 3, ptr(r), ptr(o), ptr(m), ptr(f), cap, ptr(nm))

    assert call() == 0 and call(npt=0, p=None, hs=None) == 0 and call(cap=0, m=None, f=None) == 0
    assert call(hyp=1, mh=1, rp=1) == 0 and call(hyp=4096, mh=256, rp=1000) == 0
    bad_host = hosts.copy()
    bad_host[7] = 1
    for kw in ({"n_kf": 0}, {"n_kf": 9}, {"npt": -1}, {"npt": 16385}, {"hyp": 0}, {"hyp": -1}, {"hyp": 4097},
               {"mh": 0}, {"mh": 257}, {"rp": 0}, {"rp": 1001}, {"px": 0.0}, {"px": -1.0}, {"px": float("nan")},
               {"px": float("inf")}, {"mi": 5}, {"kfp": None}, {"kpo": None}, {"cur": None}, {"p": None},
               {"hs": None}, {"hs": bad_host}, {"st": None}, {"r": None}, {"o": None}, {"m": None}, {"f": None},
               {"nm": None}, {"wd": 0}, {"ht": -3}):
        assert call(**kw) == -1, kw
    info = np.zeros(8, np.int64)
    for args in ((-1, 48, 800, 2.0, 30, 0), (4097, 48, 800, 2.0, 30, 0), (256, 0, 800, 2.0, 30, 0),
                 (256, 257, 800, 2.0, 30, 0), (256, 48, 0, 2.0, 30, 0), (256, 48, 1001, 2.0, 30, 0),
                 (256, 48, 800, 0.0, 30, 0), (256, 48, 800, -2.0, 30, 0), (256, 48, 800, float("nan"), 30, 0),
                 (256, 48, 800, float("inf"), 30, 0), (256, 48, 800, 2.0, 5, 0)):
        assert lib.viso_set_reloc_seed(h, *args) == -1, args
    assert lib.viso_get_reloc_seed_report(h, rep.ctypes.data, out.ctypes.data) == -4  # off: VISO_ERR_STATE
    for args in ((256, 48, 800, 2.0, 30, 0), (1, 1, 1, 0.5, 6, 2 ** 64 - 1), (4096, 256, 1000, 50.0, 16384, 9),
                 (0, 0, 0, 0.0, 0, 0)):
        assert lib.viso_set_reloc_seed(h, *args) == 0, args
        assert lib.viso_get_reloc_seed(h, info.ctypes.data) == 0 and info[0] == (1 if args[0] else 0)
        if args[0]:
            assert lib.viso_get_reloc_seed_report(h, rep.ctypes.data, out.ctypes.data) == 0 and np.isnan(rep).all()
            assert lib.viso_get_reloc_seed_report(h, None, out.ctypes.data) == -1
            assert lib.viso_get_reloc_seed_report(h, rep.ctypes.data, None) == -1
    assert lib.viso_get_reloc_seed(h, None) == -1
    assert list(info) == [0, 0, 0, 0, 0, 0, -1, -1]
