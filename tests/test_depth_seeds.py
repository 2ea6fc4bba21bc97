"""Depth seeds (viso_depth_seeds_*): the map grows by an
epipolar search over the frames after a keyframe.  Every corner of a new
keyframe that the map does not cover becomes a seed with the whole inverse
depth range; every later frame searches the seed's epipolar segment for the
host patch and narrows the range; a converged seed becomes a map point.

The rule is the project's own (the reference has no counterpart); its
restatement is tests/depth_seed_ref.py.  CPU tests check the geometry, that
every status occurs on a rendered plane, that the filter does what it is for
on the synthetic drive, and the decision margins of the GPU parity cases.  GPU
tests compare the three stage entries and the frame path (host calls, a device
chunk, the tolerance mode, the mode off, and all the map's other modes on)
against the restatement.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import depth_seed_ref as ref
from tests import lk_warp_ref as lk
from tests import mono_kf_ref, oracle_lib
from tests.test_lk_warp import IDENT, Plane, _pose, _rz

# ------------------------------------------------------------------ 1. geometry
K1 = (310.0, 290.0, 161.5, 47.25)


def test_pixel_of_an_inverse_depth_and_back():
    rng = np.random.default_rng(1)
    n = 200
    host = _pose(_rz(0.1), (0.3, -0.2, 0.5))
    cur = _pose(_rz(-0.2) @ np.array([[1, 0, 0], [0, np.cos(0.1), -np.sin(0.1)], [0, np.sin(0.1), np.cos(0.1)]]),
                (-0.7, 0.4, -0.6))
    uv = np.stack([rng.uniform(0, 320, n), rng.uniform(0, 96, n)], 1)
    depth = rng.uniform(2.0, 40.0, n)
    rho = 1.0 / depth
    R, t = ref.relative(cur, np.repeat(host[:, None], n, 1))
    f, q = ref.ray(uv, K1, R)
    u, v, z = ref.px(q, t, rho, K1)
    # the host point at depth 1 / rho, through the world into the current camera
    Rh, th = host[:9].reshape(3, 3), host[9:]
    Pw = (np.stack(f, 1) * depth[:, None] - th) @ Rh
    pu, pv, pz = lk.project(cur, K1, (Pw[:, 0], Pw[:, 1], Pw[:, 2]))
    assert np.abs(u - pu).max() < 1e-9 and np.abs(v - pv).max() < 1e-9
    assert np.abs(z * depth - pz).max() < 1e-12 * np.abs(pz).max()
    # an exact match recovers the depth on either axis
    for k, m in ((0, u), (1, v)):
        got = ref.rho_of(m, np.full(n, k), q, t, K1)
        # (where the axis carries parallax at all: 1 px of it over the depth range)
        far = np.abs(ref.px(q, t, np.full(n, 0.5), K1)[k] - ref.px(q, t, np.full(n, 0.025), K1)[k]) > 1.0
        assert far.sum() > n // 2
        assert np.abs(got[far] / rho[far] - 1.0).max() < 1e-12, k


def test_new_rows_and_fusion_known_answers():
    r = ref.new_rows([[10, 20], [30, 40]], 2, 2.0, 50.0)
    assert np.array_equal(r["h"], [2, 2]) and np.array_equal(r["uv"], [[10, 20], [30, 40]])
    assert np.all(r["mu"] == (1 / 50.0 + 1 / 2.0) / 2.0) and np.all(r["s2"] == ((1 / 2.0 - 1 / 50.0) / 4.0) ** 2)
    assert not r["cnt"].any()


# ------------------------------------------------------------------ 2. every status on a rendered plane
W2, H2 = 320, 96
K2 = (300.0, 300.0, 160.0, 48.0)
Z2 = 8.0


@functools.lru_cache(maxsize=None)
def _plane2(kind="noise"):
    plane = Plane(K2, W2, H2, Z0=Z2, seed=21, comps=1 if kind == "stripes" else 48)
    if kind == "stripes":  # a cosine of 8 px period along x
        plane.fu, plane.fv = np.array([0.125]), np.array([0.0])
        plane.ph, plane.amp, plane.gain = np.array([0.3]), np.array([1.0]), 70.0
    return plane


@functools.lru_cache(maxsize=None)
def _render2(kind, tx, tz=0.0):
    p = oracle_lib.pyramid(_plane2(kind).render(_pose(t=(tx, 0.0, tz))))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _seeds2(kind="noise"):
    key = _plane2(kind).render(IDENT)
    rows, winners = ref.create(key, W2, H2, K2, IDENT, np.zeros((0, 3)), 16, 0, 2.0, 60.0, fast_thresh=20)
    assert winners == len(rows["h"]) > 50
    return rows


def _status(rows):
    return set(rows["cnt"][:, 3].tolist())


def test_every_status_occurs_and_the_plane_is_found():
    prm = ref.params(max_steps=32, depth_min=2.0, depth_max=60.0)
    seen = set()
    # a sideways baseline growing over 12 frames, from too small to see
    rows = _seeds2()
    hist = []
    for f in range(12):
        b = 0.002 if f == 0 else 0.04 * f
        rows, dg = ref.update(rows, [_render2("noise", 0.0)], [IDENT], _render2("noise", -b), _pose(t=(-b, 0, 0)),
                              W2, H2, K2, prm)
        st = rows["cnt"][:, 3]
        hist.append(np.bincount(st, minlength=10).tolist())
        seen |= _status(rows)
        if f == 0:
            assert (st[st != 5] == 4).all()  # no parallax yet (5: the corner's patch leaves the keyframe)
            assert not rows["cnt"][:, :2].any()
    print("status counts per frame", hist)
    assert {0, 4, 5, 6} <= seen  # (6: a segment near the border with fewer than 3 steps inside the image)
    out = ref.promote(rows, [IDENT], K2, 10000, prm)
    conv, prom, dropped, surv = out["counts"]
    assert prom == conv >= 0.8 * len(rows["h"]) and dropped >= 1
    rel = np.abs(out["points"][:, 2] - Z2) / Z2
    print("promoted", prom, "median relative depth error", np.median(rel), "largest", rel.max())
    assert np.median(rel) < 0.01 and rel.max() < 0.1
    assert (out["host"] == 0).all() and len(out["rows"]["h"]) == surv
    # 1: out of view (the camera 3 m to the side); 3: a segment of more than 8 x 7 px at max_steps 8
    r1, _ = ref.update(_seeds2(), [_render2("noise", 0.0)], [IDENT], _render2("noise", -3.0), _pose(t=(-3.0, 0, 0)),
                       W2, H2, K2, prm)
    seen |= _status(r1)
    assert 1 in _status(r1) and (r1["cnt"][r1["cnt"][:, 3] == 1, 2] == 1).all()
    r3, _ = ref.update(_seeds2(), [_render2("noise", 0.0)], [IDENT], _render2("noise", -0.5), _pose(t=(-0.5, 0, 0)),
                       W2, H2, K2, ref.params(max_steps=8))
    assert 3 in _status(r3) and not r3["cnt"][r3["cnt"][:, 3] == 3, :3].any()
    seen |= _status(r3)
    # 2: the camera 7.2 m forward of a plane 8 m away: a zoom of 10, |det A| = 100
    near = ref.new_rows([[164.0, 50.0], [157.0, 45.0]], 0, 2.0, 60.0)
    near["mu"][:] = 1.0 / Z2
    near["s2"][:] = 0.002 ** 2
    r2, _ = ref.update(near, [_render2("noise", 0.0)], [IDENT], _render2("noise", 0.0, -7.2), _pose(t=(0, 0, -7.2)),
                       W2, H2, K2, prm)
    assert _status(r2) == {2} and (r2["cnt"][:, 2] == 1).all()
    # 7: a flat current image; 8: stripes of 8 px period; 9: a seed whose mu lies outside the depth range
    flat = np.full_like(_render2("noise", 0.0), 128)
    r7, _ = ref.update(_seeds2(), [_render2("noise", 0.0)], [IDENT], flat, _pose(t=(-0.3, 0, 0)), W2, H2, K2, prm)
    assert 7 in _status(r7) and (r7["cnt"][r7["cnt"][:, 3] == 7, 1] == 1).all()
    stripes = ref.new_rows([[100.0, 40.0], [163.0, 50.0], [220.0, 30.0]], 0, 2.0, 60.0)
    r8, d8 = ref.update(stripes, [_render2("stripes", 0.0)], [IDENT], _render2("stripes", -0.4), _pose(t=(-0.4, 0, 0)),
                        W2, H2, K2, prm)
    assert _status(r8) == {8} and (r8["cnt"][:, 1] == 1).all() and (r8["cnt"][:, 2] == 0).all()
    # (a range narrowed to 2 .. 6 m while the seed lives: mu + 2 sigma = 0.11 < rho_min = 1/6, so the segment
    # runs from rho_min down to 0.11, over the plane's 0.125)
    outside = ref.new_rows([[100.0, 40.0], [163.0, 50.0]], 0, 2.0, 6.0)
    outside["mu"][:] = 0.10
    outside["s2"][:] = 0.005 ** 2
    r9, _ = ref.update(outside, [_render2("noise", 0.0)], [IDENT], _render2("noise", -1.0), _pose(t=(-1.0, 0, 0)),
                       W2, H2, K2, ref.params(max_steps=32, depth_min=2.0, depth_max=6.0))
    assert _status(r9) == {9} and (r9["cnt"][:, 1] == 1).all()
    seen |= _status(r2) | _status(r7) | _status(r8) | _status(r9)
    assert seen == set(range(10))


def test_promotion_classes_and_room():
    prm = ref.params(min_good=3, conv_rel=0.05, max_bad=4, max_lost=4)
    rows = ref.new_rows(np.arange(16).reshape(8, 2), 0, 2.0, 60.0)
    rows["h"][:] = [0, 1, 0, 1, 0, 1, 0, 1]
    rows["mu"][:] = 0.125
    tight = (0.05 * 0.125) ** 2
    rows["s2"][:] = [tight, tight, np.nextafter(tight, 1.0), tight, 1.0, tight, 1.0, tight]
    #            converged  good<3   s2 above   conv+bad  dropped   conv  lost    conv
    rows["cnt"][:, :3] = [[3, 0, 0], [2, 0, 0], [9, 0, 0], [3, 4, 0], [0, 4, 0], [5, 0, 3], [0, 0, 4], [3, 0, 0]]
    kf = np.stack([IDENT, _pose(t=(0.5, 0.0, 0.0))])
    full = ref.promote(rows, kf, K2, 100, prm)
    assert full["counts"] == [4, 4, 2, 2]
    assert np.array_equal(full["host"], [0, 1, 1, 1]) and np.array_equal(full["rows"]["uv"][:, 0], [2, 4])
    # R_h^T (f / mu - t_h) of the first and the second promoted seed
    assert np.allclose(full["points"][0], [(0 - K2[2]) / K2[0] * 8.0, (1 - K2[3]) / K2[1] * 8.0, 8.0], rtol=1e-15)
    assert np.allclose(full["points"][1], [(6 - K2[2]) / K2[0] * 8.0 - 0.5, (7 - K2[3]) / K2[1] * 8.0, 8.0], rtol=1e-15)
    two = ref.promote(rows, kf, K2, 2, prm)  # a converged seed that does not fit stays a seed
    assert two["counts"] == [4, 2, 2, 4]
    assert np.array_equal(two["points"], full["points"][:2])
    assert np.array_equal(two["rows"]["uv"][:, 0], [2, 4, 10, 14])
    none = ref.promote(rows, kf, K2, 0, prm)
    assert none["counts"] == [4, 0, 2, 6] and len(none["points"]) == 0


# ------------------------------------------------------------------ 3. it does what it is for
W3, H3 = 320, 96
KF3, LAST3 = 4, 20
MEASURED = {}


@functools.lru_cache(maxsize=None)
def _seq3():
    from viso_amd.synth import Sequence
    return Sequence(W3, H3, seed=0, z_amp=20.0, z_period=1000.0)  # forward, with the sideways sway


def _scene_depth(seq, pose, uv):
    """The depth (z in the camera of `pose`) of the synthetic scene's box at
    the pixels uv: the nearest of its back wall, side walls and ground."""
    p, K = seq.p, seq.K
    R, t = pose[:9].reshape(3, 3), pose[9:]
    C = -R.T @ t
    dc = np.stack([(uv[:, 0] - K[2]) / K[0], (uv[:, 1] - K[3]) / K[1], np.ones(len(uv))], 1)
    d = dc @ R
    best = np.full(len(uv), 1e30)
    for ax, val in ((2, p.wall_z), (0, -p.wall_x), (0, p.wall_x), (1, p.ground_y)):
        with np.errstate(all="ignore"):
            tt = (val - C[ax]) / d[:, ax]
        best = np.where((np.abs(d[:, ax]) >= 1e-12) & (tt > 0.1) & (tt < best), tt, best)
    return best


def test_filter_against_two_view_triangulation():
    seq = _seq3()
    K = seq.K
    pyr = lambda f: oracle_lib.pyramid(seq.image(f))
    prm = ref.params(max_steps=32, depth_min=2.0, depth_max=60.0, conv_rel=0.15)
    kp, kpose = pyr(KF3), seq.pose(KF3)
    rows, winners = ref.create(seq.image(KF3), W3, H3, K, kpose, np.zeros((0, 3)), 16, 0, 2.0, 60.0)
    for f in range(KF3 + 1, LAST3 + 1):
        rows, _ = ref.update(rows, [kp], [kpose], pyr(f), seq.pose(f), W3, H3, K, prm)
    out = ref.promote(rows, [kpose], K, 10000, prm)
    R, t = kpose[:9].reshape(3, 3), kpose[9:]
    Pc = out["points"] @ R.T + t
    uv = np.stack([Pc[:, 0] / Pc[:, 2] * K[0] + K[2], Pc[:, 1] / Pc[:, 2] * K[1] + K[3]], 1)
    gt = _scene_depth(seq, kpose, uv)
    med_f = float(np.median(np.abs(Pc[:, 2] - gt) / gt))
    # the two-view step on the same keyframe's winners, against the last frame
    m = mono_kf_ref.mono_points(kp, pyr(LAST3), W3, H3, K, kpose, seq.pose(LAST3), np.zeros((0, 3)), 16, 0.25)
    assert m["counts"][1] == winners
    Pc2 = m["points"] @ R.T + t
    gt2 = _scene_depth(seq, kpose, m["xy"][m["accept"] == 1].astype(np.float64))
    med_t = float(np.median(np.abs(Pc2[:, 2] - gt2) / gt2))
    MEASURED.update(filter=(len(Pc), med_f), two_view=(len(Pc2), med_t), winners=winners)
    print(f"{winners} winners; filter: {len(Pc)} promoted, median relative depth error {med_f:.4f}; two-view: "
          f"{len(Pc2)} accepted, median {med_t:.4f}")
    assert med_f <= 1.5 * med_t
    assert len(Pc) > len(Pc2)


# ------------------------------------------------------------------ 4. the GPU parity cases
W, H = 416, 128
K6 = (300.0, 300.0, 208.0, 64.0)
SIZES = (0, 1, 3, 63, 64, 65, 257, 2049)
STEPS = (8, 64)
KF_POSES = np.stack([IDENT, _pose(_rz(0.05), (-0.5, 0.05, 0.0)), _pose(t=(0.1, 0.0, 2.0))])
CUR_POSES = [_pose(t=(0.02, -0.01, -1.0)),        # forward
             _pose(t=(-0.8, 0.1, 0.0)),           # sideways
             _pose(_rz(0.3), (0.05, 0.0, -0.5))]  # rolled (and a little forward)
DMIN, DMAX = 1.05, 9.0  # (the plane is 8 m from keyframes 0 and 1 and 10 m from keyframe 2)
BAR = 1e-9    # the smallest relative margin a parity seed may have at any of its decisions
DROPPED = {}  # per case: candidates drawn, candidates left out


def _prm(max_steps):
    return ref.params(max_steps=max_steps, depth_min=DMIN, depth_max=DMAX, max_score=64 * 20.0 ** 2, uniqueness=1.5,
                      min_good=3, conv_rel=0.05, max_bad=4, max_lost=4)


@functools.lru_cache(maxsize=None)
def _scene6():
    plane = Plane(K6, W, H, seed=21)
    kfs = [oracle_lib.pyramid(plane.render(p)) for p in KF_POSES]
    curs = [oracle_lib.pyramid(plane.render(p)) for p in CUR_POSES]
    for a in kfs + curs:
        a.setflags(write=False)
    return plane, kfs, curs


def _candidates(rng, m):
    """m candidate seed rows on the three keyframes: 70 % at integer corners;
    60 % with mu near the plane's inverse depth and a sigma of 2e-4 .. 0.25
    (status 0, 3, 4, 6 .. 8), the others anywhere in the depth range (1, 2,
    5, 7); 4 % on keyframe 2 with mu + 2 sigma below the plane's 0.1, which
    lies below rho_min (9: the segment runs from rho_min down over the
    plane); a tenth near the image centre with a depth of 1.05 .. 1.2 (the
    forward frame's rejected warps); counters 0 .. 3."""
    fx, fy, cx, cy = K6
    kind = rng.uniform(size=m)
    out = (kind >= 0.6) & (kind < 0.64)
    h = np.where(out, 2, rng.integers(0, 3, m)).astype(np.int32)
    uv = np.stack([rng.uniform(2, W - 2, m), rng.uniform(2, H - 2, m)], 1)
    uv = np.where(rng.uniform(size=(m, 1)) < 0.7, np.rint(uv), uv)
    true = np.zeros(m)
    for i in range(m):
        R, t = KF_POSES[h[i]][:9].reshape(3, 3), KF_POSES[h[i]][9:]
        dw, tw = R.T @ np.array([(uv[i, 0] - cx) / fx, (uv[i, 1] - cy) / fy, 1.0]), R.T @ t
        true[i] = dw[2] / (8.0 + tw[2])
    rmin, rmax = 1.0 / DMAX, 1.0 / DMIN
    sig = np.exp(rng.uniform(np.log(2e-4), np.log(0.25), m))
    mu = np.where(kind < 0.6, true + sig * rng.uniform(-1.5, 1.5, m),
                  np.exp(rng.uniform(np.log(rmin), np.log(rmax), m)))
    mu = np.clip(mu, rmin, rmax)
    mu_out = rng.uniform(0.075, 0.09, m)
    mu = np.where(out, mu_out, mu)
    sig = np.where(out, 0.5 * (0.0995 - mu_out) * rng.uniform(0.5, 1.0, m), sig)
    near = kind >= 0.9
    uv = np.where(near[:, None], np.rint(np.stack([rng.uniform(cx - 40, cx + 40, m), rng.uniform(cy - 30, cy + 30, m)],
                                                  1)), uv)
    mu = np.where(near, 1.0 / rng.uniform(1.05, 1.2, m), mu)
    sig = np.where(near, rng.uniform(0.0005, 0.004, m), sig)
    rows = ref.empty_rows(m)
    rows["h"][:], rows["uv"][:], rows["mu"][:], rows["s2"][:] = h, uv, mu, sig * sig
    rows["cnt"][:, :3] = rng.integers(0, 4, (m, 3))
    return rows


def _cur_of(n):
    return SIZES.index(n) % 3


@functools.lru_cache(maxsize=None)
def _case6(n, max_steps):
    """The n seeds of a parity case and their expected update: the first n of
    the case's seeded candidate stream whose every decision, in the
    restatement alone, is more than BAR (relative) clear.  A seed's row
    depends on no other seed, so the chosen set has the margins the choice
    saw."""
    _, kfs, curs = _scene6()
    c = _cur_of(n)
    rng = np.random.default_rng(1000 * max_steps + n)
    kept, drawn = ref.empty_rows(0), 0
    while len(kept["h"]) < n:
        need = n - len(kept["h"])
        cand = _candidates(rng, need + 8)
        _, dg = ref.update(cand, kfs, KF_POSES, curs[c], CUR_POSES[c], W, H, K6, _prm(max_steps))
        clear = dg["margin"] > BAR
        drawn += int(min(len(clear), np.searchsorted(np.cumsum(clear), need) + 1))
        kept = ref.take_rows(ref.concat_rows(kept, ref.take_rows(cand, np.nonzero(clear)[0])), slice(0, n))
    DROPPED[(n, max_steps)] = (drawn, drawn - n)
    exp, dg = ref.update(kept, kfs, KF_POSES, curs[c], CUR_POSES[c], W, H, K6, _prm(max_steps))
    for r in (kept, exp):
        for a in r.values():
            a.setflags(write=False)
    return kept, exp, dg


def test_parity_cases_cover_every_status_with_clear_margins():
    status, levels, shifts, worst = set(), set(), set(), np.inf
    for ms in STEPS:
        for n in SIZES:
            rows, exp, dg = _case6(n, ms)
            assert len(rows["h"]) == n
            status |= set(exp["cnt"][:, 3].tolist())
            levels |= set(dg["l"][dg["l"] >= 0].tolist())
            shifts |= set(dg["shift"][exp["cnt"][:, 3] == 0].tolist())
            if n:
                worst = min(worst, float(dg["margin"].min()))
            drawn, left = DROPPED[(n, ms)]
            assert left <= 0.15 * drawn, (n, ms, drawn, left)
            # the promotion of the updated rows decides clear of its bound too
            _, m = ref.classify(exp, _prm(ms))
            assert n == 0 or m.min() > BAR
    print("smallest decision margin", worst, "; candidates drawn and left out per case", DROPPED)
    print("levels", sorted(levels), "shifts of the fused seeds", sorted(shifts))
    assert status == set(range(10))
    assert levels == {0, 1, 2, 3} and {-1, 0} <= shifts
    assert worst > BAR
    _, exp, dg = _case6(2049, 64)
    assert (exp["cnt"][:, 3] == 0).sum() > 300
    js = dg["jstar"][exp["cnt"][:, 3] == 0]
    assert js.min() == 0 and js.max() >= 40  # the first step, and steps only a long search has


# ------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _ctx(fast=False):
    from viso_amd import api
    fx, fy, cx, cy = K6
    kw = {"precision": 1} if fast else {}
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=W, height=H, **kw))


BITS = {"mu": True, "s2": True, "points": True}
WORST = {"mu": 0.0, "s2": 0.0, "points": 0.0}


def _reldiff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def _check_rows(got, exp, where):
    assert np.array_equal(got["h"], exp["h"]), where
    assert np.array_equal(got["uv"], exp["uv"]), where
    assert np.array_equal(got["cnt"], exp["cnt"]), where
    for k in ("mu", "s2"):
        d = _reldiff(got[k], exp[k])
        WORST[k] = max(WORST[k], d)
        BITS[k] &= np.array_equal(got[k], exp[k])
        assert d <= 1e-9, (where, k, d)


def _update_gpu(ctx, rows, c, max_steps):
    _, kfs, curs = _scene6()
    p = _prm(max_steps)
    return ctx.depth_seeds_update(rows, kfs, KF_POSES, curs[c], CUR_POSES[c], W, H, max_steps, DMIN, DMAX,
                                  p["max_score"], p["uniqueness"])


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_gpu_update_matches_restatement(n, max_steps):
    rows, exp, dg = _case6(n, max_steps)
    got, ls = _update_gpu(_ctx(), rows, _cur_of(n), max_steps)
    where = f"n = {n}, max_steps = {max_steps}"
    _check_rows(got, exp, where)
    assert np.array_equal(ls[:, 0], dg["l"]), where
    assert np.array_equal(ls[:, 1], dg["jstar"]), where
    print(f"{where}: bit-equal mu {np.array_equal(got['mu'], exp['mu'])}, s2 {np.array_equal(got['s2'], exp['s2'])}; "
          f"status counts {np.bincount(exp['cnt'][:, 3], minlength=10).tolist()}")


@pytest.mark.gpu
def test_gpu_update_in_tolerance_mode_gives_the_same_rows():
    for n, ms in ((65, 8), (257, 64)):
        rows, exp, dg = _case6(n, ms)
        got, ls = _update_gpu(_ctx(True), rows, _cur_of(n), ms)
        _check_rows(got, exp, f"fast, n = {n}")
        assert np.array_equal(ls[:, 1], dg["jstar"])


@pytest.mark.gpu
def test_gpu_second_update_follows_the_first():
    """Two frames in a row through the stage entry: the rows the GPU wrote are
    what the restatement continues from."""
    _, kfs, curs = _scene6()
    rows, exp, _ = _case6(257, 64)
    c = _cur_of(257)
    got, _ = _update_gpu(_ctx(), rows, c, 64)
    c2 = (c + 1) % 3
    exp2, dg2 = ref.update(got, kfs, KF_POSES, curs[c2], CUR_POSES[c2], W, H, K6, _prm(64))
    got2, ls2 = _update_gpu(_ctx(), got, c2, 64)
    clear = dg2["margin"] > BAR
    assert clear.mean() > 0.85
    for k in ("cnt", "mu", "s2"):
        assert np.array_equal(got2[k][clear], exp2[k][clear]), k


# ------------------------------------------------------------------ GPU: creation
@functools.lru_cache(maxsize=None)
def _image6(i=0):
    plane, _, _ = _scene6()
    img = plane.render(KF_POSES[i])
    img.setflags(write=False)
    return img


def _every_cell_points(cell, pose):
    """A point 8 m in front of `pose` at the centre of every cell."""
    fx, fy, cx, cy = K6
    uv = np.array([[x + 0.5 * min(cell, W - x), y + 0.5 * min(cell, H - y)] for y in range(0, H, cell)
                   for x in range(0, W, cell)])
    Pc = np.stack([(uv[:, 0] - cx) / fx * 8.0, (uv[:, 1] - cy) / fy * 8.0, np.full(len(uv), 8.0)], 1)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    return (Pc - t) @ R


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["empty map, cell 16", "cell 8", "cell 64", "every cell marked", "half the map",
                                  "the cap"])
def test_gpu_create_matches_restatement(case):
    ctx = _ctx()
    thresh = int(ctx.params.fast_thresh)
    pose, img, host = KF_POSES[1], _image6(1), 1
    cell = {"cell 8": 8, "cell 64": 64}.get(case, 16)
    pts = np.zeros((0, 3))
    n_live = 0
    if case == "every cell marked":
        pts = _every_cell_points(cell, pose)
    elif case == "half the map":
        pts = _every_cell_points(cell, pose)[::2]
    elif case == "the cap":
        n_live = ref.K_MAX_SEEDS - 5
    exp, winners = ref.create(img, W, H, K6, pose, pts, cell, host, DMIN, DMAX, n_live=n_live, fast_thresh=thresh,
                              max_features=int(ctx.params.max_features))
    got, counts = ctx.depth_seeds_create(img, pose, pts, cell, host, DMIN, DMAX, n_live)
    print(case, "winners", winners, "seeds", len(exp["h"]))
    assert counts == [winners, len(exp["h"])]
    for k in exp:
        assert np.array_equal(got[k], exp[k]), (case, k)
    if case == "every cell marked":
        assert winners == 0
    elif case == "the cap":
        assert len(exp["h"]) == 5 < winners
    else:
        assert winners >= 14  # (cell 64: the image has 7 x 2 cells)


# ------------------------------------------------------------------ GPU: promotion
def _promotable(n, max_steps):
    """The updated rows of a parity case with counters that let every class occur."""
    _, exp, _ = _case6(n, max_steps)
    rows = ref.copy_rows(exp)
    rng = np.random.default_rng(n)
    rows["cnt"][:, :3] = rng.integers(0, 6, (n, 3))
    tight = rng.uniform(size=n) < 0.4
    rows["s2"][:] = np.where(tight, (0.03 * rows["mu"]) ** 2, rows["s2"])
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_promote_matches_restatement(n):
    ctx = _ctx()
    rows = _promotable(n, 64)
    prm = _prm(64)
    conv = ref.promote(rows, KF_POSES, K6, 100000, prm)["counts"][0]
    for room in (0, 1, conv + 7):
        exp = ref.promote(rows, KF_POSES, K6, room, prm)
        got = ctx.depth_seeds_promote(rows, KF_POSES, room, prm["min_good"], prm["conv_rel"], prm["max_bad"],
                                      prm["max_lost"])
        where = f"n = {n}, room = {room}"
        assert got["counts"] == exp["counts"], where
        assert np.array_equal(got["host"], exp["host"]), where
        for k in exp["rows"]:
            assert np.array_equal(got["rows"][k], exp["rows"][k]), (where, k)
        d = _reldiff(got["points"], exp["points"])
        WORST["points"] = max(WORST["points"], d)
        BITS["points"] &= np.array_equal(got["points"], exp["points"])
        assert d <= 1e-9, where
    if n >= 63:
        c = ref.promote(rows, KF_POSES, K6, 100000, prm)["counts"]
        assert min(c) > 0, c  # converged, promoted, dropped and survivors all occur


# ------------------------------------------------------------------ GPU: arguments
@pytest.mark.gpu
def test_gpu_stage_entry_arguments():
    from viso_amd import _lib
    ctx = _ctx()
    _, kfs, curs = _scene6()
    rows, _, _ = _case6(3, 8)
    p = _prm(8)
    good = dict(max_steps=8, depth_min=DMIN, depth_max=DMAX, max_score=p["max_score"], uniqueness=1.5)

    def upd(r=rows, kf_poses=KF_POSES, **kw):
        a = dict(good, **kw)
        return ctx.depth_seeds_update(r, kfs[:len(kf_poses)], kf_poses, curs[0], CUR_POSES[0], W, H, **a)

    upd()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(max_steps=7), dict(max_steps=65), dict(depth_min=0.0), dict(depth_min=-1.0),
                dict(depth_min=DMAX), dict(depth_max=inf), dict(depth_min=nan), dict(max_score=0.0),
                dict(max_score=nan), dict(max_score=inf), dict(uniqueness=0.999), dict(uniqueness=nan)):
        with pytest.raises(_lib.VisoError) as e:
            upd(**bad)
        assert e.value.rc == -1, bad
    far = ref.copy_rows(rows)
    far["h"][1] = 3  # a host the call has no keyframe for
    with pytest.raises(_lib.VisoError) as e:
        upd(far)
    assert e.value.rc == -1
    far["h"][1] = -1
    with pytest.raises(_lib.VisoError) as e:
        upd(far)
    assert e.value.rc == -1
    lib = _lib.load()
    z = np.zeros(64)
    zi = np.zeros(64, np.int32)
    pz, pzi = z.ctypes.data, zi.ctypes.data
    kfp = np.ascontiguousarray(np.stack(kfs))
    # NULL context, pyramids, poses, rows; counts out of range
    assert lib.viso_depth_seeds_update(None, kfp.ctypes.data, KF_POSES.ctypes.data, 3, curs[0].ctypes.data, pz, W, H, 1,
                                       8, DMIN, DMAX, 100.0, 1.5, pzi, pz, pz, pz, pzi, None) == -1
    for kw in (dict(kf=None), dict(kp=None), dict(cur=None), dict(cp=None), dict(h=None), dict(mu=None),
               dict(n_kf=0), dict(n_kf=9), dict(n=-1), dict(n=8193), dict(w=8)):
        a = dict(kf=kfp.ctypes.data, kp=KF_POSES.ctypes.data, cur=curs[0].ctypes.data, cp=pz, h=pzi, mu=pz, n_kf=3, n=1,
                 w=W)
        a.update(kw)
        rc = lib.viso_depth_seeds_update(ctx.h, a["kf"], a["kp"], a["n_kf"], a["cur"], a["cp"], a["w"], H, a["n"], 8,
                                         DMIN, DMAX, 100.0, 1.5, a["h"], pz, a["mu"], pz, pzi, None)
        assert rc == -1, kw
    # promotion
    for bad in (dict(min_good=0), dict(min_good=1001), dict(conv_rel=0.0), dict(conv_rel=1.001), dict(conv_rel=nan),
                dict(max_bad=0), dict(max_bad=1001), dict(max_lost=0), dict(max_lost=1001), dict(room=-1),
                dict(room=16385)):
        a = dict(room=10, min_good=3, conv_rel=0.05, max_bad=4, max_lost=4)
        a.update(bad)
        with pytest.raises(_lib.VisoError) as e:
            ctx.depth_seeds_promote(rows, KF_POSES, **a)
        assert e.value.rc == -1, bad
    cnt4 = np.zeros(4, np.int32)
    assert lib.viso_depth_seeds_promote(ctx.h, None, 3, 1, 3, 0.05, 4, 4, 1, pzi, pz, pz, pz, pzi, pz, pzi,
                                        cnt4.ctypes.data) == -1
    assert lib.viso_depth_seeds_promote(ctx.h, KF_POSES.ctypes.data, 3, 1, 3, 0.05, 4, 4, 1, pzi, pz, pz, pz, pzi, None,
                                        pzi, cnt4.ctypes.data) == -1
    assert lib.viso_depth_seeds_promote(ctx.h, KF_POSES.ctypes.data, 3, 1, 3, 0.05, 4, 4, 1, pzi, pz, pz, pz, pzi, pz,
                                        pzi, None) == -1
    # creation
    img = _image6(0)
    for bad in (dict(cell=7), dict(cell=65), dict(host=-1), dict(host=8), dict(depth_min=0.0), dict(depth_min=50.0),
                dict(depth_max=inf), dict(n_live=-1), dict(n_live=8193)):
        a = dict(cell=16, host=0, depth_min=DMIN, depth_max=DMAX, n_live=0)
        a.update(bad)
        with pytest.raises(_lib.VisoError) as e:
            ctx.depth_seeds_create(img, IDENT, np.zeros((0, 3)), **a)
        assert e.value.rc == -1, bad
    n = ctypes.c_size_t(0)
    assert lib.viso_depth_seeds_create(ctx.h, None, W, H, pz, None, 0, 16, 0, DMIN, DMAX, 0, pzi, pz, pz, pz, pzi, 1,
                                       ctypes.byref(n), None) == -1
    assert lib.viso_depth_seeds_create(ctx.h, img.ctypes.data, W, H, pz, None, 5, 16, 0, DMIN, DMAX, 0, pzi, pz, pz, pz,
                                       pzi, 1, ctypes.byref(n), None) == -1
    assert _lib.KERNEL_IDS["seeds"] == 14
    for name in ("viso_depth_seeds_create", "viso_depth_seeds_update", "viso_depth_seeds_promote"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


@pytest.mark.gpu
def test_gpu_stage_entries_run_through_the_timed_launch():
    ctx = _ctx()
    rows, _, _ = _case6(65, 8)
    ctx.timing_enable(True)
    try:
        before = ctx.timing("seeds")[0]
        _update_gpu(ctx, rows, _cur_of(65), 8)
        ctx.depth_seeds_promote(rows, KF_POSES, 10)
        assert ctx.timing("seeds")[0] == before + 2
    finally:
        ctx.timing_enable(False)


# ------------------------------------------------------------------ the C++ facade
def _build_cpp(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "depth_seeds_check")
    libdir = os.path.join(root, "viso_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "depth_seeds_check.cpp"), "-L", libdir, "-lviso_amd",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    return exe


def test_cpp_facade_compiles_and_links(tmp_path):
    import subprocess
    out = subprocess.run([_build_cpp(tmp_path)], capture_output=True, text=True, check=True)
    assert "depth seeds facade ok" in out.stdout


@pytest.mark.gpu
def test_gpu_cpp_facade_runs(tmp_path):
    import subprocess
    out = subprocess.run([_build_cpp(tmp_path), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "depth seeds facade ok" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------ GPU: the frame path
WP, HP = 320, 96
SEEDS = dict(interval=4, cell=16, max_steps=32, depth_min=2.0, depth_max=60.0, max_score=57600.0, uniqueness=1.5,
             min_good=3, conv_rel=0.15, max_bad=4, max_lost=4)
# (a monocular map has the scale of its first baseline: its depths are about 1)
SEEDS_MONO = dict(SEEDS, depth_min=0.1, depth_max=5.0, cell=8)


@functools.lru_cache(maxsize=None)
def _seqp():
    from viso_amd.synth import Sequence
    return Sequence(WP, HP, seed=0, z_amp=20.0, z_period=1000.0)


@functools.lru_cache(maxsize=None)
def _imgp(f, cam=0):
    img = _seqp().image(f, cam)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _pyrp(f):
    p = oracle_lib.pyramid(_imgp(f))
    p.setflags(write=False)
    return p


def _gv(seeds=None, stereo=True, fast=False, **modes):
    import viso_amd
    seq = _seqp()
    kw = {"precision": 1} if fast else {}
    gv = viso_amd.Viso(*seq.K, width=WP, height=HP, enable_tracking=1, batch_frames=32, **kw)
    if stereo:
        gv.set_stereo(seq.p.baseline, 128, 1)
    if modes.get("cull"):
        gv.set_point_cull(*modes["cull"])
    if modes.get("refine"):
        gv.set_pose_refine(*modes["refine"])
    if modes.get("prefine"):
        gv.set_point_refine(*modes["prefine"])
    if modes.get("mono"):
        gv.set_mono_keyframes(*modes["mono"])
    if modes.get("window"):
        gv.set_map_window(*modes["window"])
    if modes.get("warp"):
        gv.set_lk_warp(1, modes["warp"])
    if seeds:
        gv.set_depth_seeds(**seeds)
    return gv


def _start(gv, stereo=True):
    """Initialise: returns the index of the frame that created the map."""
    if stereo:
        gv.process(_imgp(0), _imgp(0, 1))
        assert gv.state == 1
        return 0
    for f in range(12):
        gv.OnNewFrame(_imgp(f))
        if gv.state == 1:
            return f
    raise AssertionError("no monocular initialisation")


def _prm_of(seeds):
    return ref.params(**{k: v for k, v in seeds.items() if k not in ("interval", "cell")})


def _rows_equal(got, exp, where):
    assert len(got["h"]) == len(exp["h"]), where
    assert np.array_equal(got["h"], exp["h"]) and np.array_equal(got["uv"], exp["uv"]), where
    assert np.array_equal(got["cnt"], exp["cnt"]), where
    for k in ("mu", "s2"):
        d = _reldiff(got[k], exp[k])
        WORST[k] = max(WORST[k], d)
        BITS[k] &= np.array_equal(got[k], exp[k])
        assert d <= 1e-9, (where, k, d)


class _Model:
    """The restatement carried along a run: fed the GPU's own pose, keyframe
    poses and map after every frame."""

    def __init__(self, gv, seeds, kf_frames):
        self.seeds, self.prm = seeds, _prm_of(seeds)
        self.K = _seqp().K
        self.thresh, self.feat = int(gv.params.fast_thresh), int(gv.params.max_features)
        self.kf_frames = list(kf_frames)
        self.kf_poses = gv.keyframe_poses()
        self.points = gv.GetPoints()
        self.rows = ref.empty_rows(0)
        self.track = 0
        self.created = self.promoted = self.dropped = self.retired_seeds = 0
        self.events = []
        self._create(self.kf_frames[-1], self.kf_poses[-1])

    def _create(self, f, pose):
        new, _ = ref.create(_imgp(f), WP, HP, self.K, pose, self.points, self.seeds["cell"], len(self.kf_poses) - 1,
                            self.prm["depth_min"], self.prm["depth_max"], n_live=len(self.rows["h"]),
                            fast_thresh=self.thresh, max_features=self.feat)
        self.rows = ref.concat_rows(self.rows, new)
        self.created += len(new["h"])

    def frame(self, gv, f, pose, retired, check_points=True):
        """Frame f has run on the GPU at `pose`: the expected rows after it."""
        self.track += 1
        n_before = len(self.points)
        rows, _ = ref.update(self.rows, [_pyrp(k) for k in self.kf_frames], self.kf_poses, _pyrp(f), pose, WP, HP,
                             self.K, self.prm)
        promoted = None
        if self.track % self.seeds["interval"] == 0:
            promoted = ref.promote(rows, self.kf_poses, self.K, 16384 - n_before, self.prm)
            rows = promoted["rows"]
            self.promoted += promoted["counts"][1]
            self.dropped += promoted["counts"][2]
        points, kfp = gv.GetPoints(), gv.keyframe_poses()
        inserted = len(kfp) > len(self.kf_poses) - (1 if retired else 0)
        if retired:
            keep = np.nonzero(rows["h"] > 0)[0]
            self.dropped += len(rows["h"]) - len(keep)
            self.retired_seeds += len(rows["h"]) - len(keep)
            rows = ref.take_rows(rows, keep)
            rows["h"] -= 1
            self.kf_frames.pop(0)
        self.rows, self.points, self.kf_poses = rows, points, kfp
        if inserted:
            self.kf_frames.append(f)
            self._create(f, pose)
        assert len(self.kf_frames) == len(kfp)
        self.events.append((f, len(self.rows["h"]), 0 if promoted is None else promoted["counts"][1], retired, inserted,
                            len(points)))
        if promoted is not None and promoted["counts"][1] and check_points:
            m = promoted["counts"][1]
            assert len(points) == n_before + m, f
            d = _reldiff(points[n_before:], promoted["points"])
            WORST["points"] = max(WORST["points"], d)
            BITS["points"] &= np.array_equal(points[n_before:], promoted["points"])
            assert d <= 1e-9, f
            assert np.array_equal(points[:n_before], self.pre_points)
            assert np.array_equal(gv.point_hosts()[n_before:], promoted["host"]), f
        return promoted


N_TRACK = 16
_pipe = {}


def _pipeline(mode):
    """mode: "host" (frame by frame), "chunk" (the tracking frames as one
    device chunk) — monocular initialisation, then N_TRACK tracking frames."""
    if mode in _pipe:
        return _pipe[mode]
    gv = _gv(SEEDS_MONO, stereo=False)
    gv.ctx.timing_enable(True)
    f0 = _start(gv, stereo=False)
    res = {"f0": f0, "first_rows": gv.depth_seed_rows(), "first_info": gv.depth_seeds().tolist()}
    if mode == "chunk":
        import torch
        dl = torch.from_numpy(np.stack([_imgp(f) for f in range(f0 + 1, f0 + 1 + N_TRACK)])).cuda()
        torch.cuda.synchronize()
        gv.process_device(dl.data_ptr(), None, N_TRACK, WP * HP)
        gv.synchronize()
    else:
        model = _Model(gv, SEEDS_MONO, [0, f0])
        _rows_equal(res["first_rows"], model.rows, "creation")
        assert res["first_info"][:5] == [4, len(model.rows["h"]), len(model.rows["h"]), 0, 0]
        prev_pose, after_promotion, checked = gv.keyframe_poses()[-1], False, 0
        for f in range(f0 + 1, f0 + 1 + N_TRACK):
            model.pre_points = model.points
            gv.OnNewFrame(_imgp(f))
            pose = gv.poses[-1]
            if after_promotion:  # this frame's direct pose ran on the extended map
                X = oracle_lib.direct_pose(_pyrp(f - 1), _pyrp(f), WP, HP, model.K, model.points, prev_pose, prev_pose)
                assert np.allclose(pose, X, rtol=1e-9, atol=1e-12), f
                checked += 1
            pr = model.frame(gv, f, pose, False)
            _rows_equal(gv.depth_seed_rows(), model.rows, f"frame {f}")
            after_promotion = pr is not None and pr["counts"][1] > 0
            prev_pose = pose
        res.update(model=model, checked=checked)
    res.update(rows=gv.depth_seed_rows(), points=gv.GetPoints(), poses=gv.poses, info=gv.depth_seeds().tolist(),
               hosts=gv.point_hosts(), launches=gv.ctx.timing("seeds")[0])
    gv.close()
    _pipe[mode] = res
    return res


@pytest.mark.gpu
def test_gpu_pipeline_matches_restatement():
    res = _pipeline("host")
    m = res["model"]
    for e in m.events:
        print("frame %2d seeds %4d promoted %3d retired %d inserted %d map %4d" % e)
    # (the map of the initialisation covers most cells already; the seeds sit on the latest keyframe)
    assert len(res["first_rows"]["h"]) >= 10 and (res["first_rows"]["h"] == 1).all()
    assert m.promoted > 0 and res["checked"] > 0
    st = m.rows["cnt"][:, 3]
    seen = (st != 0) | (m.rows["cnt"][:, 0] > 0)
    assert res["info"] == [4, len(st), m.created, m.promoted, m.dropped, int((seen & (st == 0)).sum()),
                           int((st >= 7).sum()), int(((st >= 1) & (st <= 6)).sum())]
    # one creation, an update per tracking frame, a promotion every 4th
    assert res["launches"] == 1 + N_TRACK + N_TRACK // 4


@pytest.mark.gpu
def test_gpu_device_chunk_equals_frame_by_frame():
    host, chunk = _pipeline("host"), _pipeline("chunk")
    assert np.array_equal(host["poses"], chunk["poses"]) and np.array_equal(host["points"], chunk["points"])
    assert np.array_equal(host["hosts"], chunk["hosts"]) and host["info"] == chunk["info"]
    for k in host["rows"]:
        assert np.array_equal(host["rows"][k], chunk["rows"][k]), k


@pytest.mark.gpu
def test_gpu_tolerance_mode_pipeline_rows():
    gv = _gv(SEEDS, fast=True)
    f0 = _start(gv)
    model = _Model(gv, SEEDS, [f0])
    for f in range(1, 9):
        model.pre_points = model.points
        gv.OnNewFrame(_imgp(f))
        model.frame(gv, f, gv.poses[-1], False)
        _rows_equal(gv.depth_seed_rows(), model.rows, f"fast frame {f}")
    gv.close()


@pytest.mark.gpu
def test_gpu_off_is_off():
    from viso_amd import _lib
    runs = []
    for how in ("never", "setter 0", "on and off"):
        gv = _gv()
        cfg = gv.config()
        gv.ctx.timing_enable(True)
        if how == "setter 0":
            gv.set_depth_seeds(0)
        elif how == "on and off":
            gv.set_depth_seeds(**SEEDS)
            gv.set_depth_seeds(0)
        assert gv.config() == cfg
        _start(gv)
        rows, stats = [], []
        for f in range(1, 9):
            gv.OnNewFrame(_imgp(f))
            rows.append(gv.alignment())
            stats.append(gv.stats())
        n = ctypes.c_size_t(0)
        assert _lib.load().viso_get_depth_seed_rows(gv.ctx.h, None, None, None, None, None, 0, ctypes.byref(n)) == -4
        assert gv.ctx.timing("seeds")[0] == 0 and gv.depth_seeds().tolist() == [0] * 8
        runs.append((gv.poses, gv.GetPoints(), rows, stats))
        gv.close()
    for other in runs[1:]:
        assert np.array_equal(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1])
        for ra, rb in zip(runs[0][2], other[2]):
            for a, b in zip(ra, rb):
                assert np.array_equal(a, b)
        for a, b in zip(runs[0][3], other[3]):
            assert np.array_equal(a, b, equal_nan=True)
    # switched on while tracking, the poses stay those of the plain run until a promotion extends the map
    gv = _gv()
    _start(gv)
    for f in range(1, 4):
        gv.OnNewFrame(_imgp(f))
    gv.set_depth_seeds(**SEEDS)
    assert gv.depth_seeds().tolist()[:3] == [4, 0, 0]  # (no keyframe has been created since)
    gv.OnNewFrame(_imgp(4))
    assert np.array_equal(gv.poses, runs[0][0][:4])
    gv.close()


@pytest.mark.gpu
def test_gpu_setter_arguments():
    from viso_amd import _lib
    gv = _gv()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(interval=-1), dict(cell=7), dict(cell=65), dict(max_steps=7), dict(max_steps=65),
                dict(depth_min=0.0), dict(depth_min=60.0), dict(depth_max=inf), dict(depth_min=nan),
                dict(max_score=0.0), dict(max_score=inf), dict(uniqueness=0.99), dict(uniqueness=nan),
                dict(min_good=0), dict(min_good=1001), dict(conv_rel=0.0), dict(conv_rel=1.01), dict(conv_rel=nan),
                dict(max_bad=0), dict(max_bad=1001), dict(max_lost=0), dict(max_lost=1001)):
        with pytest.raises(_lib.VisoError) as e:
            gv.set_depth_seeds(**dict(SEEDS, **bad))
        assert e.value.rc == -1, bad
    assert gv.depth_seeds().tolist() == [0] * 8
    gv.set_depth_seeds(**SEEDS)
    assert gv.depth_seeds().tolist() == [4, 0, 0, 0, 0, 0, 0, 0]
    assert len(gv.depth_seed_rows()["h"]) == 0
    lib = _lib.load()
    assert lib.viso_set_depth_seeds(None, 4, 16, 32, 2.0, 60.0, 100.0, 1.5, 3, 0.1, 4, 4) == -1
    assert lib.viso_get_depth_seeds(gv.ctx.h, None) == -1 and lib.viso_get_depth_seeds(None, None) == -1
    assert lib.viso_get_depth_seed_rows(None, None, None, None, None, None, 0, None) == -1
    for name in ("viso_set_depth_seeds", "viso_get_depth_seeds", "viso_get_depth_seed_rows"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    gv.close()


@pytest.mark.gpu
def test_gpu_composes_with_insertion_window_cull_refinements_and_warp():
    """Monocular insertion every 5th frame, a window of 2 keyframes, the cull
    every 4th frame, pose and point refinement and the warp all on, seeds
    promoted every 3rd frame, over 20 tracking frames.  Every frame's seed rows
    equal the restatement fed the GPU's pose, keyframe poses and map; a
    promotion's points are compared where nothing else reshuffled the map in
    the same frame; a retirement drops exactly the retired keyframe's seeds."""
    # (patient with failing seeds, so that keyframe 0 still hosts some when it retires)
    seeds = dict(SEEDS, interval=3, cell=8, max_bad=20, max_lost=20)
    gv = _gv(seeds, cull=(4, 3, 2.0, 50), refine=(5, 1.0, 8.0), prefine=(5, 5, 3, 1.0, 8.0, 3, 0.05),
             mono=(5, 1000, 8, 0.1), window=(2, 16), warp=64.0)
    f0 = _start(gv)
    model = _Model(gv, seeds, [f0])
    _rows_equal(gv.depth_seed_rows(), model.rows, "creation")
    checked = 0
    for f in range(1, 21):
        b_cull, b_win = gv.point_cull()[2], gv.map_window()[2]
        model.pre_points = model.points
        gv.OnNewFrame(_imgp(f))
        retired = gv.map_window()[2] > b_win
        culled = gv.point_cull()[2] > b_cull
        n_kf = len(gv.keyframe_poses())
        # (nothing else touched the map: no cull, retirement, insertion or point refinement in this frame)
        quiet = not (retired or culled) and n_kf == len(model.kf_poses) and f % 5 != 0
        pr = model.frame(gv, f, gv.poses[-1], retired, check_points=quiet)
        _rows_equal(gv.depth_seed_rows(), model.rows, f"frame {f}")
        checked += bool(quiet and pr is not None and pr["counts"][1])
        assert (model.rows["h"] >= 0).all() and (model.rows["h"] < n_kf).all()
    info = gv.depth_seeds().tolist()
    poses = gv.poses
    gv.close()
    for e in model.events:
        print("frame %2d seeds %4d promoted %3d retired %d inserted %d map %4d" % e)
    assert len(poses) == 20 and np.isfinite(poses).all()
    assert info[1:5] == [len(model.rows["h"]), model.created, model.promoted, model.dropped]
    assert any(e[3] for e in model.events) and any(e[4] for e in model.events) and model.promoted > 0
    print("promotions compared point by point", checked, "; seeds that left with their keyframe", model.retired_seeds)
    assert checked > 0 and model.retired_seeds > 0


@pytest.mark.gpu
def test_gpu_zz_depth_seeds_report():
    print("bit-equal to the restatement over the GPU tests that ran:", BITS)
    print("largest relative difference:", WORST)
    assert all(v <= 1e-9 for v in WORST.values())
