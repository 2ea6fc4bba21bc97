"""Illumination-invariant LK alignment (viso_set_lk_illum): a
per-patch gain and offset projected out of the warped alignment.

The rule is the project's own; its restatement is tests/lk_illum_ref.py, over
the helpers of tests/lk_warp_ref.py.  CPU tests check the restatement's
algebra against plain loops and numpy's least squares, its invariance to an
exact affine brightness change, that it does what it is for on a rendered
plane, its guards, and the decision margins of the GPU parity cases.  GPU
tests compare the stage entry, the batched launch and the frame path against
the restatement, that off is off, and what the mode does to a run with the
consumers of the LK rows on.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import lk_illum_ref as il
from tests import lk_warp_ref as lk
from tests import oracle_lib
from tests import test_lk_warp as tw

IDENT = tw.IDENT
MEASURED = {}


def _mapped(img, g, o, exact=False):
    """g img + o as bytes (rounded, clipped); exact: asserts that the bytes
    are exact and none clips."""
    v = img.astype(np.float64) * g + o
    if exact:
        assert np.array_equal(v, np.rint(v)) and v.min() > 0 and v.max() < 255, (g, o, v.min(), v.max())
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ 1. algebra
# 3 x the values measured (printed by the test)
ORTHO_BAR = 3 * 3.32e-15   # | sum P |, | sum P Tc | over sum | P |, sum | P Tc |
COST_BAR = 3 * 8.15e-15    # the cost by subtraction against the explicitly projected residual's energy
LSTSQ_BAR = 3 * 2.44e-14   # gain, offset against numpy.linalg.lstsq, over max(|gain|, 1) and max(|offset|, 1)


@functools.lru_cache(maxsize=None)
def _patches():
    """Level-0 templates, Jacobians and current samples (1.5 px off, the
    current image 0.8 I + 30) of the plane scene's 150 points."""
    plane, kp, P = tw._plane4()
    true = tw.MOTIONS["roll 0.3"]
    cur = _mapped(plane.render(true), 0.8, 30.0)
    kl, ws, hs = lk.levels(kp, tw.W4, tw.H4)
    lane = np.arange(64)
    px, py = ((lane >> 3) - 4).astype(np.float64)[None, :], ((lane & 7) - 4).astype(np.float64)[None, :]
    uv = tw._project(IDENT, tw.K2, P)
    x, y = uv[:, :1] + px, uv[:, 1:] + py
    s = lambda X, Y: lk.sample(kl[0], ws[0], hs[0], X, Y)
    T, J0, J1 = s(x, y), -0.5 * (s(x + 1, y) - s(x - 1, y)), -0.5 * (s(x, y + 1) - s(x, y - 1))
    uc = tw._project(true, tw.K2, P) + [1.2, 0.9]
    smp = lk.sample(cur.reshape(-1), tw.W4, tw.H4, uc[:, :1] + px, uc[:, 1:] + py)
    return T, J0, J1, smp


def test_projected_jacobian_is_orthogonal_to_one_and_the_template():
    T, J0, J1, _ = _patches()
    m, Tc, stt, P0, P1 = il.project_out(T, J0, J1)
    assert (stt >= il.STT_MIN).all()
    worst = 0.0
    for P in (P0, P1):
        worst = max(worst, np.max(np.abs(P.sum(1)) / np.abs(P).sum(1)))
        worst = max(worst, np.max(np.abs((P * Tc).sum(1)) / np.abs(P * Tc).sum(1)))
    MEASURED["ortho"] = worst
    print(f"largest relative | sum P |, | sum P Tc |: {worst:.3g} (bar {ORTHO_BAR:.3g})")
    assert worst <= ORTHO_BAR


def test_cost_is_the_projected_residuals_energy():
    T, J0, J1, smp = _patches()
    m, Tc, stt, P0, P1 = il.project_out(T, J0, J1)
    *_, cost = il.iteration_sums(T, Tc, P0, P1, stt, smp)
    worst = 0.0
    for i in range(T.shape[0]):  # a plain double loop: e with its mean and its part along Tc removed
        e = [T[i, p] - smp[i, p] for p in range(64)]
        mean = sum(e) / 64
        tc = [T[i, p] - sum(T[i]) / 64 for p in range(64)]
        along = sum(tc[p] * e[p] for p in range(64)) / sum(t * t for t in tc)
        energy = sum((e[p] - mean - along * tc[p]) ** 2 for p in range(64))
        worst = max(worst, abs(cost[i] - energy) / energy)
    MEASURED["cost"] = worst
    print(f"largest relative | cost - explicit energy |: {worst:.3g} (bar {COST_BAR:.3g})")
    assert worst <= COST_BAR


def test_gain_and_offset_are_the_least_squares_fit():
    T, J0, J1, smp = _patches()
    m, Tc, stt, P0, P1 = il.project_out(T, J0, J1)
    _, _, _, se, ste, _ = il.iteration_sums(T, Tc, P0, P1, stt, smp)
    gain, offset = il.gain_offset(m, stt, se, ste)
    worst = 0.0
    for i in range(T.shape[0]):
        (g, o), *_ = np.linalg.lstsq(np.stack([T[i], np.ones(64)], 1), smp[i], rcond=None)
        worst = max(worst, abs(gain[i] - g) / max(abs(g), 1.0), abs(offset[i] - o) / max(abs(o), 1.0))
    MEASURED["lstsq"] = worst
    print(f"largest | gain, offset - lstsq |: {worst:.3g} (bar {LSTSQ_BAR:.3g}); median gain "
          f"{np.median(gain):.3f}, offset {np.median(offset):.1f}")
    assert worst <= LSTSQ_BAR


def test_mode_off_is_the_warped_restatement():
    kp, cp, P = tw._pin_scene()
    a = il.lk_align_illum([kp], [IDENT], cp, IDENT, tw.W1, tw.H1, tw.K1, P, mode=0)
    b = lk.lk_align_warped([kp], [IDENT], cp, IDENT, tw.W1, tw.H1, tw.K1, P)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in b)


# ------------------------------------------------------------------ 2. invariance
# 3 x the values measured (printed by the test).  Level 0 is
# exactly affine; levels 1-3 are not after pyrDown's rounding, so the
# positions level 0 starts from differ and the bounds are not at rounding level.
INV_UV_BAR = 3 * 2.14e-7         # px
INV_GAIN_BAR = 3 * 6.64e-8       # gain against g, relative
INV_OFFSET_BAR = 3 * 4.68e-6       # offset against o, grey levels
INV_GO = ((0.75, 30.0), (0.5, 100.0))


@functools.lru_cache(maxsize=None)
def _pin4():
    """test_lk_warp's pin scene on bytes that are multiples of 4."""
    plane = tw.Plane(tw.K1, tw.W1, tw.H1, seed=3)
    key = plane.render(IDENT) & np.uint8(0xFC)
    cur = np.roll(np.roll(key, 1, axis=0), 2, axis=1)
    _, _, P = tw._pin_scene()
    return key, cur, P


def _pin_run(cur, **kw):
    key, _, P = _pin4()
    return il.lk_align_illum([oracle_lib.pyramid(key)], [IDENT], oracle_lib.pyramid(cur), IDENT, tw.W1, tw.H1, tw.K1,
                             P, **kw)


@pytest.mark.parametrize("go", INV_GO)
def test_exact_affine_brightness_changes_nothing(go):
    g, o = go
    key, cur, P = _pin4()
    base = _pin_run(cur)
    r = _pin_run(_mapped(cur, g, o, exact=True))
    assert base["success"].mean() > 0.9
    for k in ("pair_kf", "success", "status", "shift"):
        assert np.array_equal(r[k], base[k]), k
    ok = base["success"] == 1
    duv = np.abs(r["uv_after"] - base["uv_after"]).max()
    dg = np.abs(r["gain_offset"][ok, 0] / g - 1).max()
    do = np.abs(r["gain_offset"][ok, 1] - o).max()
    bg = np.abs(base["gain_offset"][ok] - [1.0, 0.0]).max(0)
    MEASURED[go] = (duv, dg, do)
    print(f"g {g} o {o}: largest | uv_after - unmodified | {duv:.3g} px, | gain / g - 1 | {dg:.3g}, | offset - o | "
          f"{do:.3g}; unmodified pair's | gain - 1 | {bg[0]:.3g}, | offset | {bg[1]:.3g}")
    assert duv <= INV_UV_BAR and dg <= INV_GAIN_BAR and do <= INV_OFFSET_BAR


# ------------------------------------------------------------------ 3. it does what it is for
CASES3 = [(m, go) for m in ("zoom 1.3", "roll 0.3") for go in ((1.0, 0.0), (0.8, 30.0), (0.5, 20.0))]
TABLE3 = {}


@pytest.mark.parametrize("motion,go", CASES3)
def test_mode_aligns_what_a_brightness_change_loses(motion, go):
    g, o = go
    plane, kp, P = tw._plane4()
    true = tw.MOTIONS[motion]
    cp = oracle_lib.pyramid(_mapped(plane.render(true), g, o))
    depth = lk.transform(true, (P[:, 0], P[:, 1], P[:, 2]))[2].mean()
    off = true.copy()
    off[9] += 1.2 * depth / tw.K2[0]
    off[10] += 0.9 * depth / tw.K2[1]
    truth = tw._project(true, tw.K2, P)
    r = il.lk_align_illum([kp], [IDENT], cp, off, tw.W4, tw.H4, tw.K2, P)
    w = lk.lk_align_warped([kp], [IDENT], cp, off, tw.W4, tw.H4, tw.K2, P)
    ei = np.linalg.norm(r["uv_after"] - truth, axis=1)
    ew = np.linalg.norm(w["uv_after"] - truth, axis=1)
    share = np.mean((r["success"] == 1) & (ei < 0.5))
    wshare = np.mean((w["success"] == 1) & (ew < 0.5))
    mg, mo = np.nanmedian(r["gain_offset"], 0)
    TABLE3[(motion, go)] = (r["success"].mean(), share, np.median(ei), w["success"].mean(), wshare, np.median(ew))
    print(f"{motion}, g {g}, o {o}: mode {r['success'].mean():.0%} / {share:.0%} / {np.median(ei):.3f} px; plain "
          f"{w['success'].mean():.0%} / {wshare:.0%} / {np.median(ew):.3f} px; ratio "
          f"{np.median(ew) / np.median(ei):.1f}; median gain {mg:.3f}, offset {mo:.1f}")
    assert share >= 0.95
    assert np.median(ei) <= 0.25
    if go != (1.0, 0.0):
        assert np.median(ew) >= 4 * np.median(ei)


# ------------------------------------------------------------------ 4. guards
def test_flat_current_image_is_refused_by_the_gain_bound():
    key, cur, P = _pin4()
    r = _pin_run(np.full_like(cur, 90))
    through = (r["status"] & 15) != 1
    assert through.all() and ((r["status"] & 15) != 2).all()
    went = (r["status"] >> 4) == 0
    assert went.sum() > 100
    assert ((r["status"][went] & 15) == 3).all() and not r["success"].any()
    assert (np.abs(r["gain_offset"][went, 0]) < 1e-9).all()
    print("flat current image: largest | gain |", np.abs(r["gain_offset"][went, 0]).max())


def test_flat_keyframe_skips_every_level():
    key, cur, P = _pin4()
    r = il.lk_align_illum([oracle_lib.pyramid(np.full_like(key, 90))], [IDENT], oracle_lib.pyramid(cur), IDENT,
                          tw.W1, tw.H1, tw.K1, P)
    assert (r["status"] == (4 << 4)).all() and not r["success"].any()
    assert np.array_equal(r["uv_after"], r["uv_before"]) and np.isfinite(r["uv_after"]).all()
    assert np.isnan(r["gain_offset"]).all()


def _gain_scene(g):
    """A keyframe in multiples of 4 (g = 1.75: scaled into 4..144) and the
    current image g times it, exactly, not moved: every point's gain is close
    to g.  (The rule's step is the unit-gain one, so its iterations contract
    by | 1 - g |: g stays below 2.)"""
    key, _, P = _pin4()
    if g > 1:
        key = np.clip((key.astype(np.int32) * 9 // 16) & 0xFC, 4, 144).astype(np.uint8)
    else:
        key = np.clip(key, 4, 252)
    return key, _mapped(key, g, 0.0, exact=True), P[:8]


def _gain_run(key, cur, P, max_gain):
    return il.lk_align_illum([oracle_lib.pyramid(key)], [IDENT], oracle_lib.pyramid(cur), IDENT, tw.W1, tw.H1, tw.K1,
                             P, max_gain=max_gain)


def test_max_gain_thresholds():
    # the upper bound: ghi = max_gain, stepped to both sides of a point's own gain
    key, cur, P = _gain_scene(1.75)
    r = _gain_run(key, cur, P, 4.0)
    print("gains at g = 1.75:", r["gain_offset"][:, 0])
    assert r["success"].all() and np.abs(r["gain_offset"][:, 0] - 1.75).max() < 0.05
    for i in range(len(P)):
        gi = r["gain_offset"][i, 0]
        for mgain, ok in ((gi, 1), (np.nextafter(gi, np.inf), 1), (np.nextafter(gi, -np.inf), 0)):
            q = _gain_run(key, cur, P[i:i + 1], mgain)
            assert q["success"][0] == ok and (q["status"][0] & 15) == (0 if ok else 3), (i, mgain)
            assert np.array_equal(q["gain_offset"][0], r["gain_offset"][i])
            assert np.array_equal(q["uv_after"][0], r["uv_after"][i])
    # the lower bound: glo = 1 / max_gain, max_gain stepped through the values around 1 / gain
    key, cur, P = _gain_scene(0.5)
    r = _gain_run(key, cur, P, 4.0)
    print("gains at g = 0.5:", r["gain_offset"][:, 0])
    assert r["success"].all() and np.abs(r["gain_offset"][:, 0] - 0.5).max() < 0.0125
    seen = set()
    for i in range(len(P)):
        gi = r["gain_offset"][i, 0]
        mgain = 1.0 / gi
        for _ in range(3):
            mgain = np.nextafter(mgain, -np.inf)
        for _ in range(7):
            ok = int(1.0 / mgain <= gi)
            q = _gain_run(key, cur, P[i:i + 1], mgain)
            assert q["success"][0] == ok and (q["status"][0] & 15) == (0 if ok else 3), (i, mgain)
            seen.add(ok)
            mgain = np.nextafter(mgain, np.inf)
    assert seen == {0, 1}


# ------------------------------------------------------------------ 5. the GPU parity cases
W, H, K6, RATIO, SIZES = tw.W, tw.H, tw.K6, tw.RATIO, tw.SIZES
KF_POSES, CUR_POSES = tw.KF_POSES, tw.CUR_POSES
GO6 = ((0.75, 30.0), (1.0, 20.0), (0.5, 60.0), (1.25, -40.0))  # the current images' mappings
# gains spread around 0.5 under the third mapping: both sides of glo = 1 / 2
MAX_GAIN6 = 2.0
FLAT6 = (slice(40, 100), slice(150, 230))  # a flat region (rows, columns) of keyframes 0 and 1
FLAG_BAR = 1e-9
DROPPED = {}


@functools.lru_cache(maxsize=None)
def _scene6():
    plane, _, _ = tw._scene6()
    kfs = []
    for j, p in enumerate(KF_POSES):
        img = plane.render(p).copy()
        if j < 2:
            img[FLAT6] = 128
        kfs.append(oracle_lib.pyramid(img))
    curs = [oracle_lib.pyramid(_mapped(plane.render(p), g, o)) for p, (g, o) in zip(CUR_POSES, GO6)]
    for a in kfs + curs:
        a.setflags(write=False)
    return kfs, curs


def _restate6(c, P, margins=None, mode=1):
    kfs, curs = _scene6()
    return il.lk_align_illum(kfs, KF_POSES, curs[c], CUR_POSES[c], W, H, K6, P, max_area_ratio=RATIO, mode=mode,
                             max_gain=MAX_GAIN6, margins=margins)


@functools.lru_cache(maxsize=None)
def _case6(n, seed=0):
    """The n points of a parity case: the first n of its seeded stream of
    candidates (test_lk_warp's generator) none of whose flag-changing
    decisions, in the restatement alone, is within FLAG_BAR (relative).  The
    stream is not thinned on the `cost > lastCost` margin: the points that tie
    there are the converged ones, and a flipped stop moves them by far less
    than the comparison allows."""
    c = tw._cur_of(n)
    rng = np.random.default_rng(7000 * seed + n)
    kept, drawn, ties = np.zeros((0, 3)), 0, 0
    while len(kept) < n:
        P = tw._candidates(rng, n - len(kept) + 8)
        mg = {}
        _restate6(c, P, mg)
        clear = mg["flag_margin"] > FLAG_BAR
        used = int(min(len(P), np.searchsorted(np.cumsum(clear), n - len(kept)) + 1))
        drawn += used
        ties += int((mg["cost_ties"][:used] > 0).sum())
        kept = np.concatenate([kept, P[clear]])[:n]
    DROPPED[n] = (drawn, drawn - n, ties)
    return kept


@functools.lru_cache(maxsize=None)
def _expect6(n):
    return _restate6(tw._cur_of(n), _case6(n))


def test_parity_cases_cover_every_path_and_leave_out_few():
    status, shifts = set(), set()
    taps = flat = failed = 0
    for n in SIZES:
        r = _expect6(n)
        drawn, out, ties = DROPPED[n]
        assert out <= 0.01 * drawn, (n, DROPPED[n])
        if n == 0:
            continue
        plain = _restate6(tw._cur_of(n), _case6(n), mode=0)
        through = np.isin(r["status"] & 15, (0, 3))
        assert np.array_equal(through, (plain["status"] & 15) == 0)
        status |= set((r["status"] & 15).tolist())
        shifts |= set(r["shift"][through].tolist())
        taps += int((plain["status"][through] >> 4).sum())
        flat += int(((r["status"][through] >> 4) - (plain["status"][through] >> 4)).sum())
        failed += int(((r["status"] == 0) & (r["success"] == 0)).sum())
    print("per case: candidates drawn, left out for a flag margin, with a tied cost comparison", DROPPED)
    print(f"skipped levels: {taps} by their taps, {flat} flat; failed alignments {failed}")
    assert status == {0, 1, 2, 3}
    assert {-2, -1, 0, 1} <= shifts
    assert taps > 0 and flat > 0 and failed > 0
    r = _expect6(2049)
    assert r["success"].sum() > 200 and np.isnan(r["gain_offset"][:, 0]).sum() > 0
    assert ((r["status"] & 15) == 3).sum() > 0


# ------------------------------------------------------------------ GPU: the stage entry (6)
@functools.lru_cache(maxsize=None)
def _ctx(fast=False):
    from viso_amd import api
    fx, fy, cx, cy = K6
    kw = {"precision": 1} if fast else {}
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=W, height=H, **kw))


BITS = {"uv_after": True, "gain_offset": True}


def _check_rows(got, exp, where="", a_rtol=1e-12, a_atol=0.0):
    """got: (pair_kf, success, uv_before, uv_after, A, shift, status, gain_offset)."""
    pk, sc, ub, ua, A, sh, st, go = got
    assert np.array_equal(pk, exp["pair_kf"]), where
    assert np.array_equal(st, exp["status"]), where
    assert np.array_equal(sh, exp["shift"]), where
    assert np.array_equal(sc, exp["success"]), where
    assert np.allclose(A, exp["A"], rtol=a_rtol, atol=a_atol, equal_nan=True), where
    assert np.array_equal(ub, exp["uv_before"]), where
    assert np.array_equal(np.isnan(go), np.isnan(exp["gain_offset"])), where
    if len(pk):
        assert np.abs(ua - exp["uv_after"]).max() < 1e-6, where
        assert np.allclose(go, exp["gain_offset"], rtol=1e-9, atol=0.0, equal_nan=True), where
    BITS["uv_after"] &= np.array_equal(ua, exp["uv_after"])
    BITS["gain_offset"] &= np.array_equal(go, exp["gain_offset"], equal_nan=True)


def _stage(n, fast=False, **kw):
    kfs, curs = _scene6()
    c = tw._cur_of(n)
    return _ctx(fast).lk_align_illum(kfs, KF_POSES, curs[c], CUR_POSES[c], W, H, _case6(n), RATIO, MAX_GAIN6, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gpu_stage_entry_matches_restatement(n):
    exp = _expect6(n)
    got = _stage(n)
    _check_rows(got, exp, f"n = {n}")
    print(f"n = {n}: bit-equal uv_after {np.array_equal(got[3], exp['uv_after'])}, gain_offset "
          f"{np.array_equal(got[7], exp['gain_offset'], equal_nan=True)}; status counts "
          f"{np.bincount(exp['status'] & 15, minlength=4).tolist()}")


@pytest.mark.gpu
def test_gpu_stage_entry_arguments_and_optional_outputs():
    from viso_amd import _lib
    kfs, curs = _scene6()
    P = _case6(5)
    ctx = _ctx()
    for bad in (1.499, 16.001, 0.0, -4.0, float("nan"), float("inf")):
        with pytest.raises(_lib.VisoError) as e:
            ctx.lk_align_illum(kfs, KF_POSES, curs[0], CUR_POSES[0], W, H, P, RATIO, bad)
        assert e.value.rc == -1
    for bad in (3.999, 64.001, float("nan")):
        with pytest.raises(_lib.VisoError) as e:
            ctx.lk_align_illum(kfs, KF_POSES, curs[0], CUR_POSES[0], W, H, P, bad, 4.0)
        assert e.value.rc == -1
    for mg in (1.5, 16.0):
        ctx.lk_align_illum(kfs, KF_POSES, curs[0], CUR_POSES[0], W, H, P, RATIO, mg)
    assert _lib.KERNEL_IDS["lkwarp"] == 13 and len(_lib.KERNEL_IDS) + len(_lib.CHAIN_KERNEL_IDS) == 20
    full = _stage(65)
    for kw in ({"warp_rows": False}, {"gain_rows": False}, {"warp_rows": False, "gain_rows": False}):
        part = _stage(65, **kw)
        for a, b in zip(part, full):
            assert a is None or np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
        assert (part[4] is None) == (not kw.get("warp_rows", True)) and (part[7] is None) == (not kw.get("gain_rows", True))


@pytest.mark.gpu
def test_gpu_tolerance_mode_gives_the_same_rows():
    for n in (65, 257):
        exact, fast = _stage(n), _stage(n, fast=True)
        _check_rows(fast, _expect6(n), f"fast, n = {n}")
        for a, b in zip(exact, fast):
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ------------------------------------------------------------------ GPU: the frame path (7-10)
N_PIPE = 11  # the stereo frame and 10 tracking frames
# frame k's (gain, offset) on bytes that are multiples of 4: exact, and inside 1..254 (asserted)
FRAME_GO = [None, (1.0, 10.0), (0.75, 30.0), (0.5, 100.0), (1.0, -3.0), (0.75, -2.0), (0.5, 0.0), (1.0, 15.0),
            (0.5, 130.0), (0.75, 12.0), (1.0, 0.0)]
MAX_GAIN = 4.0
BRIGHT_ITER = 10


@functools.lru_cache(maxsize=None)
def _frame(k):
    img = tw._image(k)
    if k > 0:
        img = _mapped(img & np.uint8(0xFC), *FRAME_GO[k], exact=True)
        img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _fpyr(k):
    p = oracle_lib.pyramid(_frame(k))
    p.setflags(write=False)
    return p


def _viso(illum=MAX_GAIN, warp=RATIO, bright=BRIGHT_ITER, **kw):
    import viso_amd
    seq = tw._seq()
    gv = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32, **kw)
    gv.set_stereo(seq.p.baseline, 128, 1)
    if bright:
        gv.set_brightness(bright)
    if warp:
        gv.set_lk_warp(1, warp)
    if illum:
        gv.set_lk_illum(1, illum)
    gv.process(_frame(0), tw._image(0, 1))
    assert gv.state == 1
    return gv


def _rows(gv):
    return tuple(gv.alignment()) + tuple(gv.lk_warp_rows()) + (gv.lk_illum_rows(),)


def _restate(kfp, f, pose, points, mode=1):
    return il.lk_align_illum([_fpyr(0)], kfp, _fpyr(f), pose, W, H, tw._seq().K, points, max_area_ratio=RATIO,
                             mode=mode, max_gain=MAX_GAIN)


def _chunk(gv, first, last):
    import torch
    dl = torch.from_numpy(np.stack([_frame(f) for f in range(first, last + 1)])).cuda()
    torch.cuda.synchronize()
    gv.process_device(dl.data_ptr(), None, last - first + 1, W * H)
    gv.synchronize()


_runs = {}


def _pipeline(mode):
    """mode: "host" (frame by frame) or "chunk" (one device chunk), both with
    the brightness chain, the warp and the mode on."""
    if mode not in _runs:
        gv = _viso()
        gv.ctx.timing_enable(True)
        points, kfp = gv.GetPoints(), gv.keyframe_poses()
        rows = {}
        if mode == "chunk":
            _chunk(gv, 1, N_PIPE - 1)
            rows[N_PIPE - 1] = _rows(gv)
        else:
            for f in range(1, N_PIPE):
                gv.OnNewFrame(_frame(f))
                rows[f] = _rows(gv)
        _runs[mode] = {"rows": rows, "poses": gv.poses, "points": gv.GetPoints(), "first_points": points,
                       "kf_poses": kfp, "launches": gv.ctx.timing("lkwarp")[0],
                       "lkalign": gv.ctx.timing("lkalign")[0], "info": gv.lk_illum(), "winfo": gv.lk_warp()}
        gv.close()
    return _runs[mode]


@pytest.mark.gpu
def test_gpu_batched_launch_equals_frame_by_frame():
    """A device chunk of 4 frames against the same frames one by one, without
    the brightness chain (with it every frame is finished behind its own
    chain, one launch each): one launch over 4 frames."""
    gv = _viso(bright=None)
    gv.ctx.timing_enable(True)
    pts, kfp = gv.GetPoints(), gv.keyframe_poses()
    _chunk(gv, 1, 4)
    got, poses = _rows(gv), gv.poses
    assert gv.ctx.timing("lkwarp")[0] == 1 and gv.lk_illum()[1] == 4
    gv.close()
    one = _viso(bright=None)
    for f in range(1, 5):
        one.OnNewFrame(_frame(f))
        _check_rows(_rows(one), _restate(kfp, f, one.poses[-1], pts), f"frame {f}")
    assert np.array_equal(poses, one.poses)
    for a, b in zip(got, _rows(one)):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    one.close()
    _check_rows(got, _restate(kfp, 4, poses[3], pts), "chunk of 4")


@pytest.mark.gpu
def test_gpu_pipeline_matches_restatement_on_host_frames_and_a_chunk():
    host, chunk = _pipeline("host"), _pipeline("chunk")
    pts, kfp = host["first_points"], host["kf_poses"]
    assert len(pts) > 50 and len(kfp) == 1 and np.array_equal(host["points"], pts)
    for f in range(1, N_PIPE):
        exp = _restate(kfp, f, host["poses"][f - 1], pts)
        _check_rows(host["rows"][f], exp, f"frame {f}")
        go = exp["gain_offset"][exp["success"] == 1]
        print(f"frame {f} (g, o) {FRAME_GO[f]}: aligned {int(exp['success'].sum())}, status 3 "
              f"{int(((exp['status'] & 15) == 3).sum())}, median gain {np.median(go[:, 0]):.3f}, offset "
              f"{np.median(go[:, 1]):.1f}")
    last = N_PIPE - 1
    info = [1, last, int((exp["pair_kf"] >= 0).sum()), int(exp["success"].sum()),
            int(((exp["status"] & 15) == 3).sum()), 0, 0, 0]
    assert list(host["info"]) == info and exp["success"].sum() > 20
    assert host["launches"] == last and host["lkalign"] == 0
    # the chunk: the same poses, map and last rows, bit for bit
    for k in ("poses", "points"):
        assert np.array_equal(host[k], chunk[k]), k
    for a, b in zip(host["rows"][last], chunk["rows"][last]):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    _check_rows(chunk["rows"][last], exp, "chunk")
    # (behind the brightness chain every frame of the chunk is finished on its own: one launch each)
    assert chunk["launches"] == last and chunk["lkalign"] == 0 and list(chunk["info"]) == info
    assert list(chunk["winfo"]) == list(host["winfo"])


@pytest.mark.gpu
def test_gpu_off_is_off():
    from viso_amd import _lib
    n = ctypes.c_size_t(0)
    getter = lambda gv: _lib.load().viso_get_lk_illum_rows(gv.ctx.h, None, 0, ctypes.byref(n))

    def run(warp, how):
        gv = _viso(illum=None, warp=warp)
        cfg = gv.config()
        gv.ctx.timing_enable(True)
        if how == "zero":
            gv.set_lk_illum(0)
        if how == "one":  # (only with the warp off: kept, inert)
            gv.set_lk_illum(1, MAX_GAIN)
        assert gv.config() == cfg
        rows = []
        for f in range(1, 6):
            gv.OnNewFrame(_frame(f))
            rows.append(tuple(gv.alignment()) + (tuple(gv.lk_warp_rows()) if warp else ()))
            assert getter(gv) == -4
        assert list(gv.lk_illum()) == [0] * 8
        return gv, rows, cfg

    for warp, hows in ((None, ("never", "zero", "one")), (RATIO, ("never", "zero"))):
        runs = [run(warp, how) for how in hows]
        for gv, rows, cfg in runs[1:]:
            assert cfg == runs[0][2]
            assert np.array_equal(gv.poses, runs[0][0].poses) and np.array_equal(gv.GetPoints(), runs[0][0].GetPoints())
            for ra, rb in zip(rows, runs[0][1]):
                for a, b in zip(ra, rb):
                    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
            assert gv.ctx.timing("lkwarp")[0] == runs[0][0].ctx.timing("lkwarp")[0]
            assert gv.ctx.timing("lkalign")[0] == runs[0][0].ctx.timing("lkalign")[0]
        if warp is None:
            # the kept mode comes into force with the warp, while tracking
            kept = runs[2][0]
            kept.set_lk_warp(1, RATIO)
            kept.OnNewFrame(_frame(6))
            assert getter(kept) == 0 and kept.lk_illum()[1] == 1
            _check_rows(_rows(kept), _restate(kept.keyframe_poses(), 6, kept.poses[-1], kept.GetPoints()), "kept")
            kept.set_lk_warp(0)
            assert getter(kept) == -4 and list(kept.lk_illum()) == [0] * 8
        else:
            # switched on at frame 6, off at 8, on again at 9
            never, gv = runs[0][0], runs[1][0]
            for f in range(6, 11):
                if f in (6, 9):
                    gv.set_lk_illum(1, MAX_GAIN)
                if f == 8:
                    gv.set_lk_illum(0)
                never.OnNewFrame(_frame(f))
                gv.OnNewFrame(_frame(f))
                a, b = never.alignment(), gv.alignment()
                on = f != 8
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
                assert np.array_equal(a[3], b[3]) == (not on), f
                exp = _restate(gv.keyframe_poses(), f, gv.poses[-1], gv.GetPoints(), mode=1 if on else 0)
                if on:
                    _check_rows(_rows(gv), exp, f"frame {f}")
                else:
                    assert getter(gv) == -4
                    tw._check_rows(tuple(b) + tuple(gv.lk_warp_rows()), exp, f"frame {f}")
            assert np.array_equal(never.poses, gv.poses)
            for bad in ((2, 4.0), (-1, 4.0), (1, 1.4), (1, 16.5), (1, float("nan")), (1, float("inf"))):
                with pytest.raises(_lib.VisoError) as e:
                    gv.set_lk_illum(*bad)
                assert e.value.rc == -1
        for gv, _, _ in runs:
            gv.close()


@pytest.mark.gpu
def test_gpu_mode_keeps_the_consumers_fed_through_exposure_changes():
    """Cull, pose refinement and point refinement on, over the exposed
    sequence, once with the mode and once without.  Over the frames whose
    exposure differs much from the keyframe's (| o | >= 10 or g <= 0.75) the
    mode aligns more points, and its aligned points lie closer, in median, to
    their projections (uv_before); the map after the last frame is at least
    as large.  No ratio is fixed in advance; the counts go into DESIGN.md §24."""
    from tests import test_point_refine as tpr
    hard = [f for f in range(1, N_PIPE) if abs(FRAME_GO[f][1]) >= 10 or FRAME_GO[f][0] <= 0.75]
    out = {}
    for mode in (1, 0):
        gv = tpr._viso(cull=(4, 3, 2.0, 50), refine=(5, 1.0, 8.0))
        gv.set_brightness(BRIGHT_ITER)
        gv.set_lk_warp(1, RATIO)
        if mode:
            gv.set_lk_illum(1, MAX_GAIN)
        per = []
        for f in range(1, N_PIPE):
            gv.OnNewFrame(_frame(f))
            pk, sc, ub, ua = gv.alignment()
            d = np.linalg.norm(ua - ub, axis=1)[sc == 1]
            per.append((f, int((pk >= 0).sum()), int(sc.sum()), d, len(gv.GetPoints())))
        assert np.isfinite(gv.poses).all() and len(gv.poses) == N_PIPE - 1
        assert gv.lk_illum()[1] == (N_PIPE - 1 if mode else 0)
        out[mode] = per
        gv.close()
    for mode in (1, 0):
        for f, paired, aligned, d, nmap in out[mode]:
            print(f"mode {mode} frame {f:2d} (g, o) {FRAME_GO[f]}: paired {paired:4d} aligned {aligned:4d} median "
                  f"| uv_after - uv_before | {np.median(d) if len(d) else float('nan'):.3f} px, map {nmap}")
    aligned = {m: sum(p[2] for p in out[m] if p[0] in hard) for m in out}
    dist = {m: float(np.median(np.concatenate([p[3] for p in out[m] if p[0] in hard]))) for m in out}
    print("over frames", hard, "aligned", aligned, "median distance", dist, "last map", out[1][-1][4], out[0][-1][4])
    assert aligned[1] > aligned[0]
    assert dist[1] < dist[0]
    assert out[1][-1][4] >= out[0][-1][4]


@pytest.mark.gpu
def test_gpu_zz_bit_equality_report():
    """Not a bar (the bars are in _check_rows): whether every GPU row of this
    run was bit-equal to the restatement, for DESIGN.md §24."""
    print("bit-equal to the restatement over this run:", BITS)
