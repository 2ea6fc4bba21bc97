"""The crafted stereo VO stage cases (tests/svo_cases.py) on the CPU: a brute
force restatement of circular matching pins the spec's row index and tie rule
(oracle/oracle_svo.cpp), a census proves that every case reaches the edge it
is named for *through an accepted match*, the motion cases populate the
spec's exits (oracle_svo_estimate_trace), and viso_svo_create's parameter
bounds are checked (they are refused before a device is touched).  The GPU
side of the same cases is tests/test_svo_stages.py."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import svo_cases as sc

MATCH_CASES = sc.match_cases()
MOTION_CASES = sc.motion_cases()


def match_params(case):
    return ol.svo_params(case.w, case.h, *sc.K, **case.kw)


# ------------------------------------------------------------------ brute-force circular matching
class Step:
    """One of the four searches of a circle, restated without any index: every
    feature of the target set is looked at."""

    def __init__(self, S, u, v, c, d, du_lo, du_hi, dv):
        self.S, self.u, self.v, self.c, self.du_lo, self.du_hi, self.dv = S, int(u), int(v), int(c), du_lo, du_hi, dv
        dd = self.u - S.u.astype(np.int64)
        m = (S.cls == c) & (S.v >= self.v - dv) & (S.v <= self.v + dv) & (dd >= du_lo) & (dd <= du_hi)
        self.idx = np.nonzero(m)[0]
        self.sad = np.abs(S.desc[self.idx].astype(np.int64) - d.astype(np.int64)).sum(axis=1)
        if len(self.idx):
            self.win = int(self.idx[np.lexsort((self.idx, self.sad))[0]])  # min SAD, then lowest index
            self.tied = self.idx[self.sad == self.sad.min()]
        else:
            self.win, self.tied = -1, self.idx


class Circle:
    """The circle of one current-left feature: its steps, whether it closed
    and whether the disparity rules accepted it."""

    def __init__(self, f4, i2, D, Rr):
        F1, G1, F2, G2 = f4  # L1, R1, L2, R2
        self.i2, self.steps, self.closed, self.accepted, self.quad = i2, [], False, False, None
        c = F2.cls[i2]
        s = Step(G2, F2.u[i2], F2.v[i2], c, F2.desc[i2], 0, D, 1)
        self.steps.append(s)
        if s.win < 0:
            return
        r2 = s.win
        s = Step(G1, G2.u[r2], G2.v[r2], c, G2.desc[r2], -Rr, Rr, Rr)
        self.steps.append(s)
        if s.win < 0:
            return
        r1 = s.win
        s = Step(F1, G1.u[r1], G1.v[r1], c, G1.desc[r1], -D, 0, 1)
        self.steps.append(s)
        if s.win < 0:
            return
        l1 = s.win
        s = Step(F2, F1.u[l1], F1.v[l1], c, F1.desc[l1], -Rr, Rr, Rr)
        self.steps.append(s)
        self.closed = s.win == i2
        self.d1, self.d2 = int(F1.u[l1] - G1.u[r1]), int(F2.u[i2] - G2.u[r2])
        self.accepted = self.closed and self.d1 >= 1 and self.d2 >= 1
        self.quad = (l1, r1, i2, r2)


_circles = {}


def circles(case):
    if case.name not in _circles:
        p = match_params(case)
        _circles[case.name] = [Circle(case.f4, i2, p.disp_max, p.match_radius) for i2 in range(len(case.f4[2]))]
    return _circles[case.name]


def brute_force_match(case):
    q = [c.quad for c in circles(case) if c.accepted]
    return np.array(q, np.int32).reshape(len(q), 4)


# ------------------------------------------------------------------ census: the kernel's view of a step
class Geo:
    """A step as best_match (svo.hip) lays it out: column bands of width
    64 - 2 nms_n, the window's bands [ba, bq] and rows [va, vb], and the
    candidate list = the class's features of those bands and rows, band-major
    (each band in index order)."""

    def __init__(self, case, st):
        p = match_params(case)
        sw = 64 - 2 * p.nms_n
        nband = 4 * ((case.w + 4 * sw - 1) // (4 * sw))
        band = lambda u: np.minimum(np.asarray(u) // sw, nband - 1)  # noqa: E731
        self.sw, self.band = sw, band
        self.ua, self.ub = st.u - st.du_hi, st.u - st.du_lo
        self.ba, self.bq = int(band(max(self.ua, 0))), int(band(self.ub))
        self.nq = self.bq - self.ba + 1
        self.row_lo, self.row_hi = st.v - st.dv < 0, st.v + st.dv > case.h - 1
        va, vb = max(st.v - st.dv, 0), min(st.v + st.dv, case.h - 1)
        S = st.S
        b = band(S.u)
        m = (S.cls == st.c) & (S.v >= va) & (S.v <= vb) & (b >= self.ba) & (b <= self.bq)
        i = np.nonzero(m)[0]
        self.lst = i[np.lexsort((i, b[i]))]
        self.slot = {int(j): k for k, j in enumerate(self.lst)}
        self.win_band = int(band(S.u[st.win])) if st.win >= 0 else -1


def _accepted_steps(case):
    for c in circles(case):
        if c.accepted:
            for k, st in enumerate(c.steps):
                yield c, k, st, Geo(case, st)


def census(case):
    """Facts of a match case, each counted over the steps of ACCEPTED circles
    (a wrong winner there changes the output; in a rejected circle it would go
    unnoticed)."""
    f = dict(n=[len(s) for s in case.f4], accepted=0, max_list=0, last_slot_lists=[], max_span=0, ties=0,
             tie_band_inverted=0, tie_one_band=0, tie_across_halves=0, tie_same_lane=0, tie_closing=0,
             tie_not_closed=0, span8_first=0, span8_last=0, col_lo=0, col_hi_partial=0, row_lo_1=0, row_hi_1=0,
             row_lo_r=0, row_hi_r=0, row_both=0, disp_rejected_cur=0, disp_rejected_prev=0, empty_list_queries=0,
             win_32767=0, tie_lost_32767=0, disparities=set())
    cs = circles(case)
    f["accepted"] = sum(c.accepted for c in cs)
    for c in cs:
        if c.closed and not c.accepted:
            f["disp_rejected_cur"] += c.d2 < 1 and len(c.steps[0].idx) >= 2
            f["disp_rejected_prev"] += c.d1 < 1 and len(c.steps[2].idx) >= 2
        if len(c.steps) == 1 and c.steps[0].win < 0 and len(Geo(case, c.steps[0]).lst) == 0:
            f["empty_list_queries"] += 1
        if len(c.steps) == 4 and not c.closed and c.i2 in c.steps[3].tied:
            f["tie_not_closed"] += 1
        if c.accepted:
            f["disparities"].update((c.d1, c.d2))
    w_last_band = (case.w // (64 - 2 * match_params(case).nms_n)) * (64 - 2 * match_params(case).nms_n)
    for c, k, st, g in _accepted_steps(case):
        n = len(g.lst)
        f["max_list"] = max(f["max_list"], n)
        f["max_span"] = max(f["max_span"], g.nq)
        ws = g.slot[st.win]
        if ws == n - 1:
            f["last_slot_lists"].append(n)
        if g.nq == 8:
            f["span8_first"] += g.win_band == g.ba
            f["span8_last"] += g.win_band == g.bq
        f["col_lo"] += g.ua < 0
        f["col_hi_partial"] += g.ub >= case.w and case.w % g.sw != 0 and st.S.u[st.win] >= w_last_band
        if st.dv == 1:
            f["row_lo_1"] += g.row_lo
            f["row_hi_1"] += g.row_hi
        else:
            f["row_lo_r"] += g.row_lo
            f["row_hi_r"] += g.row_hi
        f["row_both"] += g.row_lo and g.row_hi
        if st.win == 32767:
            f["win_32767"] += 1
        if len(st.tied) >= 2:
            losers = [int(j) for j in st.tied if j != st.win]
            assert all(j > st.win for j in losers)
            f["ties"] += 1
            f["tie_closing"] += k == 3
            f["tie_lost_32767"] += 32767 in losers
            lb = g.band(st.S.u[losers])
            f["tie_band_inverted"] += bool((lb < g.win_band).any())
            f["tie_one_band"] += bool((lb == g.win_band).all())
            for j in losers:
                a, b = g.slot[j], ws
                if a // 128 == b // 128 and a % 128 < 64 <= b % 128:
                    f["tie_same_lane" if b - a == 64 else "tie_across_halves"] += 1
    return {k: int(v) if isinstance(v, (bool, np.generic)) else v for k, v in f.items()}


def census_line(case):
    f = census(case)
    f["last_slot_lists"] = [n for n in f["last_slot_lists"] if n >= 64]
    keep = {k: v for k, v in f.items() if k != "disparities" and v not in (0, [])}
    return f"{case.name}: w={case.w} h={case.h} {case.kw} {keep}"


# what each case must show (fact -> minimum count), beyond >= 1 accepted circle
EXPECT = {
    "tie_index_vs_band": dict(tie_band_inverted=1, tie_one_band=1, tie_across_halves=1, tie_same_lane=1,
                              tie_closing=1, tie_not_closed=1),
    "bands8": dict(span8_first=1, span8_last=1),
    "clamp_left": dict(col_lo=4),
    "clamp_right": dict(col_hi_partial=2),
    "clamp_rows": dict(row_lo_1=1, row_hi_1=1, row_lo_r=1, row_hi_r=1),
    "short_image": dict(row_both=4),
    "class_absent": dict(empty_list_queries=4),
    "zero_disparity_winner": dict(disp_rejected_cur=1, disp_rejected_prev=1),
    "index_32767": dict(win_32767=1, tie_lost_32767=1),
}


@pytest.mark.parametrize("case", MATCH_CASES, ids=repr)
def test_sets_are_valid_input(case):
    """What viso_svo_match requires of its input."""
    p = match_params(case)
    for S in case.f4:
        assert len(S) <= p.max_features
        assert S.u.dtype == S.v.dtype == S.cls.dtype == np.int32 and S.desc.dtype == np.uint8
        assert S.desc.shape == (len(S), 32)
        if len(S):
            assert (np.diff(S.v) >= 0).all()
            assert S.u.min() >= 0 and S.u.max() < case.w and S.v.min() >= 0 and S.v.max() < case.h
            assert S.cls.min() >= 0 and S.cls.max() <= 3


@pytest.mark.parametrize("case", MATCH_CASES, ids=repr)
def test_brute_force_equals_spec(case):
    """Scanning every feature with (SAD, index) order gives the spec's matches:
    the spec's row index loses no candidate and its tie rule is lowest index."""
    exp = ol.svo_match(case.f4, case.h, match_params(case))
    assert np.array_equal(brute_force_match(case), exp), census_line(case)


@pytest.mark.parametrize("case", MATCH_CASES, ids=repr)
def test_match_case_census(case):
    f = census(case)
    line = census_line(case)
    if case.name.startswith("empty_"):
        k = sc.SET_NAMES.index(case.name[6:])
        assert f["n"][k] == 0 and all(n > 0 for i, n in enumerate(f["n"]) if i != k), line
        assert f["accepted"] == 0, line
        return
    assert f["accepted"] >= 1, line
    for fact, least in EXPECT.get(case.name, {}).items():
        assert f[fact] >= least, (fact, line)
    if case.name.startswith("dense_"):
        # the query's list has exactly that many candidates, the winner in the last slot
        assert int(case.name[6:]) in f["last_slot_lists"], line
    if case.name == "bands8":
        assert f["max_span"] == 8 and {1, 335} <= f["disparities"], line
    if case.name == "class_absent":
        assert 1 not in case.f4[sc.R2].cls and (case.f4[sc.L2].cls == 1).sum() == 4, line
    if case.name == "index_32767":
        assert f["n"][sc.R2] == 32768 == match_params(case).max_features, line


def test_match_cases_cover_the_list():
    names = {c.name for c in MATCH_CASES}
    want = {"tie_index_vs_band", "bands8", "clamp_left", "clamp_right", "clamp_rows", "short_image", "empty_L1",
            "empty_R1", "empty_L2", "empty_R2", "class_absent", "zero_disparity_winner", "index_32767"}
    want |= {f"dense_{n}" for n in (64, 65, 128, 129, 256, 257, 400)}
    assert names == want
    short = next(c for c in MATCH_CASES if c.name == "short_image")
    assert short.h < 2 * match_params(short).match_radius + 1


# ------------------------------------------------------------------ motion cases: the spec's exits
def motion_params(ctx):
    w, h, kw = sc.MOTION_CONTEXTS[ctx]
    return ol.svo_params(w, h, *sc.K, **kw)


_spec_motion = {}


def spec_motion(case):
    """(motion, inlier mask, n or -1, trace) of the spec, computed once."""
    if case.name not in _spec_motion:
        m, inl, n = ol.svo_estimate(case.uv8, case.frame, motion_params(case.ctx))
        _spec_motion[case.name] = (m, inl, n, ol.svo_estimate_trace())
    return _spec_motion[case.name]


def tree_shape(M):
    """The reduction tree of svo_refine_kernel for M matches: leaves padded to
    P2, in-wave levels, 64-leaf chunks, levels over the chunks."""
    P2 = 1
    while P2 < M:
        P2 <<= 1
    nch = (P2 + 63) // 64
    return dict(P2=P2, lv_in=6 if P2 >= 64 else P2.bit_length() - 1, nch=nch, lv_out=(nch - 1).bit_length())


def motion_census_line(case):
    tr = spec_motion(case)[3]
    return (f"{case.name}: M={len(case.uv8)} ctx={case.ctx} frame={case.frame} exit={ol.SVO_EXIT_NAMES[tr['exit']]} "
            f"best_h={tr['best_h']} best_cnt={tr['best_cnt']} shared={tr['shared']} n_final={tr['n_final']} "
            f"tree={tree_shape(len(case.uv8))}")


def test_motion_cases_populate_every_exit():
    """Every exit of the spec's `estimate` is taken by a motion case,
    `refine_failed` included: it is reachable (a best hypothesis whose inliers
    are two distinct points, or points of one image row at one disparity,
    gives a singular refinement system; the hypothesis is then kept)."""
    seen = {}
    for c in MOTION_CASES:
        if not c.refused:
            seen.setdefault(spec_motion(c)[3]["exit"], []).append(c.name)
    for code, name in enumerate(ol.SVO_EXIT_NAMES):
        assert seen.get(code), name
    assert set(seen) == set(range(len(ol.SVO_EXIT_NAMES)))


@pytest.mark.parametrize("case", [c for c in MOTION_CASES if c.kind == "refine_failed"], ids=repr)
def test_refine_failure_cases(case):
    """The refinement's solve fails, the best hypothesis is kept: the result is
    that hypothesis' motion (not the identity) and its own inliers."""
    m, inl, n, tr = spec_motion(case)
    line = motion_census_line(case)
    assert tr["exit"] == ol.SVO_EXIT_REFINE_FAILED and n == tr["n_final"] == tr["best_cnt"] >= 6, line
    assert inl.sum() == n and not np.array_equal(m, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), line


def test_motion_cases_cover_the_tree_shapes():
    """Every branch of the refinement tree by M: lane_tree below 64 leaves,
    one chunk, several chunks, and 128 chunks (lv_out 7); the boundaries
    around 64, 4096 and the capacities."""
    by_ctx = {k: {len(c.uv8) for c in MOTION_CASES if c.ctx == k and not c.refused} for k in sc.MOTION_CONTEXTS}
    assert set(sc.DEFAULT_M) <= by_ctx["default"] and set(sc.LARGE_M) <= by_ctx["large"]
    shapes = {(t["lv_in"], t["lv_out"]) for t in (tree_shape(M) for M in by_ctx["default"] | by_ctx["large"])
              if t["P2"] >= 8}
    assert {(3, 0), (4, 0), (5, 0), (6, 0), (6, 1), (6, 2), (6, 3), (6, 4), (6, 6), (6, 7)} <= shapes
    for k, cap in sc.MOTION_MCAP.items():
        assert cap in by_ctx[k]
        assert [len(c.uv8) for c in MOTION_CASES if c.ctx == k and c.refused] == [cap + 1]
    # solved cases on both sides of every boundary (a failed estimate runs no tree)
    ok = {len(c.uv8) for c in MOTION_CASES if not c.refused and spec_motion(c)[2] > 0}
    assert {6, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 800, 4095, 4096, 4097, 8000} <= ok


@pytest.mark.parametrize("case", [c for c in MOTION_CASES if c.kind == "late_failure"], ids=repr)
def test_late_failure_cases(case):
    """A hypothesis with >= 6 inliers whose refined motion keeps only 1..5:
    the spec answers -1, the identity and an all-zero inlier mask."""
    m, inl, n, tr = spec_motion(case)
    line = motion_census_line(case)
    assert tr["exit"] == ol.SVO_EXIT_FINAL_FEW and tr["best_cnt"] >= 6 and 1 <= tr["n_final"] <= 5, line
    assert n == -1 and not inl.any() and np.array_equal(m, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), line


def test_all_fail_and_count_tie_cases():
    fail = next(c for c in MOTION_CASES if c.kind == "all_fail")
    assert len(np.unique(fail.uv8, axis=0)) == 2 and len(fail.uv8) == 12
    m, inl, n, tr = spec_motion(fail)
    assert tr["exit"] == ol.SVO_EXIT_NO_HYPOTHESIS and tr["best_cnt"] == 0 and tr["best_h"] == 0, tr
    assert n == -1 and not inl.any()
    tie = next(c for c in MOTION_CASES if c.kind == "count_tie")
    m, inl, n, tr = spec_motion(tie)
    assert len(tie.uv8) == 6 and n == 6 and inl.all()
    assert tr["best_cnt"] == 6 and tr["shared"] and tr["best_h"] == 0, tr


def test_trace_changes_no_result():
    """The traced estimate is the estimate: known-answer recovery as before,
    and reading the trace between calls leaves a repeated call unchanged."""
    c = next(c for c in MOTION_CASES if c.name == "m257_noise0.5_out")
    p = motion_params(c.ctx)
    a = ol.svo_estimate(c.uv8, c.frame, p)
    ol.svo_estimate_trace()
    b = ol.svo_estimate(c.uv8, c.frame, p)
    assert a[2] == b[2] > 150 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.abs(a[0] - sc.TURN)[:9].max() < 2e-3 and np.abs(a[0] - sc.TURN)[9:].max() < 0.05


# ------------------------------------------------------------------ viso_svo_create parameter bounds
VISO_OK, VISO_ERR_ARG, VISO_ERR_NODEVICE = 0, -1, -5


def _create(**kw):
    """viso_svo_create's return code (a created context is destroyed)."""
    from viso_amd import _lib, svo
    w, h = kw.pop("width", 640), kw.pop("height", 200)
    p = svo.default_params(w, h, *sc.K, **kw)
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    rc = lib.viso_svo_create(ctypes.byref(p), 0, ctypes.byref(ctx))
    if rc == VISO_OK:
        lib.viso_svo_destroy(ctx)
    else:
        assert not ctx.value
    return rc


ACCEPTED = (VISO_OK, VISO_ERR_NODEVICE)  # with / without a GPU: the arguments passed the check


def test_create_window_band_bound():
    """48-column bands (nms_n 8): a window of disp_max + 1 columns may span
    the 8 bands best_match reads only up to disp_max 335."""
    assert _create(nms_n=8, disp_max=335) in ACCEPTED
    assert _create(nms_n=8, disp_max=336) == VISO_ERR_ARG


def test_create_max_features_bound():
    """The packed (SAD, index) key of best_match holds 15 index bits."""
    assert _create(max_features=32768) in ACCEPTED
    assert _create(max_features=32769) == VISO_ERR_ARG


def test_create_selected_match_bound():
    """ncam x buckets x bucket_max <= 8192 = the leaves of svo_refine_kernel's tree."""
    one = dict(bucket_width=640, bucket_height=200)  # one bucket
    assert _create(bucket_max=8192, **one) in ACCEPTED
    assert _create(bucket_max=8193, **one) == VISO_ERR_ARG
    w, h, kw = sc.MOTION_CONTEXTS["large"]
    assert _create(width=w, height=h, **kw) in ACCEPTED
