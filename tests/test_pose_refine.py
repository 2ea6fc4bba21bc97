"""Pose refinement (viso_set_pose_refine / viso_refine_pose,
include/viso/viso_c.h; DESIGN.md §Pose refinement): every tracking frame's
direct pose is refined on its LK-aligned features.  The repo's own spec,
restated in tests/pose_refine_ref.py; the reference computes the aligned
positions (src/viso.cpp:121) and only draws them (src/viso.cpp:123-135).

GPU vs the restatement: status, observations, steps and inliers exact where
the restatement's recorded margin is above 1e-9, costs and rms within 1e-9
relative, the pose within 1e-10 relative (the bar of tests/test_pipeline.py).
The sums' order is fixed and restated exactly, so the two sides differ only
where sin / cos round differently; summing in a shuffled order instead moves
the n = 2465 pose by 2e-16 relative at most (test_sensitivity_to_the_order_of_
the_sums, DESIGN.md §Pose refinement), far below the bar, which therefore
stands as it is.

Stage parity runs 3 iterations: from the 4.4e-2 start the cost still falls by
more than 1e-5 relative in pass 3, while passes 4 and 5 change it by 1e-8 to
1e-13 (converged), which would put decision 2 on a rounding error."""
import functools

import numpy as np
import pytest

from tests import oracle_lib
from tests import pose_refine_ref as ref

K_KITTI = (718.856, 718.856, 607.19, 185.22)
XI_TRUE = [0.3, -0.1, 0.5, 0.01, 0.03, -0.02]
XI_START = [0.05, -0.03, 0.04, 0.02, -0.015, 0.01]
IDENT = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
BAR = 1e-10
PARITY_N = (0, 5, 6, 63, 64, 65, 1023, 1024, 1025, 2049, 16384)
PARITY_ITER, PARITY_SEED = 3, 0


def _dist(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _project(P, T):
    T = np.asarray(T, np.float64)
    Pc = np.asarray(P).reshape(-1, 3) @ T[:9].reshape(3, 3).T + T[9:]
    fx, fy, cx, cy = K_KITTI
    return np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], 1)


def _scene(n, seed, noise=0.0, outliers=0.0, exclusions=False):
    """Points uniform in x +-15, y +-4, z 5..60 seen from T_true; uv_after =
    their projections (+ noise px Gaussian, a fraction displaced by up to
    +-30 px); the start exp(XI_START) T_true.  exclusions: rows i >= 6 with
    i % 17 == 3 have no pair, i % 19 == 5 failed, i % 23 == 7 moved 20 px."""
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-15, 15, n), rng.uniform(-4, 4, n), rng.uniform(5, 60, n)], 1)
    T_true = np.array(ref.left_update(XI_TRUE, IDENT))
    ua = _project(P, T_true) + noise * rng.standard_normal((n, 2))
    m = rng.random(n) < outliers
    ua[m] += rng.uniform(-30, 30, (int(m.sum()), 2))
    ub = ua + rng.uniform(-1, 1, (n, 2))
    pk = np.zeros(n, np.int32)
    sc = np.ones(n, np.uint8)
    if exclusions:
        i = np.arange(n)
        pk[(i >= 6) & (i % 17 == 3)] = -1
        sc[(i >= 6) & (i % 19 == 5)] = 0
        ub[(i >= 6) & (i % 23 == 7)] += 20.0
    X = np.array(ref.left_update(XI_START, list(T_true)))
    return {"P": P, "pk": pk, "sc": sc, "ub": ub, "ua": ua, "T_true": T_true, "X": X}


def _refine(s, iterations, huber=1.0, shift=8.0, **kw):
    return ref.refine(s["P"], s["pk"], s["sc"], s["ub"], s["ua"], s["X"], K_KITTI, iterations, huber, shift, **kw)


@functools.lru_cache(maxsize=None)
def _parity_case(n, iterations=PARITY_ITER):
    s = _scene(n, PARITY_SEED, noise=0.1, outliers=0.2, exclusions=True)
    return s, _refine(s, iterations)


# ------------------------------------------------------------------ CPU
@pytest.mark.parametrize("n", [6, 64, 2465])
def test_noise_free_recovery(n):
    s = _scene(n, 1)
    r = _refine(s, 5)
    d0, d = _dist(s["X"], s["T_true"]), _dist(r["pose"], s["T_true"])
    print("n", n, "start", d0, "result", d, "report", r["report"])
    assert d0 > 4e-2 and d <= 1e-12
    assert r["report"][0] == n and r["report"][5] in (0, 3)
    assert r["report"][7] <= 1e-9 < r["report"][6]


def test_outliers_are_down_weighted():
    s = _scene(2465, 2, outliers=0.2)
    r = _refine(s, 5, huber=1.0, shift=1e9)
    d0, d = _dist(s["X"], s["T_true"]), _dist(r["pose"], s["T_true"])
    print("start", d0, "result", d, "ratio", d0 / d, "inliers", r["report"][4])
    assert d * 50 <= d0
    assert 0.7 * 2465 < r["report"][4] < 0.9 * 2465


def test_five_observations_abandon():
    s = _scene(5, 3)
    r = _refine(s, 5)
    assert r["report"][5] == 1 and r["report"][1] == 0 and r["report"][0] == 5
    assert np.array_equal(r["pose"], s["X"])
    assert r["report"][3] == r["report"][2] and r["report"][7] == r["report"][6]
    assert len(r["passes"]) == 1


def _one_image_point():
    """Six observations of one point on the optical axis: J^T J has two zero rows."""
    P = np.tile([[0.0, 0.0, 10.0]], (6, 1))
    ua = np.tile([[K_KITTI[2] + 0.25, K_KITTI[3] - 0.5]], (6, 1))
    return {"P": P, "pk": np.zeros(6, np.int32), "sc": np.ones(6, np.uint8), "ub": ua.copy(), "ua": ua,
            "X": np.array(IDENT)}


def test_degenerate_geometry_is_status_2():
    s = _one_image_point()
    r = _refine(s, 5)
    assert r["report"][5] == 2 and r["report"][1] == 0 and r["report"][0] == 6
    assert np.array_equal(r["pose"], s["X"])


def _behind_scene():
    """The scene of 64 points plus one that the start sees 0.02 in front of
    the camera and the first step puts behind it."""
    s = _scene(64, 4)
    R, t = s["X"][:9].reshape(3, 3), s["X"][9:]
    Pc = np.array([0.001, 0.001, 0.02])
    s["P"] = np.vstack([s["P"], (Pc - t) @ R])
    uv = _project(s["P"][-1:], s["X"])
    s["ua"] = np.vstack([s["ua"], uv])
    s["ub"] = np.vstack([s["ub"], uv])
    s["pk"] = np.zeros(65, np.int32)
    s["sc"] = np.ones(65, np.uint8)
    return s


def test_a_point_that_turns_behind_the_camera_is_skipped():
    s = _behind_scene()
    r = _refine(s, 5)
    used = [p[0] for p in r["passes"]]
    print("used per pass", used, "report", r["report"])
    assert r["report"][0] == 65 and used[0] == 65 and used[-1] == 64
    assert _dist(r["pose"], s["T_true"]) <= 1e-12


def test_shift_and_success_exclude_exactly_their_rows():
    s = _scene(200, 5, exclusions=True)
    i = np.arange(200)
    want = [int(j) for j in i if not (j >= 6 and (j % 17 == 3 or j % 19 == 5 or j % 23 == 7))]
    r = _refine(s, 3)
    assert r["observations"] == want and r["report"][0] == len(want) < 200
    # the excluded rows' content does not matter
    t = {k: v.copy() for k, v in s.items()}
    out = np.setdiff1d(i, want)
    t["ua"][out] += 1000.0
    t["ub"][out] += 1000.0
    t["ub"][(i >= 6) & (i % 23 == 7)] += 20.0
    r2 = _refine(t, 3)
    assert np.array_equal(r2["pose"], r["pose"]) and np.array_equal(r2["report"], r["report"])
    # the threshold itself: a shift of exactly max_shift_px is an observation
    e = _scene(8, 6)
    e["ub"] = e["ua"] - np.array([3.0, 4.0])
    assert _refine(e, 1, shift=5.0)["report"][0] == 8
    assert _refine(e, 1, shift=4.999)["report"][5] == 1


def test_sensitivity_to_the_order_of_the_sums():
    s = _scene(2465, PARITY_SEED, noise=0.1, outliers=0.2, exclusions=True)
    base = _refine(s, PARITY_ITER)
    spread = max(_dist(_refine(s, PARITY_ITER, permute_seed=k)["pose"], base["pose"]) for k in range(4))
    print("pose spread over 4 shuffled summation orders", spread)
    # an order of magnitude below the bar: the 1e-10 bar needs no widening
    assert spread <= 0.1 * BAR


def test_parity_cases_sit_clear_of_every_threshold():
    for n in PARITY_N:
        s, r = _parity_case(n)
        m = r["margin"]
        print("n", n, "report", r["report"], "margins", m.shift, m.z, m.huber, m.cost)
        assert m.value > 1e-9, n
        if n >= 6:
            assert r["report"][5] == 0 and r["report"][1] == PARITY_ITER
            assert 0 < r["report"][4] < r["report"][0]  # both Huber branches at the result
            assert r["passes"][0][2] < r["passes"][0][0]
        else:
            assert r["report"][5] == 1
        if n >= 63:
            assert r["report"][0] < n


def test_abi_exports_and_null_context():
    from viso_amd import _lib
    lib = _lib.load()
    for name in ("viso_set_pose_refine", "viso_get_pose_refine", "viso_refine_pose"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert _lib.KERNEL_IDS["refine"] == 10
    rep = np.zeros(8)
    pose = np.zeros(12)
    assert lib.viso_set_pose_refine(None, 5, 1.0, 8.0) == -1
    assert lib.viso_get_pose_refine(None, rep.ctypes.data) == -1
    assert lib.viso_refine_pose(None, None, None, None, None, None, 0, pose.ctypes.data, 5, 1.0, 8.0,
                                pose.ctypes.data, rep.ctypes.data) == -1


# ------------------------------------------------------------------ GPU: the stage
@functools.lru_cache(maxsize=None)
def _ctx():
    from viso_amd import api
    fx, fy, cx, cy = K_KITTI
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=1242, height=375))


def _gpu(s, iterations, huber=1.0, shift=8.0):
    return _ctx().refine_pose(s["P"], s["pk"], s["sc"], s["ub"], s["ua"], s["X"], iterations, huber, shift)


def _same(got, r):
    pose, rep = got
    exp = r["report"]
    print("gpu", rep, "\nref", exp, "\nmargin", r["margin"].value)
    if r["margin"].value > 1e-9:
        for k in (0, 1, 4, 5):
            assert rep[k] == exp[k], k
    else:
        assert rep[0] == exp[0]
    if rep[5] == exp[5] and rep[1] == exp[1]:
        for k in (2, 3, 6, 7):
            assert abs(rep[k] - exp[k]) <= 1e-9 * abs(exp[k]), k
    d = _dist(pose, r["pose"])
    print("pose relative difference", d)
    assert d < BAR


@pytest.mark.gpu
@pytest.mark.parametrize("n", PARITY_N)
def test_gpu_stage_matches_restatement(n):
    """The abandon threshold (5, 6), one wave +-1, one pass of the workgroup
    +-1, lanes with unequal counts (2049) and the capacity."""
    s, r = _parity_case(n)
    _same(_gpu(s, PARITY_ITER), r)


@pytest.mark.gpu
def test_gpu_stage_runs_until_the_cost_stops_falling():
    """20 iterations: the restatement stops with status 3 on a cost
    difference at rounding level, so the status and the step count are
    compared only if its margin allows; the pose is converged either way."""
    s = _scene(65, PARITY_SEED, noise=0.1, outliers=0.2, exclusions=True)
    r = _refine(s, 20)
    assert r["report"][5] == 3
    _same(_gpu(s, 20), r)


@pytest.mark.gpu
def test_gpu_stage_crafted_decisions():
    s = _one_image_point()
    pose, rep = _gpu(s, 5)
    assert rep[5] == 2 and rep[1] == 0 and rep[0] == 6 and np.array_equal(pose, s["X"])
    s = _scene(5, 3)
    pose, rep = _gpu(s, 5)
    assert rep[5] == 1 and rep[0] == 5 and np.array_equal(pose, s["X"])
    s = _behind_scene()
    _same(_gpu(s, 5), _refine(s, 5))
    e = _scene(8, 6)
    e["ub"] = e["ua"] - np.array([3.0, 4.0])
    assert _gpu(e, 1, shift=5.0)[1][0] == 8
    assert _gpu(e, 1, shift=4.999)[1][5] == 1


@pytest.mark.gpu
def test_gpu_stage_argument_codes():
    from viso_amd import _lib
    lib, h = _lib.load(), _ctx().h
    s = _scene(8, 7)
    P, pk, sc, ub, ua = (np.ascontiguousarray(s[k]) for k in ("P", "pk", "sc", "ub", "ua"))
    X, out, rep = np.ascontiguousarray(s["X"]), np.zeros(12), np.zeros(8)

    def call(n=8, it=5, hub=1.0, shift=8.0, po=out, rp=rep, pin=X, pts=P):
        return lib.viso_refine_pose(h, None if pts is None else pts.ctypes.data, pk.ctypes.data, sc.ctypes.data,
                                    ub.ctypes.data, ua.ctypes.data, n, None if pin is None else pin.ctypes.data,
                                    it, hub, shift, None if po is None else po.ctypes.data,
                                    None if rp is None else rp.ctypes.data)

    assert call() == 0
    for kw in ({"n": -1}, {"n": 16385}, {"it": 0}, {"it": 21}, {"hub": 0.0}, {"hub": -1.0}, {"shift": 0.0},
               {"shift": -2.0}, {"po": None}, {"rp": None}, {"pin": None}, {"pts": None}):
        assert call(**kw) == -1, kw
    assert call(it=1) == 0 and call(it=20) == 0


# ------------------------------------------------------------------ GPU: the pipeline
W, H = 416, 128  # the smallest synthetic size whose stereo initialisation makes a map (328 points)
N_PIPE = 13      # the stereo frame and 12 tracking frames
REFINE = (5, 1.0, 8.0)


@functools.lru_cache(maxsize=None)
def _seq():
    from viso_amd.synth import Sequence
    return Sequence(W, H, seed=0, z_amp=20.0, z_period=1000.0)


@functools.lru_cache(maxsize=None)
def _image(f, cam=0):
    img = _seq().image(f, cam)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _pyr(f):
    p = oracle_lib.pyramid(_image(f))
    p.setflags(write=False)
    return p


def _viso(refine=REFINE, mono=None, window=None, ba=0):
    import viso_amd
    seq = _seq()
    gv = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32)
    gv.set_stereo(seq.p.baseline, 128, 1)
    if refine is not None:
        gv.set_pose_refine(*refine)
    if mono:
        gv.set_mono_keyframes(*mono)
    if window:
        gv.set_map_window(*window)
    if ba:
        gv.set_bundle_adjust(ba)
    gv.process(_image(0), _image(0, 1))
    assert gv.state == 1
    return gv


def _expected(f, points, prev_pose, kf_frames, kf_poses):
    """Frame f's refined pose by the restatement: the oracle's direct pose
    from the GPU's own previous pose, its LK row at that pose."""
    K = _seq().K
    X = oracle_lib.direct_pose(_pyr(f - 1), _pyr(f), W, H, K, points, prev_pose, prev_pose)
    pk, sc, ub, ua = oracle_lib.lk_align([_pyr(k) for k in kf_frames], kf_poses, _pyr(f), X, W, H, K, points)
    return ref.refine(points, pk, sc, ub, ua, X, K, *REFINE), X


_runs = {}


def _pipeline(batched):
    if batched not in _runs:
        gv = _viso()
        pts = gv.GetPoints()
        reports = []
        if batched:
            import torch
            dl = torch.from_numpy(np.stack([_image(f) for f in range(1, N_PIPE)])).cuda()
            torch.cuda.synchronize()
            gv.process_device(dl.data_ptr(), None, N_PIPE - 1, W * H)
            gv.synchronize()
            reports.append(gv.pose_refine())
        else:
            for f in range(1, N_PIPE):
                gv.OnNewFrame(_image(f))
                reports.append(gv.pose_refine())
        _runs[batched] = {"points": pts, "poses": gv.poses, "reports": np.array(reports), "align": gv.alignment()}
        gv.close()
    return _runs[batched]


@pytest.mark.gpu
def test_gpu_pipeline_one_step_parity():
    res = _pipeline(False)
    pts, poses, reports = res["points"], res["poses"], res["reports"]
    assert len(poses) == N_PIPE - 1 and len(pts) > 50
    prev = np.array(IDENT)
    for f in range(1, N_PIPE):
        r, X = _expected(f, pts, prev, [0], [IDENT])
        d = _dist(poses[f - 1], r["pose"])
        rep = reports[f - 1]
        print("frame", f, "relative difference", d, "moved from X by", _dist(r["pose"], X), "\n  gpu", rep,
              "\n  ref", r["report"])
        assert d < BAR
        assert rep[0] == r["report"][0] and rep[0] > 0
        assert rep[7] <= rep[6]
        assert not np.array_equal(poses[f - 1], X)
        prev = poses[f - 1]
    # viso_get_alignment still reports the alignment computed at X
    pk, sc, ub, ua = res["align"]
    K = _seq().K
    X = oracle_lib.direct_pose(_pyr(N_PIPE - 2), _pyr(N_PIPE - 1), W, H, K, pts, poses[-2], poses[-2])
    at_x = oracle_lib.lk_align([_pyr(0)], [IDENT], _pyr(N_PIPE - 1), X, W, H, K, pts)
    at_res = oracle_lib.lk_align([_pyr(0)], [IDENT], _pyr(N_PIPE - 1), poses[-1], W, H, K, pts)
    m = (pk >= 0) & (at_x[0] >= 0) & (at_res[0] >= 0)
    assert m.sum() > 50
    d_x, d_res = np.abs(ub - at_x[2])[m].max(), np.abs(ub - at_res[2])[m].max()
    print("uv_before against the oracle's at X", d_x, "at the refined pose", d_res)
    assert d_x < 1e-6 < 1e-4 < d_res


@pytest.mark.gpu
def test_gpu_pipeline_ingest_forms_agree():
    a, b = _pipeline(False), _pipeline(True)
    assert np.array_equal(a["poses"], b["poses"])
    assert np.array_equal(a["reports"][-1], b["reports"][-1])


@pytest.mark.gpu
def test_gpu_off_is_off():
    runs = []
    for refine in (None, (0, 1.0, 8.0)):
        gv = _viso(refine=None)
        cfg = gv.config()
        if refine is not None:
            gv.set_pose_refine(*refine)
            assert gv.config() == cfg
        for f in range(1, 8):
            gv.OnNewFrame(_image(f))
        assert np.isnan(gv.pose_refine()).all()
        assert gv.ctx.timing("refine")[0] == 0
        runs.append(gv.poses)
        gv.close()
    assert np.array_equal(runs[0], runs[1]) and len(runs[0]) == 7
    # and on, it moves the poses
    assert not np.array_equal(_pipeline(False)["poses"][:7], runs[0])


@pytest.mark.gpu
def test_gpu_setter_codes_and_setting_while_tracking():
    from viso_amd import _lib
    gv = _viso(refine=None)
    lib, h = _lib.load(), gv.ctx.h
    for it, hub, shift in ((-1, 1.0, 8.0), (21, 1.0, 8.0), (5, 0.0, 8.0), (5, -1.0, 8.0), (5, 1.0, 0.0),
                           (5, 1.0, -8.0), (5, float("nan"), 8.0)):
        assert lib.viso_set_pose_refine(h, it, hub, shift) == -1, (it, hub, shift)
    for it in (1, 20, 0):
        assert lib.viso_set_pose_refine(h, it, 0.5, 3.0) == 0
    assert lib.viso_set_pose_refine(h, 0, 0.0, 0.0) == 0  # off: the other two are not read
    pts = gv.GetPoints()
    gv.ctx.timing_enable(True)
    gv.OnNewFrame(_image(1))
    gv.OnNewFrame(_image(2))
    assert np.isnan(gv.pose_refine()).all()
    gv.set_pose_refine(*REFINE)  # while tracking: frame 3 is the first refined
    gv.OnNewFrame(_image(3))
    poses = gv.poses
    assert gv.ctx.timing("refine")[0] == 1
    K = _seq().K
    X2 = oracle_lib.direct_pose(_pyr(1), _pyr(2), W, H, K, pts, poses[0], poses[0])
    assert _dist(poses[1], X2) < BAR
    r, _ = _expected(3, pts, poses[1], [0], [IDENT])
    assert _dist(poses[2], r["pose"]) < BAR
    assert gv.pose_refine()[0] == r["report"][0]
    gv.set_pose_refine(0)
    gv.OnNewFrame(_image(4))
    X4 = oracle_lib.direct_pose(_pyr(3), _pyr(4), W, H, K, pts, poses[2], poses[2])
    assert _dist(gv.poses[3], X4) < BAR and gv.ctx.timing("refine")[0] == 1
    gv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ba", [2, 0])
def test_gpu_composes_with_insertion_window_and_ba(ba):
    """Monocular insertion every 5th frame (8-pixel cells, 0.1 degrees: some
    sixty points per insertion at this size), a window of 2 keyframes and,
    for ba = 2, the BA behind every insertion, over 20 frames.  The frame
    after every insertion has one-step parity against the map, the keyframes
    and the pose (the BA's, when on) that the insertion left."""
    n = 21
    gv = _viso(mono=(5, 1000, 8, 0.1), window=(2, 16), ba=ba)
    kf_frames, snaps = [0], {}
    retired = 0
    for f in range(1, n):
        gv.OnNewFrame(_image(f))
        st = gv.stats()
        if st[14] > 0:
            now = int(gv.map_window()[2])
            if now > retired:
                kf_frames = kf_frames[1:]
                retired = now
            kf_frames = kf_frames + [f]
            snaps[f] = (gv.GetPoints(), gv.keyframe_poses(), list(kf_frames))
    poses = gv.poses
    kf_end = gv.keyframe_poses()
    gv.close()
    print("insertions at", sorted(snaps), "keyframes at the end", kf_frames, "retired", retired)
    assert len(poses) == n - 1 and np.isfinite(poses).all() and np.isfinite(kf_end).all()
    assert len(snaps) >= 2 and retired >= 1 and len(kf_end) == len(kf_frames) == 2
    for f, (pts, kfp, frames) in sorted(snaps.items()):
        assert np.isfinite(pts).all()
        if not ba:
            # a keyframe's pose is its frame's refined pose
            for k, kf in enumerate(frames):
                if kf > 0:
                    assert np.array_equal(kfp[k], poses[kf - 1]), (f, kf)
        if f + 1 < n:
            r, X = _expected(f + 1, pts, kfp[-1], frames, kfp)
            d = _dist(poses[f], r["pose"])
            print("frame", f + 1, "after the insertion at", f, "relative difference", d, "observations",
                  r["report"][0], "of", len(pts))
            assert d < BAR and r["report"][0] > 0
