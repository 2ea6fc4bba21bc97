"""Sliding-window map (viso_set_map_window / viso_map_retire,
include/viso/viso_c.h): an insertion into a full window first retires the
oldest keyframe and culls the points it hosts (DESIGN.md §Sliding-window map).
The repo's own spec, restated in tests/map_window_ref.py.

Sequence: that of tests/test_keyframes.py (the camera driving forward).  GPU
vs the restatement: keep flags, hosts, counts and the kept points exact (the
points are copies; the CPU test and every parity case show no decision within
1e-9 of a threshold), the pose after a retirement within 1e-10 relative of
oracle_lib.direct_pose on the new map (the bar of tests/test_mono_keyframes.py)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import map_window_ref, oracle_lib

CELL = 16
W, H = 1242, 375
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)


@functools.lru_cache(maxsize=None)
def _seq(w, h):
    from viso_amd.synth import Sequence
    return Sequence(w, h, seed=0, z_amp=20.0, z_period=1000.0)


@functools.lru_cache(maxsize=None)
def _image(w, h, f, cam=0):
    img = _seq(w, h).image(f, cam)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _pyr(w, h, f):
    p = oracle_lib.pyramid(_image(w, h, f))
    p.setflags(write=False)
    return p


def _world(points_cam, pose):
    R, t = np.asarray(pose[:9]).reshape(3, 3), np.asarray(pose[9:])
    return (np.asarray(points_cam, np.float64).reshape(-1, 3) - t) @ R


def _stereo_world(w, h, f):
    """Frame f's stereo points in world coordinates, by its ground-truth pose."""
    seq = _seq(w, h)
    xs, ys, _ = oracle_lib.fast(_image(w, h, f), 50)
    pc = oracle_lib.stereo_points(_image(w, h, f), _image(w, h, f, 1), xs, ys, 128, 1, seq.K, seq.p.baseline)
    return _world(pc, seq.pose(f))


# ------------------------------------------------------------------ CPU
def test_restatement_on_the_synthetic_sequence():
    """Window 2, an insertion every 5 frames, the ground-truth poses: every
    keyframe brings its stereo points; frames 10...40 each retire the older
    of the two keyframes."""
    w, h, interval, window = 320, 96, 5, 2
    seq = _seq(w, h)
    pts, kf = _stereo_world(w, h, 0), [0]
    host = np.zeros(len(pts), np.int32)
    retirements = 0
    for f in range(interval, 41, interval):
        if len(kf) == window:
            before = len(pts)
            r = map_window_ref.retire(pts, host, seq.pose(f), [seq.pose(k) for k in kf], seq.K, w, h, CELL)
            kept, survivors = len(r["points"]), r["counts"][3]
            print("frame", f, "map", before, "counts", r["counts"], "kept", kept, "culled", before - kept,
                  "margin", r["margin"])
            assert survivors >= 8
            assert before - kept >= 100
            assert kept >= 100
            # no decision sits on a threshold: the GPU tests may demand exact masks
            assert r["margin"] > 1e-9
            assert r["counts"][0] >= r["counts"][1] >= r["counts"][2] >= survivors
            assert kept == int(np.count_nonzero(host != 0)) + survivors
            pts, host, kf = r["points"], r["host"], kf[1:]
            assert host.max() < len(kf)
            retirements += 1
        new = _stereo_world(w, h, f)
        pts = np.concatenate([pts, new])
        host = np.concatenate([host, np.full(len(new), len(kf), np.int32)])
        kf.append(f)
    assert retirements == 7


K_HAND = (100.0, 100.0, 80.0, 48.0)
W_HAND, H_HAND = 160, 96


def _at(u, v, z=10.0):
    """The point that the identity pose sees at pixel (u, v), depth z."""
    return [(u - K_HAND[2]) / K_HAND[0] * z, (v - K_HAND[3]) / K_HAND[1] * z, z]


def _hand(points, host, kf_poses, pose_c=IDENT):
    return map_window_ref.retire(points, host, pose_c, kf_poses, K_HAND, W_HAND, H_HAND, CELL)


def _shifted(tx):
    p = IDENT.copy()
    p[9] = tx
    return p


def test_a_live_point_marks_its_cell():
    # cell (2, 1): a live point and a retired-host point; cell (5, 1): a retired-host point alone
    pts = [_at(40.0, 24.0), _at(42.0, 26.0), _at(88.0, 24.0)]
    r = _hand(pts, [1, 0, 0], [IDENT, IDENT])
    assert list(r["keep"]) == [1, 0, 1]
    assert list(r["host"]) == [0, 0]
    assert r["counts"] == [2, 2, 1, 1]
    # the same point with the live one elsewhere survives
    r = _hand([_at(120.0, 70.0)] + pts[1:], [1, 0, 0], [IDENT, IDENT])
    assert list(r["keep"]) == [1, 1, 1]


def test_the_higher_index_wins_a_cell():
    pts = [_at(40.0, 24.0), _at(42.0, 26.0), _at(44.0, 28.0), _at(100.0, 24.0)]
    r = _hand(pts, [0, 0, 0, 0], [IDENT, IDENT])
    assert list(r["keep"]) == [0, 0, 1, 1]
    assert r["counts"] == [4, 4, 4, 2]
    assert np.array_equal(r["points"], np.array(pts)[[2, 3]])


def test_unseen_points_die():
    behind = _at(40.0, 24.0, -10.0)
    outside = _at(-3.0, 24.0)
    # seen by c, but the only remaining keyframe looks 50 m to the side
    lost = _at(100.0, 24.0)
    r = _hand([behind, outside, lost], [0, 0, 0], [IDENT, _shifted(50.0)])
    assert list(r["keep"]) == [0, 0, 0]
    assert r["counts"] == [3, 1, 0, 0]
    # no remaining keyframe at all
    r = _hand([lost], [0], [IDENT])
    assert list(r["keep"]) == [0] and r["counts"] == [1, 1, 0, 0]


def test_the_survivor_is_hosted_by_the_newest_seeing_keyframe():
    P = _at(100.0, 24.0)
    # keyframes 1 and 2 see it, keyframe 3 (the newest) does not
    r = _hand([P], [0], [IDENT, IDENT, _shifted(0.1), _shifted(50.0)])
    assert list(r["keep"]) == [1] and list(r["host"]) == [1]
    r = _hand([P], [0], [IDENT, IDENT, _shifted(50.0), _shifted(50.0)])
    assert list(r["host"]) == [0]
    r = _hand([P], [0], [IDENT, _shifted(50.0), _shifted(0.1), IDENT])
    assert list(r["host"]) == [2]


def test_abi_exports_and_null_context():
    from viso_amd import _lib
    lib = _lib.load()
    for name in ("viso_set_map_window", "viso_get_map_window", "viso_get_point_hosts", "viso_map_retire"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.viso_set_map_window(None, 2, 16) == -1
    info = (ctypes.c_int64 * 8)()
    assert lib.viso_get_map_window(None, info) == -1
    n = ctypes.c_size_t(0)
    assert lib.viso_get_point_hosts(None, None, 0, ctypes.byref(n)) == -1
    assert lib.viso_map_retire(None, 320, 96, None, None, 1, None, None, 0, 16, None, None, None, ctypes.byref(n),
                               None) == -1


# ------------------------------------------------------------------ GPU: the stage
@functools.lru_cache(maxsize=None)
def _ctx(w, h):
    from viso_amd import api
    K = _seq(w, h).K
    return api.Context(api.default_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3], width=w, height=h))


def _rot(rng, deg):
    a = rng.normal(size=3)
    a *= np.deg2rad(deg) * rng.uniform() / np.linalg.norm(a)
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def _case(w, h, n, n_kf, seed):
    """Seeded points in and around c's frustum (depths 2-40 m, up to 20 % outside
    the image), random hosts (the retired keyframe's share growing with n),
    keyframes a few metres and degrees from c."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = _seq(w, h).K
    pose_c = _seq(w, h).pose(12)
    u = rng.uniform(-0.2 * w, 1.2 * w, n)
    v = rng.uniform(-0.2 * h, 1.2 * h, n)
    z = rng.uniform(2.0, 40.0, n)
    pts = _world(np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1), pose_c)
    Rc, tc = pose_c[:9].reshape(3, 3), pose_c[9:]
    kfs = []
    for _ in range(n_kf):
        dR = _rot(rng, 8.0)
        dt = rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 0.3, 4.0])
        kfs.append(np.concatenate([(dR @ Rc).ravel(), dR @ tc + dt]))
    # about 60 live points at most, so that some cells stay unmarked at every n
    live = rng.uniform(size=n) < min(0.5, 60.0 / max(n, 1))
    host = np.where(live & (n_kf > 1), rng.integers(1, max(n_kf, 2), n), 0).astype(np.int32)
    return pose_c, np.array(kfs), pts, host


def _parity(w, h, pose_c, kfs, pts, host, cell):
    r = map_window_ref.retire(pts, host, pose_c, kfs, _seq(w, h).K, w, h, cell)
    g = _ctx(w, h).map_retire(w, h, pose_c, kfs, pts, host, cell)
    print("n", len(host), "n_kf", len(kfs), "cell", cell, "gpu", g["counts"], g["n"], "ref", r["counts"],
          len(r["points"]), "margin", r["margin"])
    assert r["margin"] > 1e-9
    assert g["counts"] == r["counts"]
    assert g["n"] == len(r["points"])
    assert np.array_equal(g["keep"], r["keep"])
    assert np.array_equal(g["host"], r["host"])
    assert np.array_equal(g["points"], r["points"])  # copies: bit-equal
    return r


N_STAGE = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 16384]


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf", [1, 2, 8])
@pytest.mark.parametrize("n", N_STAGE)
def test_gpu_stage_matches_restatement(n, n_kf):
    """Point counts on both sides of a wave (64), a launch block (256), a
    compaction round (1024) and several rounds, at each cell size."""
    w, h = 320, 96
    pose_c, kfs, pts, host = _case(w, h, n, n_kf, seed=1000 * n_kf + n)
    kept = 0
    for cell in (8, 16, 64):
        r = _parity(w, h, pose_c, kfs, pts, host, cell)
        kept += r["counts"][3]
    if n >= 255 and n_kf > 1:
        assert kept > 0  # the case has survivors to get wrong


@pytest.mark.gpu
def test_gpu_stage_full_size_image():
    """1242 x 375: a partial last cell column (1242 = 77 x 16 + 10)."""
    pose_c, kfs, pts, host = _case(W, H, 5000, 3, seed=7)
    r = _parity(W, H, pose_c, kfs, pts, host, CELL)
    assert r["counts"][3] > 0


@pytest.mark.gpu
def test_gpu_stage_degenerate_sets():
    w, h = 320, 96
    seq = _seq(w, h)
    fx, fy, cx, cy = seq.K
    pose_c, kfs, pts, host = _case(w, h, 700, 3, seed=3)
    # all live
    r = _parity(w, h, pose_c, kfs, pts, np.where(host == 0, 1, host).astype(np.int32), CELL)
    assert r["keep"].all() and r["counts"] == [0, 0, 0, 0]
    # all hosted by the retired keyframe, none visible in c (behind it)
    rng = np.random.default_rng(5)
    z = -rng.uniform(2.0, 40.0, 700)
    back = _world(np.stack([rng.uniform(-3, 3, 700), rng.uniform(-1, 1, 700), z], axis=1), pose_c)
    g = _parity(w, h, pose_c, kfs, back, np.zeros(700, np.int32), CELL)
    assert not g["keep"].any() and g["counts"] == [700, 0, 0, 0]
    # every point in one cell, the keyframes at c: the last one alone survives...
    u, v = rng.uniform(161.0, 175.0, 700), rng.uniform(33.0, 47.0, 700)
    d = rng.uniform(2.0, 40.0, 700)
    one = _world(np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], axis=1), pose_c)
    same = np.array([pose_c, pose_c, pose_c])
    r = _parity(w, h, pose_c, same, one, np.zeros(700, np.int32), CELL)
    assert r["counts"] == [700, 700, 700, 1] and r["keep"][699] == 1 and list(r["host"]) == [1]
    # ...and none once a live point marks the cell
    hst = np.zeros(700, np.int32)
    hst[350] = 2
    r = _parity(w, h, pose_c, same, one, hst, CELL)
    assert r["counts"] == [699, 699, 0, 0] and int(r["keep"].sum()) == 1 and list(r["host"]) == [1]


@pytest.mark.gpu
def test_gpu_stage_argument_codes():
    from viso_amd import _lib
    lib, c = _lib.load(), _ctx(320, 96)
    pose = np.ascontiguousarray(IDENT)
    pts, host = np.zeros((2, 3)), np.zeros(2, np.int32)
    out, oh, keep = np.zeros((2, 3)), np.zeros(2, np.int32), np.zeros(2, np.uint8)
    n = ctypes.c_size_t(0)

    def call(w=320, h=96, n_kf=1, npts=2, cell=16, hosts=host):
        return lib.viso_map_retire(c.h, w, h, pose.ctypes.data, pose.ctypes.data, n_kf, pts.ctypes.data,
                                   hosts.ctypes.data, npts, cell, out.ctypes.data, oh.ctypes.data,
                                   keep.ctypes.data, ctypes.byref(n), None)

    assert call() == 0
    for kw in ({"w": 15}, {"h": 15}, {"w": 4097}, {"n_kf": 0}, {"n_kf": 9}, {"npts": -1}, {"npts": 16385},
               {"cell": 7}, {"cell": 65}, {"hosts": np.array([0, 1], np.int32)},
               {"hosts": np.array([-1, 0], np.int32)}):
        assert call(**kw) == -1, kw


# ------------------------------------------------------------------ GPU: the pipeline
def _new(w=W, h=H):
    import viso_amd
    seq = _seq(w, h)
    gv = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    gv.set_stereo(seq.p.baseline, 128, 1)
    return gv


def _n_points(gv):
    from viso_amd import _lib
    n = ctypes.c_size_t(0)
    _lib.call("viso_get_points", gv.ctx.h, None, 0, ctypes.byref(n))
    return int(n.value)


def _snapshot(gv):
    return {"points": gv.GetPoints(), "hosts": gv.point_hosts(), "kf": gv.keyframe_poses(),
            "info": gv.map_window(), "stats": gv.stats()}


def _run_per_frame(n, interval, window, mono=False, ba=0):
    """Stereo initialisation at frame 0; then a frame per call, with the
    map's state read around every check frame.  Returns before / after
    snapshots per check frame, the poses and the final snapshot."""
    gv = _new()
    if mono:
        gv.set_mono_keyframes(interval, 1000, CELL, 0.25)
    else:
        gv.set_keyframes(interval, 1000)
    gv.set_map_window(window, CELL)
    if ba:
        gv.set_bundle_adjust(ba)
    gv.process(_image(W, H, 0), _image(W, H, 0, 1))
    assert gv.state == 1
    around = {}
    for f in range(1, n):
        check = f % interval == 0
        before = _snapshot(gv) if check else None
        if mono:
            gv.OnNewFrame(_image(W, H, f))
        else:
            gv.process(_image(W, H, f), _image(W, H, f, 1))
        if check:
            around[f] = (before, _snapshot(gv))
    gv.synchronize()
    res = {"around": around, "poses": gv.poses, "final": _snapshot(gv)}
    gv.close()
    return res


_runs = {}


def _pipeline(kind):
    if kind not in _runs:
        _runs[kind] = _run_per_frame(31, 5, 2, mono=(kind == "mono"))
    return _runs[kind]


def _check_retirements(res, mono):
    seq = _seq(W, H)
    poses = res["poses"]
    retired = []
    for f, (b, a) in sorted(res["around"].items()):
        if a["info"][2] == b["info"][2]:
            continue  # (the window was not full yet)
        retired.append(f)
        pose_c = poses[f - 1]  # frame f is tracking frame f, pose f - 1
        r = map_window_ref.retire(b["points"], b["hosts"], pose_c, b["kf"], seq.K, W, H, CELL)
        kept = len(r["points"])
        print("frame", f, "map", len(b["points"]), "counts", r["counts"], "kept", kept, "after the insertion",
              len(a["points"]), "margin", r["margin"], "info", list(a["info"]))
        assert r["margin"] > 1e-9
        assert kept > 0
        assert np.array_equal(a["points"][:kept], r["points"])
        assert np.array_equal(a["hosts"][:kept], r["host"])
        n_kf = len(a["kf"])
        assert np.array_equal(a["kf"][:len(b["kf"]) - 1], b["kf"][1:])
        assert list(a["info"][4:7]) == [f, r["counts"][0], r["counts"][3]] and a["info"][7] == kept
        assert a["info"][2] == b["info"][2] + 1 and a["info"][3] == b["info"][3] + len(b["points"]) - kept
        # the check's own insertion, on top of the culled map
        added = len(a["points"]) - kept
        assert a["stats"][14] == added and a["stats"][15] == n_kf
        if added or not mono:
            assert n_kf == 2 and (a["hosts"][kept:] == 1).all()
            assert np.array_equal(a["kf"][1], pose_c)
        else:
            assert n_kf == 1
        if not mono:
            assert a["stats"][15] == 2
        # the next frame tracks against the new map (the run's last frame has no next one)
        if f < len(poses):
            exp = oracle_lib.direct_pose(_pyr(W, H, f), _pyr(W, H, f + 1), W, H, seq.K, a["points"], pose_c, pose_c)
            rel = np.linalg.norm(poses[f] - exp) / np.linalg.norm(exp)
            print("  next pose relative difference", rel)
            assert rel < 1e-10
    return retired


@pytest.mark.gpu
def test_gpu_pipeline_retirements_match_restatement():
    """1242 x 375, stereo insertion every 5 frames, window 2, 31 frames a call
    each: one-step parity at every retirement."""
    res = _pipeline("stereo")
    assert _check_retirements(res, mono=False) == [10, 15, 20, 25, 30]
    assert res["final"]["info"][2] == 5 and res["final"]["stats"][15] == 2


@pytest.mark.gpu
def test_gpu_pipeline_monocular_schedule():
    """The monocular insertion's schedule (BA off), window 2: frame 10 retires
    the keyframe of the initial map."""
    res = _pipeline("mono")
    retired = _check_retirements(res, mono=True)
    print("retirements at", retired)
    assert retired and retired[0] == 10
    b, a = res["around"][10]
    assert (b["hosts"] == 0).any() and len(b["kf"]) == 2


@pytest.mark.gpu
def test_gpu_pipeline_ingest_forms_agree():
    import torch
    a = _pipeline("stereo")
    n = 31
    gv = _new()
    gv.set_keyframes(5, 1000)
    gv.set_map_window(2, CELL)
    gv.process(_image(W, H, 0), _image(W, H, 0, 1))
    dl = torch.from_numpy(np.stack([_image(W, H, f) for f in range(1, n)])).cuda()
    dr = torch.from_numpy(np.stack([_image(W, H, f, 1) for f in range(1, n)])).cuda()
    torch.cuda.synchronize()
    gv.process_device(dl.data_ptr(), dr.data_ptr(), n - 1, W * H)
    gv.synchronize()
    b = _snapshot(gv)
    poses = gv.poses
    gv.close()
    fa = a["final"]
    assert fa["points"].shape == b["points"].shape
    assert np.array_equal(fa["hosts"], b["hosts"])
    assert np.array_equal(fa["info"], b["info"])
    assert fa["stats"][14] == b["stats"][14] and fa["stats"][15] == b["stats"][15]
    assert np.abs(fa["points"] - b["points"]).max() <= 1e-9 * np.abs(fa["points"]).max()
    assert fa["kf"].shape == b["kf"].shape
    assert np.abs(fa["kf"] - b["kf"]).max() <= 1e-10 * np.linalg.norm(fa["kf"], axis=1).max()
    rel = np.linalg.norm(a["poses"] - poses, axis=1) / np.linalg.norm(a["poses"], axis=1)
    assert rel.max() < 1e-10, rel.max()


@pytest.mark.gpu
def test_gpu_off_is_off():
    def run(setter):
        gv = _new()
        gv.set_keyframes(5, 1000)
        if setter:
            gv.set_map_window(0, 16)
        for f in range(16):
            gv.process(_image(W, H, f), _image(W, H, f, 1))
        gv.synchronize()
        out = gv.poses, gv.GetPoints(), gv.map_window(), gv.stats()
        gv.close()
        return out
    a, b = run(False), run(True)
    assert len(a[0]) == 15 and np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert a[2][2] == 0 and b[2][2] == 0 and a[2][0] == 0 and b[2][4] == -1
    assert a[3][15] == b[3][15] and a[3][15] > 2


def _long_run(window):
    """61 frames, stereo insertion every 5; per frame: stats, the map size and
    the direct pose's time."""
    gv = _new()
    gv.set_keyframes(5, 1000)
    if window:
        gv.set_map_window(window, CELL)
    gv.ctx.timing_enable(True)
    gv.ctx.timing_select(["direct"])
    rows, t_prev = [], 0.0
    for f in range(61):
        gv.process(_image(W, H, f), _image(W, H, f, 1))
        gv.synchronize()
        st = gv.stats()
        t = gv.ctx.timing("direct")[1]
        rows.append((f, st[9], _n_points(gv), t - t_prev, st[14], st[15]))
        t_prev = t
    info = gv.map_window()
    gv.close()
    return rows, info


@pytest.mark.gpu
def test_gpu_insertion_no_longer_stops():
    rows, info = _long_run(3)
    frozen, finfo = _long_run(0)
    for name, rr in (("window 3", rows), ("no window", frozen)):
        print(name, ": frame, level-0 nGood, map size, direct ms, points added, keyframes")
        for r in rr:
            print("  %2d %6d %6d %7.3f %5d %d" % r)
    cells = -(-W // CELL) * -(-H // CELL)
    per_insertion = [rows[0][2]]  # the initial map counts as one
    for f, _, n_map, _, added, n_kf in rows:
        if f > 0 and f % 5 == 0:
            if f >= 15:
                assert added > 0, f
            per_insertion.append(int(added))
        assert n_map <= sum(sorted(per_insertion)[-3:]) + cells, (f, n_map)
        assert n_kf <= 3
    assert info[2] == 10
    assert rows[-1][5] == 3
    for f, _, _, _, added, _ in frozen:
        if f >= 40 and f % 5 == 0:
            assert added == 0, f
    assert finfo[2] == 0


@pytest.mark.gpu
def test_gpu_bundle_adjust_composes():
    off = _run_per_frame(31, 5, 3)
    on = _run_per_frame(31, 5, 3, ba=2)
    assert sorted(on["around"]) == sorted(off["around"])
    for f in sorted(on["around"]):
        a, a0 = on["around"][f][1], off["around"][f][1]
        assert np.isfinite(a["points"]).all() and np.isfinite(a["kf"]).all()
        assert a["stats"][15] == a0["stats"][15] and len(a["kf"]) == len(a0["kf"])
        assert a["info"][2] == a0["info"][2] and a["info"][4] == a0["info"][4]
        assert len(a["hosts"]) == len(a["points"])
        assert a["hosts"].min() >= 0 and a["hosts"].max() < len(a["kf"])
    assert np.isfinite(on["poses"]).all() and len(on["poses"]) == 30
    assert on["final"]["info"][2] == off["final"]["info"][2] == 4
    assert on["final"]["stats"][15] == 3


@pytest.mark.gpu
def test_gpu_setter_codes():
    from viso_amd import _lib
    gv = _new()
    lib, h = _lib.load(), gv.ctx.h
    for window, cell in ((1, 16), (9, 16), (-1, 16), (2, 7), (2, 65)):
        assert lib.viso_set_map_window(h, window, cell) == -1, (window, cell)
    for window, cell in ((2, 8), (8, 64), (0, 16), (0, 0)):
        assert lib.viso_set_map_window(h, window, cell) == 0, (window, cell)
    gv.set_keyframes(5, 1000)
    for f in range(11):
        gv.process(_image(W, H, f), _image(W, H, f, 1))
    gv.synchronize()
    assert gv.stats()[15] == 3
    assert lib.viso_set_map_window(h, 2, 16) == -4  # three keyframes already
    assert lib.viso_set_map_window(h, 3, 16) == 0
    assert list(gv.map_window()[:5]) == [3, 16, 0, 0, -1]
    gv.close()
