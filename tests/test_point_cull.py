"""Map point culling (viso_set_point_cull / viso_point_tracks_update /
viso_points_cull, include/viso/viso_c.h; DESIGN.md §Map point culling): every
map point keeps a track record {age, seen, found, fail_run} of its LK
alignments, and the points that keep failing leave the map.  The repo's own
spec, restated in tests/point_cull_ref.py; the reference computes the
alignments (src/viso.cpp:768-843) and only draws them.

Everything compared is an integer or a copied coordinate, so GPU and
restatement must be equal.  A flag could differ only where the reprojection
error sits on reproj_px; every case asserts that none is within 1e-9 px of it
(both sides compute it in fp64 with +, *, / alone in one operand order, so
they should not differ at all; 1e-9 px is four orders above an ulp of a pixel
coordinate of a thousand)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import map_window_ref, oracle_lib
from tests import point_cull_ref as ref
from tests import pose_refine_ref

K_KITTI = (718.856, 718.856, 607.19, 185.22)
K_WHOLE = (700.0, 700.0, 600.0, 180.0)  # cx, cy whole: the optical axis projects exactly there
IDENT = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
XI_TRUE = [0.3, -0.1, 0.5, 0.01, 0.03, -0.02]
CULL = (4, 3, 2.0, 50)  # interval, max_fail_run, reproj_px, min_points
# the wave (64), the update's block (256) and the compaction round (1024) +- 1,
# unequal rounds, the capacity
STAGE_N = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 16384)
BAR = 1e-10


def _zeros(n):
    return np.zeros((n, 4), np.int32)


def _dist(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


# ------------------------------------------------------------------ CPU: known answers
def _axis_rows(ua, pk, sc, P=None, tracks=None, reproj=2.0):
    n = len(ua)
    P = np.tile([[0.0, 0.0, 10.0]], (n, 1)) if P is None else np.asarray(P, np.float64)
    tracks = _zeros(n) if tracks is None else tracks
    return ref.update(tracks, P, pk, sc, ua, IDENT, K_WHOLE, reproj)


def test_a_point_never_paired_ages_only():
    tr = _zeros(1)
    for k in range(5):
        r = _axis_rows([[600.0, 180.0]], [-1], [1], tracks=tr)
        tr = r["tracks"]
        assert r["counts"] == [0, 0, 0, 0]
    assert tr.tolist() == [[5, 0, 0, 0]]


def test_good_failed_and_behind_camera_rows():
    P = [[0, 0, 10.0], [0, 0, 10.0], [0, 0, 10.0], [0, 0, -10.0], [0, 0, 0.0], [0, 0, 10.0]]
    ua = [[601.0, 181.0], [601.0, 181.0], [603.0, 180.0], [600.0, 180.0], [600.0, 180.0], [0.0, 0.0]]
    pk = [0, 0, 2, 0, 0, -1]
    sc = [1, 0, 1, 1, 1, 1]
    start = np.array([[7, 5, 4, 0], [7, 5, 4, 1], [7, 5, 4, 2], [7, 5, 4, 0], [7, 5, 4, 0], [7, 5, 4, 2]], np.int32)
    r = _axis_rows(ua, pk, sc, P, start.copy())
    assert r["tracks"].tolist() == [[8, 6, 5, 0],   # good
                                    [8, 6, 4, 2],   # the alignment failed
                                    [8, 6, 4, 3],   # 3 px away
                                    [8, 6, 4, 1],   # behind the camera
                                    [8, 6, 4, 1],   # z == 0 is not in front
                                    [8, 5, 4, 2]]   # not paired
    assert r["counts"] == [5, 1, 4, 3]
    assert list(r["good"]) == [True, False, False, False, False, False]


def test_a_run_is_reset_by_one_good_frame():
    tr = _zeros(1)
    runs = []
    for ok in (0, 0, 1, 0, 0, 0):
        tr = _axis_rows([[600.5, 180.0]], [0], [ok], tracks=tr)["tracks"]
        runs.append(int(tr[0, 3]))
    assert runs == [1, 2, 0, 1, 2, 3] and tr.tolist() == [[6, 6, 1, 3]]


def test_the_exact_threshold():
    """Identity pose, P on the optical axis: the projection is exactly (cx,
    cy), so e2 is exactly 4 at cx + 2 and above it one step of 2^-30 further."""
    u, v, z = ref.project([[0.0, 0.0, 10.0]], IDENT, K_WHOLE)
    assert u[0] == 600.0 and v[0] == 180.0 and z[0] == 10.0
    r = _axis_rows([[602.0, 180.0], [602.0 + 2.0 ** -30, 180.0]], [0, 0], [1, 1])
    assert list(r["good"]) == [True, False]
    assert r["e"][0] == 2.0 and r["counts"] == [2, 1, 1, 1]


def _hand_map(fail_runs):
    n = len(fail_runs)
    pts = np.arange(3 * n, dtype=np.float64).reshape(n, 3)
    host = (np.arange(n) % 3).astype(np.int32)
    tr = np.stack([np.arange(n) + 10, np.arange(n) + 5, np.arange(n), fail_runs], 1).astype(np.int32)
    return pts, host, tr


def test_survivors_keep_their_order_and_their_rows():
    pts, host, tr = _hand_map([0, 3, 1, 5, 2, 3, 0])
    c = ref.cull(pts, host, tr, 3, 1)
    assert list(c["keep"]) == [1, 0, 1, 0, 1, 0, 1] and c["counts"] == [3, 4, 4, 0] and c["applied"]
    for k in ("points", "host", "tracks"):
        src = {"points": pts, "host": host, "tracks": tr}[k]
        assert np.array_equal(c[k], src[[0, 2, 4, 6]])


def test_abandonment_at_min_points():
    pts, host, tr = _hand_map([0, 3, 1, 5, 2, 3, 0])
    c = ref.cull(pts, host, tr, 3, 5)  # survivors == min_points - 1
    assert c["counts"] == [3, 4, 7, 1] and not c["applied"] and c["keep"].all()
    assert np.array_equal(c["points"], pts) and np.array_equal(c["tracks"], tr) and np.array_equal(c["host"], host)
    c = ref.cull(pts, host, tr, 3, 4)  # survivors == min_points
    assert c["counts"] == [3, 4, 4, 0] and c["applied"]
    # no candidates: nothing happens, whatever min_points
    c = ref.cull(pts, host, tr, 6, 100)
    assert c["counts"] == [0, 7, 7, 0] and not c["applied"] and c["keep"].all()


# ------------------------------------------------------------------ CPU: the parity cases
@functools.lru_cache(maxsize=None)
def _case(n, seed=0, max_fail=3, reproj=2.0):
    """Points in front of (rows i % 7 == 6: behind) the camera at T; rows
    i % 7 == 0 have no pair, 1 a failed alignment, 2-4 land within 1.9 px of
    their projection, 5 lands 2.1-10 px away; incoming records random, the
    fail_run also at max_fail - 1 and at max_fail."""
    rng = np.random.default_rng(1000 * seed + n)
    T = np.array(pose_refine_ref.left_update(XI_TRUE, IDENT))
    R, t = T[:9].reshape(3, 3), T[9:]
    i = np.arange(n)
    Pc = np.stack([rng.uniform(-15, 15, n), rng.uniform(-4, 4, n), rng.uniform(5, 60, n)], 1)
    Pc[i % 7 == 6, 2] *= -1.0
    P = (Pc - t) @ R
    u, v, z = ref.project(P, T, K_KITTI)
    rad = np.where(i % 7 == 5, rng.uniform(2.1, 10.0, n), rng.uniform(0.0, 1.9, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    ua = np.stack([np.where(z > 0, u, 0.0) + rad * np.cos(ang), np.where(z > 0, v, 0.0) + rad * np.sin(ang)], 1)
    pk = np.where(i % 7 == 0, -1, rng.integers(0, 4, n)).astype(np.int32)
    sc = np.where(i % 7 == 1, 0, 1).astype(np.uint8)
    age = rng.integers(0, 100, n)
    seen = (age * rng.uniform(0, 1, n)).astype(np.int64)
    found = (seen * rng.uniform(0, 1, n)).astype(np.int64)
    run = rng.choice([0, 1, max_fail - 1, max_fail, max_fail + 2], n)
    tr = np.stack([age, seen, found, run], 1).astype(np.int32)
    host = rng.integers(0, 4, n).astype(np.int32)
    s = {"P": P, "pk": pk, "sc": sc, "ua": ua, "T": T, "tracks": tr, "host": host, "max_fail": max_fail,
         "reproj": reproj}
    s["upd"] = ref.update(tr, P, pk, sc, ua, T, K_KITTI, reproj)
    for a in (P, pk, sc, ua, tr, host, s["upd"]["tracks"]):
        a.setflags(write=False)
    return s


def test_parity_cases_exercise_every_row_kind_clear_of_the_threshold():
    for n in STAGE_N:
        s = _case(n)
        r = s["upd"]
        print("n", n, "counts", r["counts"], "margin", r["margin"])
        assert r["margin"] > 1e-9, n
        if n >= 63:
            i = np.arange(n)
            assert r["counts"][0] == int((i % 7 != 0).sum())
            assert r["good"][(i % 7 >= 2) & (i % 7 <= 4)].all() and not r["good"][(i % 7 < 2) | (i % 7 > 4)].any()
            before, after = s["tracks"][:, 3], r["tracks"][:, 3]
            # a run reaching max_fail on this frame, and one reset from it
            assert ((before == s["max_fail"] - 1) & (after == s["max_fail"])).any()
            assert ((before >= s["max_fail"]) & (after == 0)).any()
            c = ref.cull(s["P"], s["host"], r["tracks"], s["max_fail"], n // 4)
            assert c["applied"] and 0 < c["counts"][0] < n
            assert ref.cull(s["P"], s["host"], r["tracks"], s["max_fail"], n)["counts"][3] == 1


# ------------------------------------------------------------------ CPU: the oracle's pipeline
W, H = 416, 128  # the smallest synthetic size whose stereo initialisation makes a map (328 points)
N_PIPE = 13      # the stereo frame and 12 tracking frames


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


def test_the_oracle_pipeline_has_points_to_cull():
    """The oracle's pipeline alone (stereo initialisation, then left images,
    its frozen map): the restatement's first cull, at tracking frame 4,
    removes points and is not abandoned."""
    seq = _seq()
    ov = oracle_lib.Viso(seq.K, W, H, enable_tracking=1)
    ov.set_stereo(seq.p.baseline, 128, 1)
    ov.on_new_stereo(_image(0), _image(0, 1))
    assert ov.state == 1
    pts = ov.points()
    tr = _zeros(len(pts))
    interval, max_fail, reproj, min_points = CULL
    for f in range(1, interval + 1):
        ov.on_new_frame(_image(f))
        pk, sc, ub, ua = ov.alignment()
        u = ref.update(tr, pts, pk, sc, ua, ov.poses()[-1], seq.K, reproj)
        print("frame", f, "counts", u["counts"], "margin", u["margin"])
        assert u["margin"] > 1e-9
        tr = u["tracks"]
    c = ref.cull(pts, np.zeros(len(pts), np.int32), tr, max_fail, min_points)
    print("map", len(pts), "cull counts", c["counts"])
    assert c["applied"] and c["counts"][0] >= 1 and c["counts"][3] == 0 and c["counts"][2] == len(pts) - c["counts"][0]


# ------------------------------------------------------------------ CPU: the ABI
def test_abi_exports_and_null_context():
    from viso_amd import _lib
    lib = _lib.load()
    for name in ("viso_set_point_cull", "viso_get_point_cull", "viso_get_point_tracks", "viso_point_tracks_update",
                 "viso_points_cull"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert _lib.KERNEL_IDS["cull"] == 11
    n = ctypes.c_size_t(0)
    info = (ctypes.c_int64 * 8)()
    cnt = (ctypes.c_int32 * 4)()
    pose = np.ascontiguousarray(IDENT)
    assert lib.viso_set_point_cull(None, 4, 3, 2.0, 50) == -1
    assert lib.viso_get_point_cull(None, info) == -1
    assert lib.viso_get_point_tracks(None, None, 0, ctypes.byref(n)) == -1
    assert lib.viso_point_tracks_update(None, None, None, None, None, 0, pose.ctypes.data, 2.0, None, cnt) == -1
    assert lib.viso_points_cull(None, None, None, None, 0, 3, 0, None, None, None, None, ctypes.byref(n), cnt) == -1


# ------------------------------------------------------------------ GPU: the stage entries
@functools.lru_cache(maxsize=None)
def _ctx(K=K_KITTI):
    from viso_amd import api
    fx, fy, cx, cy = K
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=1242, height=375))


def _same_cull(g, c):
    print("gpu", g["counts"], g["n"], "ref", c["counts"])
    assert g["counts"] == c["counts"] and g["n"] == c["counts"][2]
    assert np.array_equal(g["keep"], c["keep"])
    assert np.array_equal(g["points"], c["points"])  # copies: bit-equal
    assert np.array_equal(g["host"], c["host"])
    assert np.array_equal(g["tracks"], c["tracks"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", STAGE_N)
def test_gpu_stage_entries_match_restatement(n):
    s = _case(n)
    r = s["upd"]
    tracks, counts = _ctx().point_tracks_update(s["P"], s["pk"], s["sc"], s["ua"], s["T"], s["tracks"], s["reproj"])
    print("n", n, "gpu", counts, "ref", r["counts"], "margin", r["margin"])
    assert counts == r["counts"]
    assert np.array_equal(tracks, r["tracks"])
    # the cull of the updated records: applied, abandoned, and without candidates
    for max_fail, min_points in ((s["max_fail"], n // 4), (s["max_fail"], n), (1000, 1)):
        c = ref.cull(s["P"], s["host"], r["tracks"], max_fail, min_points)
        _same_cull(_ctx().cull_points(s["P"], s["host"], r["tracks"], max_fail, min_points), c)


@pytest.mark.gpu
def test_gpu_stage_crafted_cases():
    ctx = _ctx(K_WHOLE)
    # the exact threshold
    P = np.tile([[0.0, 0.0, 10.0]], (2, 1))
    ua = np.array([[602.0, 180.0], [602.0 + 2.0 ** -30, 180.0]])
    tracks, counts = ctx.point_tracks_update(P, [0, 0], [1, 1], ua, IDENT, _zeros(2), 2.0)
    assert tracks.tolist() == [[1, 1, 1, 0], [1, 1, 0, 1]] and counts == [2, 1, 1, 1]
    # the known answers of the restatement
    P = [[0, 0, 10.0], [0, 0, 10.0], [0, 0, 10.0], [0, 0, -10.0], [0, 0, 0.0], [0, 0, 10.0]]
    ua = [[601.0, 181.0], [601.0, 181.0], [603.0, 180.0], [600.0, 180.0], [600.0, 180.0], [0.0, 0.0]]
    start = np.array([[7, 5, 4, 0], [7, 5, 4, 1], [7, 5, 4, 2], [7, 5, 4, 0], [7, 5, 4, 0], [7, 5, 4, 2]], np.int32)
    tracks, counts = ctx.point_tracks_update(P, [0, 0, 2, 0, 0, -1], [1, 0, 1, 1, 1, 1], ua, IDENT, start, 2.0)
    assert tracks.tolist() == [[8, 6, 5, 0], [8, 6, 4, 2], [8, 6, 4, 3], [8, 6, 4, 1], [8, 6, 4, 1], [8, 5, 4, 2]]
    assert counts == [5, 1, 4, 3]
    # every point a candidate: an empty map with min_points 0, abandoned with 1
    n = 1500
    pts, host, tr = _hand_map(np.full(n, 3))
    g = ctx.cull_points(pts, host, tr, 3, 0)
    _same_cull(g, ref.cull(pts, host, tr, 3, 0))
    assert g["n"] == 0 and g["counts"] == [n, 0, 0, 0] and not g["keep"].any()
    g = ctx.cull_points(pts, host, tr, 3, 1)
    _same_cull(g, ref.cull(pts, host, tr, 3, 1))
    assert g["n"] == n and g["counts"] == [n, 0, n, 1] and g["keep"].all()
    assert np.array_equal(g["points"], pts) and np.array_equal(g["tracks"], tr) and np.array_equal(g["host"], host)
    # no candidates
    g = ctx.cull_points(pts, host, tr, 4, 1)
    assert g["n"] == n and g["counts"] == [0, n, n, 0] and g["keep"].all() and np.array_equal(g["points"], pts)
    # candidates in the last, partial round only
    n = 1024 + 37
    runs = np.zeros(n, np.int64)
    runs[[1024, 1030, n - 1]] = 3
    pts, host, tr = _hand_map(runs)
    g = ctx.cull_points(pts, host, tr, 3, 50)
    _same_cull(g, ref.cull(pts, host, tr, 3, 50))
    assert g["n"] == n - 3 and g["keep"][:1024].all() and np.array_equal(g["points"][:1024], pts[:1024])
    # abandonment at survivors == min_points - 1, application at survivors == min_points
    assert ctx.cull_points(pts, host, tr, 3, n - 2)["counts"] == [3, n - 3, n, 1]
    assert ctx.cull_points(pts, host, tr, 3, n - 3)["counts"] == [3, n - 3, n - 3, 0]


@pytest.mark.gpu
def test_gpu_stage_argument_codes():
    from viso_amd import _lib
    lib, h = _lib.load(), _ctx().h
    P, pk, sc, ua = np.zeros((2, 3)), np.zeros(2, np.int32), np.ones(2, np.uint8), np.zeros((2, 2))
    P[:, 2] = 10.0
    T, tr, cnt = np.ascontiguousarray(IDENT), _zeros(2), np.zeros(4, np.int32)
    host, out, oh, ot, keep = np.zeros(2, np.int32), np.zeros((2, 3)), np.zeros(2, np.int32), _zeros(2), np.zeros(2, np.uint8)
    m = ctypes.c_size_t(0)

    def p(a):
        return None if a is None else a.ctypes.data

    def upd(n=2, pts=P, pair=pk, succ=sc, uv=ua, pose=T, reproj=2.0, t=tr, c=cnt):
        return lib.viso_point_tracks_update(h, p(pts), p(pair), p(succ), p(uv), n, p(pose), reproj, p(t), p(c))

    assert upd() == 0 and upd(n=0, pts=None, pair=None, succ=None, uv=None, t=None) == 0
    for kw in ({"n": -1}, {"n": 16385}, {"pts": None}, {"pair": None}, {"succ": None}, {"uv": None}, {"pose": None},
               {"reproj": 0.0}, {"reproj": -1.0}, {"reproj": float("nan")}, {"t": None}, {"c": None}):
        assert upd(**kw) == -1, kw

    def cull(n=2, pts=P, hst=host, t=tr, mf=3, mp=0, o=out, o_h=oh, o_t=ot, k=keep, n_out=m, c=cnt):
        return lib.viso_points_cull(h, p(pts), p(hst), p(t), n, mf, mp, p(o), p(o_h), p(o_t), p(k),
                                    None if n_out is None else ctypes.byref(n_out), p(c))

    assert cull() == 0 and cull(mf=1000, mp=16384) == 0
    assert cull(n=0, pts=None, hst=None, t=None, o=None, o_h=None, o_t=None, k=None) == 0 and m.value == 0
    for kw in ({"n": -1}, {"n": 16385}, {"pts": None}, {"hst": None}, {"t": None}, {"mf": 0}, {"mf": 1001},
               {"mp": -1}, {"mp": 16385}, {"o": None}, {"o_h": None}, {"o_t": None}, {"k": None}, {"n_out": None},
               {"c": None}):
        assert cull(**kw) == -1, kw


# ------------------------------------------------------------------ GPU: the pipeline
def _viso(cull=CULL, refine=None, mono=None, window=None, ba=0):
    import viso_amd
    seq = _seq()
    gv = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32)
    gv.set_stereo(seq.p.baseline, 128, 1)
    if cull is not None:
        gv.set_point_cull(*cull)
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


@functools.lru_cache(maxsize=None)
def _ctx_seq():
    """A context of the sequence's size and intrinsics, for stage entries."""
    from viso_amd import api
    fx, fy, cx, cy = _seq().K
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=W, height=H))


def _snap(gv, tracks=True):
    return {"points": gv.GetPoints(), "hosts": gv.point_hosts(), "info": gv.point_cull(),
            "tracks": gv.point_tracks() if tracks else None}


def _step(gv, f):
    gv.OnNewFrame(_image(f))
    s = _snap(gv)
    s["pose"] = gv.poses[-1]
    s["row"] = gv.alignment()
    return s


class _Model:
    """The restatement carried along a run: fed the GPU's own LK row and pose
    after every frame."""

    def __init__(self, points, hosts, cull=CULL):
        self.points, self.hosts, self.tracks = points, hosts, _zeros(len(points))
        self.interval, self.max_fail, self.reproj, self.min_points = cull
        self.applied = self.removed = self.abandoned = 0
        self.last = [-1, 0, 0]
        self.margin = float("inf")

    def frame(self, t, row, pose, frames):
        """Tracking frame t (frames: the frames processed before it).  Returns
        the cull's result on a cull frame."""
        pk, sc, ub, ua = row
        assert len(pk) == len(self.points)
        u = ref.update(self.tracks, self.points, pk, sc, ua, pose, _seq().K, self.reproj)
        self.margin = min(self.margin, u["margin"])
        self.tracks = u["tracks"]
        if t % self.interval:
            return None
        c = ref.cull(self.points, self.hosts, self.tracks, self.max_fail, self.min_points)
        self.abandoned += c["counts"][3]
        if c["applied"]:
            self.applied += 1
            self.removed += len(self.points) - c["counts"][2]
            self.last = [frames, len(self.points) - c["counts"][2], c["counts"][2]]
            self.points, self.hosts, self.tracks = c["points"], c["host"], c["tracks"]
        return c

    def info(self):
        return [self.interval, self.max_fail, self.applied, self.removed, self.abandoned] + self.last


_runs = {}


def _pipeline(batched):
    if batched not in _runs:
        gv = _viso()
        first = _snap(gv)
        gv.ctx.timing_enable(True)
        snaps = {}
        if batched:
            import torch
            dl = torch.from_numpy(np.stack([_image(f) for f in range(1, N_PIPE)])).cuda()
            torch.cuda.synchronize()
            gv.process_device(dl.data_ptr(), None, N_PIPE - 1, W * H)
            gv.synchronize()
        else:
            for f in range(1, N_PIPE):
                snaps[f] = _step(gv, f)
        _runs[batched] = {"first": first, "snaps": snaps, "final": _snap(gv), "poses": gv.poses,
                          "launches": gv.ctx.timing("cull")[0]}
        gv.close()
    return _runs[batched]


@pytest.mark.gpu
def test_gpu_pipeline_matches_restatement():
    res = _pipeline(False)
    first, snaps = res["first"], res["snaps"]
    assert len(first["points"]) > 50 and not first["tracks"].any() and list(first["info"]) == [4, 3, 0, 0, 0, -1, 0, 0]
    K = _seq().K
    m = _Model(first["points"], first["hosts"])
    after_cull = None
    culls = []
    for f in range(1, N_PIPE):
        s = snaps[f]
        if after_cull is not None:
            # the frame after an applied cull tracks and aligns against the culled map
            prev = snaps[f - 1]["pose"]
            exp = oracle_lib.direct_pose(_pyr(f - 1), _pyr(f), W, H, K, m.points, prev, prev)
            d = _dist(s["pose"], exp)
            pk, sc, ub, ua = s["row"]
            o = oracle_lib.lk_align([_pyr(0)], [IDENT], _pyr(f), s["pose"], W, H, K, m.points)
            print("frame", f, "after the cull: pose relative difference", d, "row", len(pk), "uv_after difference",
                  np.abs(ua - o[3]).max())
            assert d < BAR
            assert len(pk) == len(m.points) == after_cull
            assert np.array_equal(pk, o[0]) and np.array_equal(sc, o[1]) and np.array_equal(ua, o[3])
            after_cull = None
        c = m.frame(f, s["row"], s["pose"], f)
        assert np.array_equal(s["tracks"], m.tracks), f
        assert len(s["points"]) == len(m.points)
        assert list(s["info"]) == m.info(), f
        if c is not None:
            print("frame", f, "cull", c["counts"], "map", len(m.points), "info", list(s["info"]))
            assert np.array_equal(s["points"], m.points) and np.array_equal(s["hosts"], m.hosts)
            if c["applied"]:
                culls.append(f)
                after_cull = len(m.points)
    print("culls applied at", culls, "smallest | e - reproj_px |", m.margin)
    assert m.margin > 1e-9
    assert culls and culls[0] == 4
    # one update launch a frame, one cull launch a cull frame
    assert res["launches"] == (N_PIPE - 1) + (N_PIPE - 1) // CULL[0]


@pytest.mark.gpu
def test_gpu_pipeline_ingest_forms_agree():
    a, b = _pipeline(False), _pipeline(True)
    assert np.array_equal(a["poses"], b["poses"])
    for k in ("points", "hosts", "tracks", "info"):
        assert np.array_equal(a["final"][k], b["final"][k]), k
    assert a["launches"] == b["launches"]


@pytest.mark.gpu
def test_gpu_off_is_off():
    from viso_amd import _lib
    runs = []
    for setter in (False, True):
        gv = _viso(cull=None)
        cfg = gv.config()
        gv.ctx.timing_enable(True)
        if setter:
            gv.set_point_cull(0)
            assert gv.config() == cfg
        for f in range(1, 10):
            gv.OnNewFrame(_image(f))
        n = ctypes.c_size_t(0)
        assert _lib.load().viso_get_point_tracks(gv.ctx.h, None, 0, ctypes.byref(n)) == -4
        assert gv.ctx.timing("cull")[0] == 0
        assert list(gv.point_cull()) == [0, 0, 0, 0, 0, -1, 0, 0]
        runs.append((gv.poses, gv.GetPoints(), gv.point_hosts()))
        gv.close()
    assert len(runs[0][0]) == 9
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    # and on, the map shrinks
    assert len(_pipeline(False)["final"]["points"]) < len(runs[0][1])


@pytest.mark.gpu
def test_gpu_records_follow_the_refined_pose():
    gv = _viso(refine=(5, 1.0, 8.0))
    first = _snap(gv)
    m = _Model(first["points"], first["hosts"])
    for f in range(1, 9):
        s = _step(gv, f)
        assert gv.pose_refine()[0] > 0  # the frame was refined: viso_get_poses is the refined pose
        m.frame(f, s["row"], s["pose"], f)
        assert np.array_equal(s["tracks"], m.tracks), f
        assert np.array_equal(s["points"], m.points) and list(s["info"]) == m.info()
    gv.close()
    print("culls", m.info(), "margin", m.margin)
    assert m.margin > 1e-9 and m.applied >= 1


@pytest.mark.gpu
def test_gpu_setter_codes_and_setting_while_tracking():
    from viso_amd import _lib
    gv = _viso(cull=None)
    lib, h = _lib.load(), gv.ctx.h
    for args in ((-1, 3, 2.0, 50), (4, 0, 2.0, 50), (4, 1001, 2.0, 50), (4, 3, 0.0, 50), (4, 3, -2.0, 50),
                 (4, 3, float("nan"), 50), (4, 3, 2.0, 0), (4, 3, 2.0, 16385)):
        assert lib.viso_set_point_cull(h, *args) == -1, args
    for args in ((1, 1, 0.5, 1), (1000, 1000, 100.0, 16384), (0, 0, 0.0, 0)):
        assert lib.viso_set_point_cull(h, *args) == 0, args
    n = ctypes.c_size_t(0)
    for f in range(1, 6):
        gv.OnNewFrame(_image(f))
    assert lib.viso_get_point_tracks(h, None, 0, ctypes.byref(n)) == -4
    gv.set_point_cull(*CULL)  # while tracking: frame 6 is the first counted
    assert not gv.point_tracks().any()
    first = _snap(gv)
    m = _Model(first["points"], first["hosts"])
    for f in range(6, 9):
        s = _step(gv, f)
        m.frame(f, s["row"], s["pose"], f)  # (tracking frame 8 is a cull frame: the count runs from the map's creation)
        assert (s["tracks"][:, 0] == f - 5).all() and np.array_equal(s["tracks"], m.tracks), f
        assert np.array_equal(s["points"], m.points) and list(s["info"]) == m.info()
    gv.set_point_cull(0)
    assert lib.viso_get_point_tracks(h, None, 0, ctypes.byref(n)) == -4
    gv.OnNewFrame(_image(9))
    gv.set_point_cull(*CULL)  # on again: zeroed again
    assert not gv.point_tracks().any()
    gv.OnNewFrame(_image(10))
    assert (gv.point_tracks()[:, 0] == 1).all()
    gv.close()


@pytest.mark.gpu
def test_gpu_composes_with_insertion_window_and_ba():
    """Monocular insertion every 5th frame (8-pixel cells, 0.1 degrees), a
    window of 2 keyframes, the BA behind every insertion, a cull every 4th
    frame, over 20 tracking frames (frame 20 is both a cull and a check
    frame).  The records are carried by the restatement across culls,
    retirements (the keep flags of tests/map_window_ref.py) and insertions
    (zero rows); the coordinates are read back each frame, as the BA moves
    them."""
    n = 21
    mono, cell = (5, 1000, 8, 0.1), 16
    gv = _viso(mono=mono, window=(2, cell), ba=2)
    K = _seq().K
    s0 = _snap(gv)
    tracks, hosts = _zeros(len(s0["points"])), s0["hosts"]
    kf_frames = [0]
    events = []
    for f in range(1, n):
        b = _snap(gv)
        b["kf"], b["win"] = gv.keyframe_poses(), gv.map_window()
        assert len(b["tracks"]) == len(b["points"]) == len(b["hosts"])
        s = _step(gv, f)
        a_kf, a_win, st = gv.keyframe_poses(), gv.map_window(), gv.stats()
        # the update, then the cull of a cull frame
        m = _Model(b["points"], hosts)
        m.tracks = tracks
        c = m.frame(f, s["row"], s["pose"], f)
        assert m.margin > 1e-9
        pts, hosts, tracks = m.points, m.hosts, m.tracks
        culled = c is not None and c["applied"]
        # the retirement of a check frame, on the culled map
        retired = a_win[2] > b["win"][2]
        if retired:
            r = map_window_ref.retire(pts, hosts, s["pose"], b["kf"], K, W, H, cell)
            assert r["margin"] > 1e-9
            keep = r["keep"].astype(bool)
            pts, hosts, tracks = r["points"], r["host"], tracks[keep]
            kf_frames = kf_frames[1:]
        # the insertion: zero rows behind the kept ones, hosted by the new keyframe
        added = len(s["points"]) - len(pts)
        assert added >= 0 and st[14] == added
        if added:
            kf_frames = kf_frames + [f]
            # the occupancy the insertion saw is that of the map the cull (and the retirement) left
            kfp = b["kf"][1:] if retired else b["kf"]
            g = _ctx_seq().mono_points(_pyr(f), _pyr(kf_frames[-2]), W, H, s["pose"], kfp[-1], pts, mono[2], mono[3])
            assert g["n"] == added, (f, g["n"], added)
            hosts = np.concatenate([hosts, np.full(added, len(a_kf) - 1, np.int32)])
            tracks = np.vstack([tracks, _zeros(added)])
        events.append((f, culled, c["counts"] if c is not None else None, retired, added, len(s["points"])))
        assert np.array_equal(s["tracks"], tracks), f
        assert np.array_equal(s["hosts"], hosts), f
        if not added:  # (the BA follows an insertion only)
            assert np.array_equal(s["points"], pts), f
    poses = gv.poses
    info = gv.point_cull()
    gv.close()
    for e in events:
        print("frame %2d culled %d counts %s retired %d added %3d map %4d" % e)
    print("info", list(info))
    assert len(poses) == n - 1 and np.isfinite(poses).all()
    assert sum(1 for e in events if e[4]) >= 2 and any(e[3] for e in events)
    assert info[2] == sum(1 for e in events if e[1]) and info[2] >= 1
