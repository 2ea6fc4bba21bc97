"""Point refinement (viso_set_point_refine / viso_point_obs_record /
viso_points_refine, include/viso/viso_c.h; DESIGN.md §Point refinement): every
map point's depth along its anchor keyframe's ray is refined on the LK-aligned
positions of the last frames.  The repo's own spec, restated in
tests/point_refine_ref.py; the reference computes the aligned positions
(src/viso.cpp:768-843) and only draws them.

GPU vs the restatement: status, steps, counts and flags equal, the points
within 1e-10 relative (the bar of tests/test_pipeline.py), the costs within
1e-9 relative.  Both sides compute in fp64 with +, -, *, / and sqrt alone (all
correctly rounded) in one operand order and one order of the sums, so they
should not differ at all; what was seen is in DESIGN.md §Point refinement.  A
decision could differ only where its quantity sits on its threshold; the
parity cases assert that none is within 1e-9 of it (relative for the cost
comparison and the parallax test).

The parity cases start at 0.6 or 1.7 of the true depth, 4 to 14 m, with frames
driven 3 to 6 m forward and sideways: the projection is far from linear in the
inverse depth, so the three passes the cases run are still descending.  The
cost comparison of a pass is a difference that takes either sign over the
points, so among 16384 of them one comes within 1e-10 relative of zero by
chance: the two largest cases use the first seed whose restatement keeps every
decision 1e-9 clear (SEEDS; test_parity_cases_are_clear_of_every_threshold
prints the margins)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import oracle_lib
from tests import point_cull_ref
from tests import point_refine_ref as ref
from tests import pose_refine_ref

K_KITTI = (718.856, 718.856, 607.19, 185.22)
K_WHOLE = (700.0, 700.0, 600.0, 180.0)  # cx, cy whole: the optical axis projects exactly there
IDENT = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
# a point's 8 lanes, the wave's 8 points (64 lanes), the block's 32 points
# (256 lanes) +- 1, more than one block, the capacity
STAGE_N = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2049, 16384)
STAGE_M = (1, 2, 3, 7, 8)
BAR = 1e-10
EPS = 2.0 ** -52


def _dist(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _pose(t, R=None):
    return np.concatenate([np.eye(3).ravel() if R is None else np.asarray(R, np.float64).ravel(),
                           np.asarray(t, np.float64)])


def _project(P, T, K):
    u, v, z = point_cull_ref.project(P, T, K)
    return np.stack([u, v], 1), z


# ------------------------------------------------------------------ CPU: known answers
def _axis(Z, frames, uv, K=K_WHOLE, anchor=0, flags=None, iterations=1, huber=100.0, min_obs=1, sigma=1.0):
    """One point on the identity anchor's optical axis at depth Z, one
    observation per frame."""
    m = len(frames)
    flags = np.ones((m, 1), np.uint8) if flags is None else np.asarray(flags, np.uint8).reshape(m, 1)
    return dict(points=[[0.0, 0.0, Z]], anchor_kf=[anchor], kf_poses=[IDENT], frame_poses=frames, obs_valid=flags,
                obs_uv=np.asarray(uv, np.float64).reshape(m, 1, 2), iterations=iterations, huber_px=huber,
                min_obs=min_obs, max_rel_sigma=sigma)


SIDE = _pose([-1.0, 0.0, 0.0])  # the camera one metre to the right of the anchor

# name -> (arguments, expected status, steps): the crafted cases, also run on the device
CRAFTED = {
    # Z = 8 seen where depth 10 projects: r0 = 17.5, g0 = -87.5, delta = b / H = -0.2
    "first_step": (_axis(8.0, [SIDE], [[530.0, 180.0]]), 0, 1),
    "no_anchor": (_axis(8.0, [SIDE], [[530.0, 180.0]], anchor=-1), 5, 0),
    "one_flag_short": (_axis(8.0, [SIDE] * 3, [[530.0, 180.0]] * 3, flags=[1, 0, 1], min_obs=3), 1, 0),
    # the camera moved along the ray: D parallel to the translation, g = 0, H = 0
    "on_the_baseline": (_axis(8.0, [_pose([0.0, 0.0, -1.0])], [[600.0, 180.0]]), 4, 0),
    # depth 4 seen from depth 8: delta = 1, 1 + delta = 2 is not below 2
    "step_too_long": (_axis(8.0, [SIDE], [[425.0, 180.0]]), 2, 0),
    # depth 16 seen from depth 8: delta = -0.5, 1 + delta = 0.5 is not above 0.5
    "step_too_short": (_axis(8.0, [SIDE], [[556.25, 180.0]]), 2, 0),
    # the second frame has z = -1 at depth 8 and z = 1 at depth 10, where it
    # sees the point 3 px off: pass 0 uses the first frame alone
    "behind_in_pass_0": (_axis(8.0, [SIDE, _pose([-1.0, 0.0, -9.0])], [[530.0, 180.0], [-100.0, 183.0]]), 0, 1),
}


def _run(case):
    return ref.refine(K=K_WHOLE, **case)


def test_first_step_by_hand():
    r = _run(CRAFTED["first_step"][0])
    # H = 87.5^2, b = -87.5 * 17.5, cost_0 = 17.5^2 / 2
    assert r["delta0"][0] == (-87.5 * 17.5) / (87.5 * 87.5) and abs(r["delta0"][0] + 0.2) <= EPS
    assert r["costs"][0, 0] == 153.125
    assert r["status"][0] == 0 and r["steps"][0] == 1 and r["counts"] == [1, 1, 0, 0]
    P = r["points"][0]
    assert P[0] == 0.0 and P[1] == 0.0 and abs(P[2] - 10.0) <= 4 * 10.0 * EPS
    assert r["costs"][0, 1] < 1e-20
    # with more passes: the cost is zero at depth 10 and cannot fall again
    r = _run(dict(CRAFTED["first_step"][0], iterations=4))
    assert abs(r["points"][0, 2] - 10.0) <= 4 * 10.0 * EPS and r["steps"][0] >= 1


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_crafted_statuses(name):
    case, status, steps = CRAFTED[name]
    r = _run(case)
    print(name, r["status"], r["steps"], r["costs"], r["points"], r["delta0"])
    assert r["status"][0] == status and r["steps"][0] == steps
    if steps == 0:
        assert np.array_equal(r["points"], np.asarray(case["points"]))  # unchanged, bit-equal
    if name == "no_anchor":
        assert r["counts"] == [0, 0, 0, 0] and not r["costs"].any()
    if name == "one_flag_short":
        assert r["counts"] == [0, 0, 0, 0]
        full = _run(dict(case, obs_valid=np.ones((3, 1), np.uint8)))
        assert full["status"][0] == 0 and full["counts"][0] == 1
    if name == "on_the_baseline":
        assert r["counts"] == [1, 0, 1, 0]
    if name == "step_too_long":
        assert r["delta0"][0] == 1.0 and r["counts"] == [1, 0, 0, 1]
    if name == "step_too_short":
        assert r["delta0"][0] == -0.5
    if name == "behind_in_pass_0":
        # pass 0: the first frame alone (17.5^2 / 2); pass 1: the second frame's 3 px
        assert r["costs"][0, 0] == 153.125 and abs(r["costs"][0, 1] - 4.5) < 1e-9


def test_the_cost_that_stops_falling_returns_the_previous_point():
    """Status 3 points of a parity case: the result is the point after
    `steps` updates, which a run of `steps` passes ends on with status 0."""
    s = _case(2049, 8)
    r = s["ref"]
    idx = np.nonzero(r["status"] == 3)[0]
    assert len(idx) >= 3
    seen = set()
    for i in idx[:40]:
        k = int(r["steps"][i])
        seen.add(k)
        one = {key: (s[key][i:i + 1] if key in ("points", "anchor_kf") else
                     s[key][:, i:i + 1] if key in ("obs_valid", "obs_uv") else s[key]) for key in ARGS}
        if k == 0:
            assert np.array_equal(r["points"][i], s["points"][i])
            continue
        q = ref.refine(K=K_KITTI, **dict(one, iterations=k))
        assert q["status"][0] == 0 and q["steps"][0] == k
        assert np.array_equal(q["points"][0], r["points"][i])
        assert q["costs"][0, 1] == r["costs"][i, 1]
    print("status 3 at steps", sorted(seen))


def test_the_exact_shift_bound():
    ub = [[600.0, 180.0]] * 3
    ua = [[608.0, 180.0], [608.0 + 2.0 ** -30, 180.0], [600.0, 172.0]]
    v, uv, margin = ref.record([0, 0, 0], [1, 1, 1], ub, ua, 8.0)
    assert list(v) == [1, 0, 1] and np.array_equal(uv, np.asarray(ua)) and margin == 0.0
    v, _, _ = ref.record([-1, 0, 2], [1, 0, 1], ub, [[600.0, 180.0]] * 3, 8.0)
    assert list(v) == [0, 0, 1]


def _tree_case():
    """Eight frames at SIDE see the axis point at depth 8 (512.5, 180): the
    first 1.5 px off (Huber 1: rho = 1), the others 2^-26 px off (rho =
    2^-53, half an ulp of 1)."""
    uv = [[514.0, 180.0]] + [[512.5 + 2.0 ** -26, 180.0]] * 7
    return _axis(8.0, [SIDE] * 8, uv, huber=1.0)


def test_the_sums_are_the_tree():
    r = _run(_tree_case())
    u = 2.0 ** -53
    running = 1.0
    for _ in range(7):
        running = running + u
    tree = ((1.0 + u) + (u + u)) + ((u + u) + (u + u))
    assert running == 1.0 and tree == 1.0 + 3 * EPS
    assert r["costs"][0, 0] == tree
    v = np.array([[1.0]] + [[u]] * 7)
    assert ref.tree8(v)[0] == tree


# ------------------------------------------------------------------ CPU: convergence
def _ray_points(n, rng, K):
    z = rng.uniform(5.0, 40.0, n)
    u, v = rng.uniform(0.0, 1242.0, n), rng.uniform(0.0, 375.0, n)
    return np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)


@functools.lru_cache(maxsize=None)
def _convergence(forward):
    rng = np.random.default_rng(7)
    n, m = 2000, 5
    Pt = _ray_points(n, rng, K_KITTI)
    scale = np.where(rng.integers(0, 2, n) == 1, 1.1, 0.9)
    P = Pt * scale[:, None]  # along the identity anchor's ray
    d = rng.uniform(1.2, 2.4, m) * np.where(np.arange(m) % 2 == 1, -1.0, 1.0)
    # (Tcw: the camera at +d has t = -d)
    frames = [_pose([0.0, 0.0, -abs(x)]) if forward else _pose([-x, 0.0, 0.0]) for x in d]
    uv = np.stack([_project(Pt, T, K_KITTI)[0] for T in frames])
    r = ref.refine(P, np.zeros(n, np.int32), [IDENT], frames, np.ones((m, n), np.uint8), uv, K_KITTI, 4, 1.0, 3, 0.05)
    err = np.abs(r["points"][:, 2] - Pt[:, 2]) / Pt[:, 2]
    return P, Pt, r, err


def test_convergence_sideways():
    P, Pt, r, err = _convergence(False)
    print("statuses", np.bincount(r["status"], minlength=6), "steps", np.bincount(r["steps"]), "worst relative depth error",
          err.max())
    assert (r["steps"] >= 1).all()
    assert err.max() < 1e-9


def test_convergence_forward():
    P, Pt, r, err = _convergence(True)
    flat = r["status"] == 4
    print("statuses", np.bincount(r["status"], minlength=6), "rejected", flat.mean(), "worst relative depth error",
          err[~flat].max(), "95th percentile", np.percentile(err[~flat], 95))
    assert 20 < flat.sum() < len(flat) // 2  # (the points near the epipole)
    assert np.array_equal(r["points"][flat], P[flat])  # bit-equal
    assert (r["steps"][~flat] >= 1).all()
    assert err[~flat].max() < 1e-9


# ------------------------------------------------------------------ CPU: the parity cases
ARGS = ("points", "anchor_kf", "kf_poses", "frame_poses", "obs_valid", "obs_uv", "iterations", "huber_px", "min_obs",
        "max_rel_sigma")
PARITY_ITER, PARITY_HUBER, PARITY_SIGMA = 3, 1.0, 0.05
FWD, DEPTH, SCALE = (3.0, 6.0), (4.0, 14.0), (0.6, 1.7)
SEEDS = {(16384, 7): 9, (16384, 8): 2}  # (n, m) -> seed (0 elsewhere)


@functools.lru_cache(maxsize=None)
def _case(n, m, seed=None):
    """n points seen from three keyframes and m frames driven forward and
    sideways with small rotations.  The map points lie on their anchor's ray
    at 0.6 or 1.7 of the true depth.  Observations: the true projection with
    0.3 px of noise, one in five displaced by up to 30 px, 15 % unflagged;
    rows i % 11 == 0 have no anchor, rows i % 13 == 5 no flagged observation."""
    seed = SEEDS.get((n, m), 0) if seed is None else seed
    rng = np.random.default_rng(100000 * seed + 10 * n + m)
    kf = np.stack([pose_refine_ref.left_update([0.2 * j, -0.05 * j, -0.6 * j, 0.004 * j, -0.01 * j, 0.006 * j], IDENT)
                   for j in range(3)])
    frames = np.stack([pose_refine_ref.left_update(
        [(-1.0) ** j * rng.uniform(0.8, 2.0), rng.uniform(-0.3, 0.3), -rng.uniform(FWD[0], FWD[1]),
         rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)], IDENT)
        for j in range(m)]).reshape(m, 12)
    i = np.arange(n)
    Pt = _ray_points(n, rng, K_KITTI)
    Pt = Pt * ((DEPTH[0] + (Pt[:, 2] - 5.0) * (DEPTH[1] - DEPTH[0]) / 35.0) / Pt[:, 2])[:, None]
    an = np.where(i % 11 == 0, -1, rng.integers(0, 3, n)).astype(np.int32)
    C = ref.centres(kf)[np.maximum(an, 0)]
    scale = np.where(rng.integers(0, 2, n) == 1, SCALE[1], SCALE[0])
    P = C + (Pt - C) * scale[:, None]
    uv = np.stack([_project(Pt, T, K_KITTI)[0] for T in frames])
    uv = uv + rng.normal(0.0, 0.3, uv.shape)
    out = rng.uniform(0, 1, (m, n)) < 0.2
    uv = uv + out[:, :, None] * rng.uniform(-30.0, 30.0, uv.shape)
    valid = ((rng.uniform(0, 1, (m, n)) >= 0.15) & (i % 13 != 5)[None, :]).astype(np.uint8)
    s = {"points": P, "anchor_kf": an, "kf_poses": kf.reshape(3, 12), "frame_poses": frames, "obs_valid": valid,
         "obs_uv": uv, "iterations": PARITY_ITER, "huber_px": PARITY_HUBER, "min_obs": min(3, m),
         "max_rel_sigma": PARITY_SIGMA}
    s["ref"] = ref.refine(K=K_KITTI, **s)
    s["truth"] = Pt
    for a in (P, an, valid, uv, frames, s["ref"]["points"], s["ref"]["status"], s["ref"]["steps"], s["ref"]["costs"]):
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _row(n, seed=0):
    """An LK row: rows i % 5 == 0 unpaired, 1 failed, the others shifted by
    0 to 16 px (the bound is 8)."""
    rng = np.random.default_rng(7000 * seed + n)
    i = np.arange(n)
    ub = np.stack([rng.uniform(0, 1242, n), rng.uniform(0, 375, n)], 1)
    rad, ang = rng.uniform(0.0, 16.0, n), rng.uniform(0, 2 * np.pi, n)
    ua = ub + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    pk = np.where(i % 5 == 0, -1, rng.integers(0, 4, n)).astype(np.int32)
    sc = np.where(i % 5 == 1, 0, 1).astype(np.uint8)
    return pk, sc, ub, ua


def test_parity_cases_are_clear_of_every_threshold():
    seen = np.zeros(6, np.int64)
    worst = float("inf")
    for n in STAGE_N:
        for m in STAGE_M:
            s = _case(n, m)
            r = s["ref"]
            mg = r["margins"]
            seen += np.bincount(r["status"], minlength=6)
            worst = min(worst, mg.smallest())
            if n >= 2049:
                print("n", n, "m", m, "counts", r["counts"], "statuses", np.bincount(r["status"], minlength=6), mg)
            assert mg.smallest() > 1e-9, (n, m, mg)
        v, uv, margin = ref.record(*_row(n), 8.0)
        assert margin > 1e-9, n
        if n >= 63:
            assert 0 < v.sum() < n
    print("statuses over all cases", seen, "smallest margin", worst)
    assert (seen > 0).all()  # every status occurs
    # the refinement does what it is for: the moved points end nearer the truth
    s = _case(2049, 8)
    r = s["ref"]
    mv = r["steps"] >= 1
    C = ref.centres(s["kf_poses"])[np.maximum(s["anchor_kf"], 0)]
    depth = lambda P: np.linalg.norm(P - C, axis=1)  # noqa: E731
    e0 = np.abs(depth(s["points"]) / depth(s["truth"]) - 1.0)[mv]
    e1 = np.abs(depth(r["points"]) / depth(s["truth"]) - 1.0)[mv]
    print("moved", mv.sum(), "median relative depth error before", np.median(e0), "after", np.median(e1))
    assert np.median(e1) < 0.05 * np.median(e0)


# ------------------------------------------------------------------ CPU: the oracle's pipeline
W, H = 416, 128  # the smallest synthetic size whose stereo initialisation makes a map (328 points)
N_PIPE = 13      # the stereo frame and 12 tracking frames
# interval, window, iterations, huber_px, max_shift_px, min_obs, max_rel_sigma.  The sequence drives
# forward: at 0.05 the 12 frames' parallax moves 7 points, at 0.1 more than 200
PREFINE = (4, 4, 3, 1.0, 8.0, 3, 0.1)


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


def test_the_oracle_pipeline_has_points_to_move():
    """The oracle's pipeline alone (stereo initialisation, then left images,
    its frozen map): the restatement on its poses and LK rows moves at least
    20 points in one refinement."""
    seq = _seq()
    interval, window, iterations, huber, shift, min_obs, sigma = PREFINE
    ov = oracle_lib.Viso(seq.K, W, H, enable_tracking=1)
    ov.set_stereo(seq.p.baseline, 128, 1)
    ov.on_new_stereo(_image(0), _image(0, 1))
    assert ov.state == 1
    pts, kfp = ov.points(), ov.keyframe_poses()
    an, amg = ref.anchors(pts, kfp, seq.K, W, H)
    assert amg > 1e-9
    ring = ref.Ring(window, shift)
    moved = []
    for f in range(1, N_PIPE):
        ov.on_new_frame(_image(f))
        ring.record(ov.alignment(), ov.poses()[-1])
        if f % interval == 0:
            r = ref.refine(pts, an, kfp, *ring.live(), seq.K, iterations, huber, min_obs, sigma)
            print("frame", f, "counts", r["counts"], "statuses", np.bincount(r["status"], minlength=6))
            moved.append(r["counts"][1])
    assert max(moved) >= 20


# ------------------------------------------------------------------ CPU: the ABI
def test_abi_exports_and_null_context():
    from viso_amd import _lib
    lib = _lib.load()
    for name in ("viso_set_point_refine", "viso_get_point_refine", "viso_get_point_refine_status",
                 "viso_point_obs_record", "viso_points_refine"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert _lib.KERNEL_IDS["points"] == 12
    n = ctypes.c_size_t(0)
    info = (ctypes.c_int64 * 8)()
    cnt = (ctypes.c_int32 * 4)()
    pose = np.ascontiguousarray(IDENT)
    assert lib.viso_set_point_refine(None, 4, 4, 3, 1.0, 8.0, 3, 0.05) == -1
    assert lib.viso_get_point_refine(None, info) == -1
    assert lib.viso_get_point_refine_status(None, None, None, 0, ctypes.byref(n)) == -1
    assert lib.viso_point_obs_record(None, None, None, None, None, 0, 8.0, None, None) == -1
    assert lib.viso_points_refine(None, None, None, 0, pose.ctypes.data, 1, pose.ctypes.data, 1, None, None, 3, 1.0, 1,
                                  0.05, None, None, None, None, cnt) == -1


# ------------------------------------------------------------------ GPU: the stage entries
@functools.lru_cache(maxsize=None)
def _ctx(K=K_KITTI):
    from viso_amd import api
    fx, fy, cx, cy = K
    return api.Context(api.default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=1242, height=375))


def _same(g, r, tag):
    """GPU result against the restatement's; returns whether every bit agrees."""
    assert np.array_equal(g["status"], r["status"]), tag
    assert np.array_equal(g["steps"], r["steps"]), tag
    assert g["counts"] == r["counts"], tag
    if len(r["points"]):
        assert _dist(g["points"], r["points"]) < BAR, tag
        still = r["steps"] == 0
        assert np.array_equal(g["points"][still], r["points"][still]), tag  # unchanged: bit-equal
        assert np.abs(g["costs"] - r["costs"]).max() <= 1e-9 * max(1.0, np.abs(r["costs"]).max()), tag
        assert np.allclose(g["costs"], r["costs"], rtol=1e-9, atol=0.0), tag
    return np.array_equal(g["points"], r["points"]) and np.array_equal(g["costs"], r["costs"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", STAGE_N)
def test_gpu_stage_entries_match_restatement(n):
    bits = []
    for m in STAGE_M:
        s = _case(n, m)
        g = _ctx().refine_points(**{k: s[k] for k in ARGS})
        bits.append(_same(g, s["ref"], (n, m)))
    print("n", n, "bit-equal per m", bits)
    pk, sc, ub, ua = _row(n)
    v, uv, _ = ref.record(pk, sc, ub, ua, 8.0)
    gv, guv = _ctx().point_obs_record(pk, sc, ub, ua, 8.0)
    assert np.array_equal(gv, v) and np.array_equal(guv, uv)


@pytest.mark.gpu
def test_gpu_stage_crafted_cases():
    ctx = _ctx(K_WHOLE)
    for name in sorted(CRAFTED):
        case, status, steps = CRAFTED[name]
        g = ctx.refine_points(**case)
        r = _run(case)
        print(name, g["status"], g["steps"], g["costs"], g["points"])
        assert g["status"][0] == status and g["steps"][0] == steps
        assert _same(g, r, name), name  # these are bit-equal
    g = ctx.refine_points(**_tree_case())
    assert g["costs"][0, 0] == 1.0 + 3 * EPS
    # the exact shift bound
    ub = [[600.0, 180.0]] * 3
    ua = [[608.0, 180.0], [608.0 + 2.0 ** -30, 180.0], [600.0, 172.0]]
    v, uv = ctx.point_obs_record([0, 0, 0], [1, 1, 1], ub, ua, 8.0)
    assert list(v) == [1, 0, 1] and np.array_equal(uv, np.asarray(ua))


@pytest.mark.gpu
def test_gpu_stage_argument_codes():
    from viso_amd import _lib
    lib, h = _lib.load(), _ctx().h
    P, an = np.zeros((2, 3)), np.zeros(2, np.int32)
    P[:, 2] = 10.0
    kf, fp = np.ascontiguousarray([IDENT]), np.ascontiguousarray([SIDE, SIDE])
    ov, ouv = np.ones((2, 2), np.uint8), np.full((2, 2, 2), 100.0)
    out, st, sp, co, cnt = np.zeros((2, 3)), np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros((2, 2)), np.zeros(4, np.int32)

    def p(a):
        return None if a is None else a.ctypes.data

    def call(n=2, pts=P, a=an, kfp=kf, n_kf=1, f=fp, m=2, v=ov, uv=ouv, it=3, hub=1.0, mo=2, sig=0.05, o=out, s=st,
             stp=sp, c=co, k=cnt):
        return lib.viso_points_refine(h, p(pts), p(a), n, p(kfp), n_kf, p(f), m, p(v), p(uv), it, hub, mo, sig, p(o),
                                      p(s), p(stp), p(c), p(k))

    assert call() == 0
    assert call(n=0, pts=None, a=None, v=None, uv=None, o=None, s=None, stp=None, c=None) == 0
    assert call(it=10, mo=8, sig=1.0) == 0
    bad_anchor = np.array([0, 1], np.int32)
    for kw in ({"n": -1}, {"n": 16385}, {"pts": None}, {"a": None}, {"a": bad_anchor}, {"kfp": None}, {"n_kf": 0},
               {"n_kf": 9}, {"f": None}, {"m": 0}, {"m": 9}, {"v": None}, {"uv": None}, {"it": 0}, {"it": 11},
               {"hub": 0.0}, {"hub": float("nan")}, {"hub": float("inf")}, {"mo": 0}, {"mo": 9}, {"sig": 0.0},
               {"sig": 1.5}, {"sig": float("nan")}, {"o": None}, {"s": None}, {"stp": None}, {"c": None}, {"k": None}):
        assert call(**kw) == -1, kw

    pk, sc, ub, ua = np.zeros(2, np.int32), np.ones(2, np.uint8), np.zeros((2, 2)), np.ones((2, 2))
    vo, uo = np.zeros(2, np.uint8), np.zeros((2, 2))

    def rec(n=2, a=pk, b=sc, c=ub, d=ua, shift=8.0, e=vo, f=uo):
        return lib.viso_point_obs_record(h, p(a), p(b), p(c), p(d), n, shift, p(e), p(f))

    assert rec() == 0 and rec(n=0, a=None, b=None, c=None, d=None, e=None, f=None) == 0
    for kw in ({"n": -1}, {"n": 16385}, {"a": None}, {"b": None}, {"c": None}, {"d": None}, {"shift": 0.0},
               {"shift": float("nan")}, {"shift": float("inf")}, {"e": None}, {"f": None}):
        assert rec(**kw) == -1, kw


# ------------------------------------------------------------------ GPU: the pipeline
def _viso(prefine=PREFINE, cull=None, refine=None, mono=None, window=None, ba=0):
    import viso_amd
    seq = _seq()
    gv = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32)
    gv.set_stereo(seq.p.baseline, 128, 1)
    if prefine is not None:
        gv.set_point_refine(*prefine)
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


def _snap(gv):
    return {"points": gv.GetPoints(), "info": gv.point_refine(), "status": gv.point_refine_status(),
            "kf": gv.keyframe_poses()}


def _step(gv, f):
    gv.OnNewFrame(_image(f))
    s = _snap(gv)
    s["pose"] = gv.poses[-1]
    s["row"] = gv.alignment()
    return s


class _Model:
    """The restatement carried along a run: fed the GPU's own LK row, pose,
    keyframe poses and (where something else moved or removed points) map
    after every frame."""

    def __init__(self, points, kf_poses, prefine=PREFINE):
        (self.interval, self.window, self.iterations, self.huber, self.shift, self.min_obs,
         self.sigma) = prefine
        self.ring = ref.Ring(self.window, self.shift)
        self.runs = self.moved = 0
        self.last = [-1, 0, 0, 0]
        self.status = (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
        self.margin = float("inf")
        self.amargin = float("inf")
        self.shift_margin = float("inf")
        self.rebuilt(points, kf_poses)

    def rebuilt(self, points, kf_poses):
        """The LK templates were rebuilt on this map: new anchors, an empty ring."""
        self.points, self.kf = np.array(points), np.array(kf_poses)
        self.anchor, mg = ref.anchors(self.points, self.kf, _seq().K, W, H)
        self.amargin = min(self.amargin, mg)
        self.shift_margin = min(self.shift_margin, self.ring.margin)
        self.ring.reset()

    def frame(self, t, row, pose, frames):
        """Tracking frame t (frames: the frames processed before it): the
        record and, on an interval frame, the refinement (returned)."""
        pk, sc, ub, ua = row
        assert len(pk) == len(self.points)
        # a paired point is paired with its template's keyframe
        assert np.array_equal(pk[pk >= 0], self.anchor[pk >= 0])
        self.ring.record(row, pose)
        if t % self.interval:
            return None
        r = ref.refine(self.points, self.anchor, self.kf, *self.ring.live(), _seq().K, self.iterations, self.huber,
                       self.min_obs, self.sigma)
        self.margin = min(self.margin, r["margins"].smallest())
        self.points = r["points"]
        self.runs += 1
        self.moved += r["counts"][1]
        self.last = [frames, r["counts"][0], r["counts"][1], r["counts"][2]]
        self.status = (r["status"], r["steps"])
        return r

    def info(self):
        return [self.interval, self.window, self.runs, self.moved] + self.last


def _check(s, m, tag):
    assert list(s["info"]) == m.info(), tag
    assert np.array_equal(s["status"][0], m.status[0]) and np.array_equal(s["status"][1], m.status[1]), tag


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
                          "launches": gv.ctx.timing("points")[0]}
        gv.close()
    return _runs[batched]


@pytest.mark.gpu
def test_gpu_pipeline_matches_restatement():
    res = _pipeline(False)
    first, snaps = res["first"], res["snaps"]
    assert len(first["points"]) > 50 and list(first["info"]) == list(PREFINE[:2]) + [0, 0, -1, 0, 0, 0]
    assert len(first["status"][0]) == 0
    K = _seq().K
    m = _Model(first["points"], first["kf"])
    refined, bits = [], []
    after = False
    for f in range(1, N_PIPE):
        s = snaps[f]
        if after:
            # the frame after a refinement tracks against the refined map
            prev = snaps[f - 1]["pose"]
            exp = oracle_lib.direct_pose(_pyr(f - 1), _pyr(f), W, H, K, m.points, prev, prev)
            d = _dist(s["pose"], exp)
            print("frame", f, "after the refinement: pose relative difference", d)
            assert d < BAR
            after = False
        r = m.frame(f, s["row"], s["pose"], f)
        _check(s, m, f)
        assert np.array_equal(s["kf"], m.kf)
        assert _dist(s["points"], m.points) < BAR, f
        if r is not None:
            print("frame", f, "counts", r["counts"], "statuses", np.bincount(r["status"], minlength=6), r["margins"])
            bits.append(np.array_equal(s["points"], m.points))
            refined.append(r["counts"][1])
            after = True
            m.points = s["points"]  # (carried on from the GPU's own bits)
    print("moved per refinement", refined, "bit-equal", bits, "anchor margin", m.amargin, "shift margin", m.ring.margin)
    # (a converged point's cost comparison sits on a rounding error, so the
    # refinement's own margin is printed, not asserted: the statuses above
    # were equal because every bit is)
    print("smallest decision margin", m.margin)
    assert m.amargin > 1e-9 and m.ring.margin > 1e-9
    assert len(refined) == 3 and max(refined) >= 20
    # one record launch a frame, one refine launch an interval frame
    assert res["launches"] == (N_PIPE - 1) + (N_PIPE - 1) // PREFINE[0]


@pytest.mark.gpu
def test_gpu_pipeline_ingest_forms_agree():
    a, b = _pipeline(False), _pipeline(True)
    assert np.array_equal(a["poses"], b["poses"])
    assert np.array_equal(a["final"]["points"], b["final"]["points"])
    assert np.array_equal(a["final"]["info"], b["final"]["info"])
    for x, y in zip(a["final"]["status"], b["final"]["status"]):
        assert np.array_equal(x, y)
    assert a["launches"] == b["launches"]


@pytest.mark.gpu
def test_gpu_off_is_off():
    from viso_amd import _lib
    runs = []
    for setter in (False, True):
        gv = _viso(prefine=None)
        cfg = gv.config()
        gv.ctx.timing_enable(True)
        if setter:
            gv.set_point_refine(0)
            assert gv.config() == cfg
        for f in range(1, 10):
            gv.OnNewFrame(_image(f))
        n = ctypes.c_size_t(0)
        assert _lib.load().viso_get_point_refine_status(gv.ctx.h, None, None, 0, ctypes.byref(n)) == -4
        assert gv.ctx.timing("points")[0] == 0
        assert list(gv.point_refine()) == [0, 0, 0, 0, -1, 0, 0, 0]
        runs.append((gv.poses, gv.GetPoints()))
        gv.close()
    assert len(runs[0][0]) == 9
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    # and on, the map moves
    on = _pipeline(False)
    assert len(on["final"]["points"]) == len(runs[0][1]) and not np.array_equal(on["snaps"][9]["points"], runs[0][1])


@pytest.mark.gpu
def test_gpu_setter_codes_and_switching_on_while_tracking():
    from viso_amd import _lib
    gv = _viso(prefine=None)
    lib, h = _lib.load(), gv.ctx.h
    nan, inf = float("nan"), float("inf")
    for args in ((-1, 4, 3, 1.0, 8.0, 3, 0.05), (4, 1, 3, 1.0, 8.0, 1, 0.05), (4, 9, 3, 1.0, 8.0, 3, 0.05),
                 (4, 4, 0, 1.0, 8.0, 3, 0.05), (4, 4, 11, 1.0, 8.0, 3, 0.05), (4, 4, 3, 0.0, 8.0, 3, 0.05),
                 (4, 4, 3, nan, 8.0, 3, 0.05), (4, 4, 3, inf, 8.0, 3, 0.05), (4, 4, 3, 1.0, 0.0, 3, 0.05),
                 (4, 4, 3, 1.0, nan, 3, 0.05), (4, 4, 3, 1.0, inf, 3, 0.05), (4, 4, 3, 1.0, 8.0, 0, 0.05),
                 (4, 4, 3, 1.0, 8.0, 5, 0.05), (4, 4, 3, 1.0, 8.0, 3, 0.0), (4, 4, 3, 1.0, 8.0, 3, 1.5),
                 (4, 4, 3, 1.0, 8.0, 3, nan)):
        assert lib.viso_set_point_refine(h, *args) == -1, args
    for args in ((1, 2, 1, 0.5, 0.5, 1, 1.0), (1000, 8, 10, 100.0, 100.0, 8, 1e-6), (0, 0, 0, 0.0, 0.0, 0, 0.0)):
        assert lib.viso_set_point_refine(h, *args) == 0, args
    n = ctypes.c_size_t(0)
    for f in range(1, 6):
        gv.OnNewFrame(_image(f))
    assert lib.viso_get_point_refine_status(h, None, None, 0, ctypes.byref(n)) == -4
    gv.set_point_refine(*PREFINE)  # while tracking: the ring counts from frame 6
    first = _snap(gv)
    assert list(first["info"]) == list(PREFINE[:2]) + [0, 0, -1, 0, 0, 0]
    m = _Model(first["points"], first["kf"])
    for f in range(6, 13):
        s = _step(gv, f)
        # (tracking frames 8 and 12 refine: the count runs from the map's
        # creation; at frame 8 the ring holds frames 6, 7 and 8)
        r = m.frame(f, s["row"], s["pose"], f)
        if f == 8:
            assert m.ring.count == 3 and r is not None
        _check(s, m, f)
        assert _dist(s["points"], m.points) < BAR, f
        m.points = s["points"]
    assert m.runs == 2 and m.amargin > 1e-9 and m.ring.margin > 1e-9
    gv.set_point_refine(0)
    assert lib.viso_get_point_refine_status(h, None, None, 0, ctypes.byref(n)) == -4
    gv.OnNewFrame(_image(13))
    gv.set_point_refine(*PREFINE)  # on again: empty again
    assert list(gv.point_refine()) == list(PREFINE[:2]) + [0, 0, -1, 0, 0, 0]
    gv.close()


@pytest.mark.gpu
def test_gpu_composes_with_cull_pose_refinement_insertion_window_and_ba():
    """Cull every 4th frame, pose refinement, monocular insertion every 5th
    frame (8-pixel cells, 0.1 degrees), a window of 2 keyframes and the BA
    behind every insertion, over 20 tracking frames.  The ring restarts at
    every template rebuild (an applied cull, a retirement, an insertion); the
    restatement rebuilds its ring and anchors there from the GPU's map and
    keyframe poses, and every refinement equals the restatement's on that
    ring."""
    n = 21
    gv = _viso(cull=(4, 3, 2.0, 50), refine=(5, 1.0, 8.0), mono=(5, 1000, 8, 0.1), window=(2, 16), ba=2)
    s0 = _snap(gv)
    m = _Model(s0["points"], s0["kf"])
    events = []
    for f in range(1, n):
        b_cull, b_win, b_n, b_kf = gv.point_cull()[2], gv.map_window()[2], len(m.points), len(m.kf)
        s = _step(gv, f)
        before = m.points
        r = m.frame(f, s["row"], s["pose"], f)
        _check(s, m, f)
        culled = gv.point_cull()[2] > b_cull
        retired = gv.map_window()[2] > b_win
        inserted = len(s["kf"]) > b_kf - (1 if retired else 0)
        rebuilt = culled or retired or inserted
        if r is not None and not rebuilt:
            assert _dist(s["points"], m.points) < BAR, f
        elif r is None and not rebuilt:
            assert np.array_equal(s["points"], before), f
        events.append((f, -1 if r is None else r["counts"][1], culled, retired, inserted, len(s["points"]),
                       m.ring.count))
        if rebuilt:
            m.rebuilt(s["points"], s["kf"])
        else:
            m.points = s["points"]
    info = gv.point_refine()
    poses = gv.poses
    gv.close()
    for e in events:
        print("frame %2d moved %3d culled %d retired %d inserted %d map %4d ring %d" % e)
    print("info", list(info), "margins", m.margin, m.amargin)
    assert m.amargin > 1e-9 and m.shift_margin > 1e-9
    assert len(poses) == n - 1 and np.isfinite(poses).all()
    assert info[2] == 5 and any(e[2] for e in events) and any(e[3] for e in events) and any(e[4] for e in events)
    assert any(e[1] > 0 for e in events)
