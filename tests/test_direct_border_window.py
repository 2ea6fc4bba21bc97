"""Direct pose at the image borders and the merged L(3)'s moved `last` taps
(viso_amd/csrc/direct.hip win_issue / direct_point_rs / merged_ref) against
the fp64 oracle.

The current-image window is a window of the level's continuous buffer
(origin not clamped; tests/test_direct_window_model.py is its host model), so
inputs of the classes edge_lt / edge_r / edge_b of tests/direct_cases.py (a
classification of the *inputs*, computed from the oracle alone with the
clamped origin the kernel used to have) now take the whole-patch kernel
branches instead of the per-sample one.  The cases here are made of such
points:

* 160 x 160 (level 3 is 20 x 20, the smallest level that has a window: the
  window of every level-3 point reaches past the image) and 168 x 160 (level
  3 is 21 x 20: an unclamped origin can differ from the clamped one by a
  column):
  300 random points as direct_cases.make places them plus 16 placed ones, one
  per border and corner at level 0 and at level 3, among them a projection in
  [4, 5) (a gradient tap coordinate in (-1, 0)), one in [w - 5, w - 4) (tap
  column w wraps into the next row) and the bottom-right corner (tap index
  reaches w h: zero taps).  Level 3 starts at the identity, so there the
  current projection is the `last` one and every class is reachable.  At
  level 0 the current projection is the `last` one moved by the image shift,
  and both must lie 4 px inside: a shift of (+1, +1) reaches the right and
  bottom bands (and their corner), (-1, -1) the left and top ones, so the two
  sizes take one shift each and each asserts the level-0 classes its shift
  can reach; together they cover all three.  The census is taken from the
  oracle before the GPU is looked at.  Faithful: rel. Frobenius < 1e-12
  against oracle_lib.direct_pose; tolerance mode: < 1e-4, on inputs within
  direct_cases.COND_CEILING.
* merged L(3), 416 x 160, viso_amd.synth.Sequence(416, 160, seed=0): stereo
  initialisation at frame 0, frames 1-6 in one process_device call, so five
  launches are merged ones.  Under the oracle a few points' level-3 `last`
  base pixel moves between the pose the previous frame's level 0 started from
  (the prefetch's prediction) and its solved pose: the test recomputes that
  count (>= 4 over the frames) and the level-3 border classes from the oracle,
  then holds every pose to 1e-10 rel. against oracle_lib.Viso with the map and
  the last alignment exact.  The same through the one-camera rig path.
"""
import functools

import numpy as np
import pytest

from tests import direct_cases as dc
from tests import oracle_lib

PLACED_Z = 8.0


def _rel_frob(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _placed(w, h, s):
    """16 (u, v) at level 0: per border and corner, 8 whose level-0 current
    projection (u + s, v + s for an image shift of s px) lies in the outermost
    good pixel, and 8 whose level-3 projection (u / 8, v / 8) does."""
    ws, hs = dc.level_dims(w, h)
    out = []
    # level 0: `last` projection such that the current one is half a pixel
    # inside the band next to the border the shift moves towards, and a
    # quarter pixel inside the `last` bound on the other side
    lo = 4.5 - s if s < 0 else 4.25
    hx = w - 4.5 - s if s > 0 else w - 4.25
    hy = h - 4.5 - s if s > 0 else h - 4.25
    mx, my = w / 2 + 0.3, h / 2 - 0.2
    out += [(lo, my), (hx, my), (mx, lo), (mx, hy), (lo, lo), (hx, lo), (lo, hy), (hx, hy)]
    # level 3 (starts at the identity: current = `last` projection)
    w3, h3 = ws[3], hs[3]
    l3, rx, by = 4.5, w3 - 4.5, h3 - 4.5
    cx, cy = w3 / 2 + 0.3, h3 / 2 - 0.2
    out += [(8 * u, 8 * v) for u, v in
            [(l3, cy), (rx, cy), (cx, l3), (cx, by), (l3, l3), (rx, l3), (l3, by), (rx, by)]]
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _case(w, h, s):
    c = dict(dc.make(w, h, (s, s), 300, 5, 12, 0.5))
    K = c["K"]
    uv = _placed(w, h, s)
    z = np.full(len(uv), PLACED_Z)
    extra = np.stack([(uv[:, 0] - K[2]) / K[0] * z, (uv[:, 1] - K[3]) / K[1] * z, z], 1)
    pts = np.concatenate([c["points"], extra])
    pts.setflags(write=False)
    c["points"] = pts
    cen = dc.census_of(c)
    exp = oracle_lib.direct_pose(c["last"], c["cur"], w, h, K, pts, c["pose_last"], c["pose_init"])
    exp.setflags(write=False)
    return c, cen, exp


CASES = [(160, 160, 1), (168, 160, -1)]


def _assert_census(w, h, s):
    _, cen, _ = _case(w, h, s)
    ws, hs = dc.level_dims(w, h)
    assert (ws[3], hs[3]) == (w // 8, 20)
    for k in ("edge_lt", "edge_r", "edge_b"):
        assert cen[k][3] > 0, (k, dc.format_census(cen))
    reach = ("edge_r", "edge_b") if s > 0 else ("edge_lt",)
    for k in reach:
        assert cen[k][0] > 0, (k, dc.format_census(cen))
    assert cen["win_off"] == [0, 0, 0, 0] and cen["moved"]
    return cen


def test_border_cases_populate_every_edge_class():
    """CPU: the census of the two cases (oracle only)."""
    l0 = set()
    for w, h, s in CASES:
        cen = _assert_census(w, h, s)
        l0 |= {k for k in ("edge_lt", "edge_r", "edge_b") if cen[k][0] > 0}
        assert cen["per_sample"][3] > 0 and cen["per_sample"][0] > 0
    assert l0 == {"edge_lt", "edge_r", "edge_b"}


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,s", CASES)
@pytest.mark.parametrize("fast", [False, True])
def test_gpu_direct_border_points(w, h, s, fast):
    import viso_amd
    cen = _assert_census(w, h, s)
    c, _, exp = _case(w, h, s)
    K = c["K"]
    if fast:
        assert max(cen["cond"]) <= dc.COND_CEILING, dc.format_census(cen)
        ctx = viso_amd.Context(viso_amd.default_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3],
                                                       precision=viso_amd.PRECISION_FAST))
    else:
        ctx = viso_amd.default_context(K=K)
    got = ctx.direct_pose(c["last"], c["cur"], w, h, c["points"], c["pose_last"], c["pose_init"])
    rel = _rel_frob(got, exp)
    bar = 1e-4 if fast else 1e-12
    print(f"direct pose {w}x{h} shift {s} {'fast' if fast else 'faithful'}: rel Frobenius {rel:.3e} (bar {bar:g})")
    assert np.isfinite(got).all() and rel < bar, f"rel {rel:.3e} >= {bar:g}\n" + dc.format_census(cen)


# ---------------------------------------------------------------- merged L(3)
MW, MH, MFRAMES = 416, 160, 7


def _moved_last_bases(K, w3, h3, P, pose_pred, pose_solved):
    """Points whose level-3 `last` patch has a lane with another int() base
    pixel under the solved pose than under the predicted one (both good)."""
    s = dc.SCALES[3]
    up, vp = dc._project(pose_pred, K, P, s)
    us, vs = dc._project(pose_solved, K, P, s)
    ok = (dc._inside(up - 4, vp - 4, w3, h3) & dc._inside(up + 4, vp + 4, w3, h3) &
          dc._inside(us - 4, vs - 4, w3, h3) & dc._inside(us + 4, vs + 4, w3, h3))
    moved = np.zeros(len(P), bool)
    for d in range(-4, 4):
        moved |= (np.trunc(up + d) != np.trunc(us + d)) | (np.trunc(vp + d) != np.trunc(vs + d))
    return ok & moved


@functools.lru_cache(maxsize=None)
def _merged_oracle():
    from viso_amd.synth import Sequence
    seq = Sequence(MW, MH, seed=0)
    left = np.stack([seq.image(f, 0) for f in range(MFRAMES)])
    right0 = seq.image(0, 1)
    ov = oracle_lib.Viso(seq.K, MW, MH, enable_tracking=1)
    ov.set_stereo(seq.p.baseline, 128, 1)
    ov.on_new_stereo(left[0], right0)
    for f in range(1, MFRAMES):
        ov.on_new_frame(left[f])
    assert ov.state == 1
    pts, poses = ov.points(), ov.poses()
    assert poses.shape == (MFRAMES - 1, 12)
    # census of the frames whose final solve sits in a merged launch: frame f
    # (f < MFRAMES - 1) is solved in the L(3) launch of frame f + 1
    pyr = [oracle_lib.pyramid(im) for im in left]
    ws, hs = dc.level_dims(MW, MH)
    moved, edges = [], {k: [] for k in ("per_sample", "edge_lt", "edge_r", "edge_b")}
    for f in range(1, MFRAMES):
        last_pose = dc.IDENTITY if f == 1 else poses[f - 2]
        c = dict(last=pyr[f - 1], cur=pyr[f], w=MW, h=MH, K=seq.K, points=pts, pose_last=last_pose,
                 pose_init=last_pose)
        start, _, final = dc.walk_levels(c)
        assert _rel_frob(final, poses[f - 1]) < 1e-12
        m = dc.classify_level(c, 3, start[3], last_pose)
        for k in edges:
            edges[k].append(int(m[k].sum()))
        if f < MFRAMES - 1:
            moved.append(int(_moved_last_bases(seq.K, ws[3], hs[3], pts, start[0], final).sum()))
    return dict(seq=seq, left=left, right0=right0, points=pts, poses=poses, alignment=ov.alignment(),
                moved=moved, edges=edges)


def test_merged_sequence_moves_last_bases_and_has_border_points():
    """CPU: what the merged GPU test relies on, from the oracle alone."""
    o = _merged_oracle()
    assert len(o["points"]) > 300
    assert sum(o["moved"]) >= 4, o["moved"]
    for k, v in o["edges"].items():
        assert min(v) > 0, (k, v)


@pytest.mark.gpu
def test_gpu_merged_l3_moved_bases_and_border_points():
    import torch

    import viso_amd
    o = _merged_oracle()
    assert sum(o["moved"]) >= 4 and all(min(v) > 0 for v in o["edges"].values())
    seq, left = o["seq"], o["left"]
    dl = torch.from_numpy(left).cuda()
    dr = torch.from_numpy(o["right0"][None]).cuda()
    torch.cuda.synchronize()
    fb = MW * MH
    v = viso_amd.Viso(*seq.K, width=MW, height=MH, enable_tracking=1, batch_frames=8)
    v.set_stereo(seq.p.baseline, 128, 1)
    v.process_device(dl.data_ptr(), dr.data_ptr(), 1, fb)
    v.synchronize()
    assert v.state == 1
    v.process_device(dl.data_ptr() + fb, None, MFRAMES - 1, fb)
    v.synchronize()
    gp, gP, gal = v.GetPoints(), v.poses, v.alignment()
    v.close()
    assert np.array_equal(gp, o["points"])
    assert gP.shape == o["poses"].shape
    rel = np.linalg.norm(gP - o["poses"], axis=1) / np.linalg.norm(o["poses"], axis=1)
    print("merged L(3) 416x160: pose rel per frame", rel, "moved-base points per frame", o["moved"])
    assert rel.max() <= 1e-10
    pk, sc, ub, ua = gal
    opk, osc, oub, oua = o["alignment"]
    assert np.array_equal(pk, opk) and np.array_equal(sc, osc)
    assert np.array_equal(ub, oub) and np.array_equal(ua, oua)


@pytest.mark.gpu
def test_gpu_merged_l3_one_camera_rig():
    """The same size through the rig path (rig_level_kernel shares the
    prefetch and merged_ref): one camera, initialisation + 6 timesteps in one
    device call, against the rig oracle."""
    import torch

    from viso_amd.rig import VisoRig
    from viso_amd.synth import RigSequence
    seq = RigSequence(MW, MH, seed=0, n_cams=1)
    frames = [seq.frame(f) for f in range(MFRAMES)]
    r = oracle_lib.Rig(seq.K, MW, MH, seq.extrinsics(), seq.p.baseline)
    for ls, rs in frames:
        r.process(ls, rs)
    assert r.state == 1
    g = VisoRig(*seq.K, MW, MH, seq.extrinsics())
    g.set_stereo(seq.p.baseline, 128, 1)
    dl = torch.from_numpy(np.stack([im for ls, _ in frames for im in ls])).cuda()
    dr = torch.from_numpy(np.stack([im for _, rs in frames for im in rs])).cuda()
    torch.cuda.synchronize()
    g.process_device(dl.data_ptr(), dr.data_ptr(), len(frames), MW * MH)
    g.synchronize()
    assert g.state == 1
    assert np.array_equal(g.points(0), r.points(0))
    gP, oP = g.poses, r.poses
    assert gP.shape == oP.shape == (MFRAMES - 1, 12)
    rel = np.linalg.norm(gP - oP, axis=1) / np.linalg.norm(oP, axis=1)
    assert rel.max() <= 1e-10, rel
