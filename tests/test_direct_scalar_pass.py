"""The direct pose's scalar pass (viso_amd/csrc/direct.hip scalar_pass): in a
tile of 9 or 10 points the workgroup's two idle waves compute every point's
projection, dPixel/dXi quotients, window class and bilinear weights, five
points per wave and 12 lanes per point, and the point waves read them from
LDS.  The results must not depend on who computed them.

* CPU: the inputs are usable (the pattern of tests/test_direct_cases.py), and
  a numpy model of the pass (the lane placement, the operand slot tables of
  quotient_slot, which the helper's quotient_select picks by selects, the
  per-tile T rule) gives for every point of the `gentle` case, at every
  level, bit for bit the projection of direct_cases._project,
  the quotients of dPixel/dXi written out directly, the class of a direct
  per-point evaluation and the weights of the projection's fractions.  The
  class is also held against direct_cases.classify_level wherever that
  census' window origin (clamped into the image, the kernel's of an earlier
  round) equals the kernel's unclamped one.
* GPU, stage: Context.direct_pose against oracle_lib.direct_pose, relative
  Frobenius < 1e-12 (the stage's bar), on the gentle 320 x 240 pair at sizes
  with the pass on (T = 9, 10; full and partial last tiles) and off (T = 8,
  11), and on the named cases `gentle` and `wide`; a context created with
  VISO_DIRECT_SCALAR_PASS=0 gives the same bits.
* GPU, pipeline: one device-ingest call of the stereo initialisation and 8
  tracking frames at 1242 x 375 (merged L(3) launches with the pass on)
  against the oracle: poses <= 1e-10 relative, the per-frame level-0 nGood
  and cost exact, the last alignment (pairs, successes, positions before and
  after) exact; with the switch at 0 every output is bit-equal.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import direct_cases as dc
from tests import oracle_lib

N_ON = (2049, 2304, 2305, 2465, 2560)  # T = 9, 9 (full), 10, 10, 10 (full)
N_OFF = (2048, 2561, 2700)             # T = 8, 11, 11
NAMED = ("gentle", "wide")
SWITCH = "VISO_DIRECT_SCALAR_PASS"
# direct_cases' big_step pair at T = 10: prediction misses (the per-sample
# class, sample_cw) under the pass, which `gentle` and `wide` do not reach
BIG_STEP_T10 = (640, 480, (64, 0), 2465, 0, 128, 0.5)

# direct.hip: helpers, points per helper, lanes per point; quotient_slot's
# operand slots, 4 bits per quotient (slots: 0 x, 1 y, 2 fx, 3 -fx, 4 fx x,
# 5 fy, 6 -fy, 7 fy y, 8 1.0, 9 x y, 10 z, 11 z z)
HELPERS, PER_HELPER, LANES = 2, 5, 12
K_C1, K_C2, K_DEN = 0x557653433210, 0x091181090888, 0xABBBAABBBAAA
CLS_OUT, CLS_SHARED, CLS_STRADDLE, CLS_SAMPLE = 0, 1, 2, 3


def test_sizes_pin_the_tile_counts():
    assert [dc.map_tile(n) for n in N_ON] == [9, 9, 10, 10, 10]
    assert [dc.map_tile(n) for n in N_OFF] == [8, 11, 11]
    assert [n % dc.map_tile(n) == 0 for n in N_ON] == [False, True, False, False, True]
    assert dc.census("gentle")["tile"] == dc.census("wide")["tile"] == 10


@pytest.mark.parametrize("key", list(NAMED) + list(N_ON) + list(N_OFF))
def test_case_is_usable(key):
    cen = dc.census(key)
    assert all(cen["update_finite"]), (key, cen["update_finite"])
    assert all(g > 0 for g in cen["good"]), (key, cen["good"])
    assert cen["moved"], key
    p = dc.oracle_pose(key)
    assert np.isfinite(p).all() and not np.array_equal(p, dc.get(key)["pose_init"])


_extra: dict = {}


def _get(key):
    if key != "big_step_t10":
        return dc.get(key)
    if "case" not in _extra:
        _extra["case"] = dc.make(*BIG_STEP_T10)
    return _extra["case"]


def _oracle_pose(key):
    if key != "big_step_t10":
        return dc.oracle_pose(key)
    if "pose" not in _extra:
        c = _get(key)
        _extra["pose"] = oracle_lib.direct_pose(c["last"], c["cur"], c["w"], c["h"], c["K"], c["points"],
                                                c["pose_last"], c["pose_init"])
    return _extra["pose"]


def test_big_step_case_is_usable_and_reaches_sample_cw_under_the_pass():
    c = _get("big_step_t10")
    cen = dc.census_of(c)
    assert cen["tile"] == 10 and all(cen["update_finite"]) and all(g > 0 for g in cen["good"]) and cen["moved"]
    assert np.isfinite(_oracle_pose("big_step_t10")).all()
    start, _, _ = dc.walk_levels(c)
    per_level = []
    for lv in range(3):
        m = model_pass(c, lv, start[lv], start[lv + 1])
        d = _direct(c, lv, start[lv], start[lv + 1])
        assert m["covered"].all() and np.array_equal(m["cls"], d["cls"]) and np.array_equal(m["uc"], d["uc"])
        per_level.append(int((m["cls"] == CLS_SAMPLE).sum()))
    assert max(per_level) >= 8, per_level


# ------------------------------------------------------------------ the model
def _tiles(n, split):
    """tile_range: (first, count) per workgroup."""
    if split:
        nt = min(n, 256)
        f = [(b * n) // nt for b in range(nt + 1)]
        return [(f[b], f[b + 1] - f[b]) for b in range(nt)]
    T = dc.map_tile(n)
    return [(b * T, T) for b in range((n + T - 1) // T)]


def _slots(word, k):
    return (word >> (4 * k)) & 15


def model_pass(c, lv, pose, pred, split=False):
    """The helpers' pass over every tile of case c at level lv: per map point
    `covered` (a helper published it), q (12 quotients), uc, vc, cls, fu, fv
    and the four stored doubles."""
    P = np.asarray(c["points"], np.float64)
    n = len(P)
    ws, hs = dc.level_dims(c["w"], c["h"])
    w, h = ws[lv], hs[lv]
    s = dc.SCALES[lv]
    Kfx, Kfy, Kcx, Kcy = c["K"]
    tiles = [(f, T) for f, T in _tiles(n, split) if 8 < T <= 10]  # the T rule, per workgroup
    lane = np.arange(64)
    act = lane < PER_HELPER * LANES
    p = np.where(act, lane // LANES, PER_HELPER - 1)
    k = np.where(act, lane - LANES * p, LANES - 1)
    out = dict(covered=np.zeros(n, bool), q=np.zeros((n, 12)), uc=np.zeros(n), vc=np.zeros(n),
               cls=np.zeros(n, np.int64), fu=np.zeros(n, np.int64), fv=np.zeros(n, np.int64), s=np.zeros((n, 4)))
    if not tiles:
        return out
    first = np.array([f for f, _ in tiles])[:, None, None]
    T = np.array([t for _, t in tiles])[:, None, None]
    j = PER_HELPER * np.arange(HELPERS)[None, :, None] + p[None, None, :]  # [tile][helper][lane]
    valid = act[None, None, :] & (j < T) & (first + j < n)
    i = np.where(valid, first + j, 0)
    Pl = P[i]  # every lane of a point holds the point
    R, t = np.asarray(pose[:9]), np.asarray(pose[9:])
    x, y, z = [((R[3 * a] * Pl[..., 0] + R[3 * a + 1] * Pl[..., 1]) + R[3 * a + 2] * Pl[..., 2]) + t[a]
               for a in range(3)]
    fx, fy = Kfx * s, Kfy * s
    zz, xy = z * z, x * y
    fxx, fyy = fx * x, fy * y
    one = np.ones_like(x)
    table = np.stack([x, y, fx * one, -fx * one, fxx, fy * one, -fy * one, fyy, one, xy, z, zz], -1)
    kk = np.broadcast_to(k, x.shape)

    def pick(word):  # each lane's operand at its quotient's slot
        return table[:, :, lane, np.array([_slots(word, int(a)) for a in k])]

    with np.errstate(divide="ignore", invalid="ignore"):
        q = (pick(K_C1) * pick(K_C2)) / pick(K_DEN)
    q = np.where(kk == 5, fx + q, q)
    q = np.where(kk == 9, -fy - q, q)
    lead = LANES * p  # bpermute from the point's lanes 0 and 1
    Q0 = q[..., lead]
    Q1 = q[..., lead + 1]
    uc = s * (Q0 * Kfx + Kcx)
    vc = s * (Q1 * Kfy + Kcy)
    inside = dc._inside(uc - 4, vc - 4, w, h) & dc._inside(uc + 4, vc + 4, w, h)
    with np.errstate(invalid="ignore"):
        fu = np.where(np.isfinite(uc), np.floor(uc), 0).astype(np.int64)
        fv = np.where(np.isfinite(vc), np.floor(vc), 0).astype(np.int64)
    on, x0, y0 = _window(c, lv, pred, Pl)
    whole = on & (fu - 6 >= x0) & (fu + 5 <= x0 + dc.WIN - 2) & (fv - 6 >= y0) & (fv + 5 <= y0 + dc.WIN - 2)
    cls = np.where(~inside, CLS_OUT, np.where(~whole, CLS_SAMPLE, np.where(_one_binade(uc, vc), CLS_SHARED,
                                                                           CLS_STRADDLE)))
    xx, yy = uc - np.floor(uc), vc - np.floor(vc)
    w00, w10, w01, w11 = (1 - xx) * (1 - yy), xx * (1 - yy), (1 - xx) * yy, xx * yy
    shared = cls == CLS_SHARED
    stored = np.stack([np.where(shared, w00, uc), np.where(shared, w10, vc), w01, w11], -1)
    # the stores: lane k of a valid point writes quotient k, its lane 0 the rest
    sel = valid
    assert not out["covered"][i[sel & (kk == 0)]].any()
    out["q"][i[sel], kk[sel]] = q[sel]
    lead0 = sel & (kk == 0)
    for name, arr in (("uc", uc), ("vc", vc), ("cls", cls), ("fu", fu), ("fv", fv)):
        out[name][i[lead0]] = arr[lead0]
    out["s"][i[lead0]] = stored[lead0]
    out["covered"][i[lead0]] = True
    # every lane of a point agrees on the point's scalars
    for name, arr in (("uc", uc), ("vc", vc), ("cls", cls)):
        assert np.array_equal(arr[sel], out[name][i[sel]], equal_nan=True)
    return out


def _window(c, lv, pred, P):
    """win_issue: the window of the level's continuous buffer, not clamped."""
    ws, hs = dc.level_dims(c["w"], c["h"])
    w, h = ws[lv], hs[lv]
    shp = P.shape[:-1]
    up, vp = dc._project(pred, c["K"], P.reshape(-1, 3), dc.SCALES[lv])
    up, vp = up.reshape(shp), vp.reshape(shp)
    with np.errstate(invalid="ignore"):
        on = (w >= dc.WIN) & (h >= dc.WIN) & (up > -1e6) & (up < 1e6) & (vp > -1e6) & (vp < 1e6)
    x0 = np.where(on, np.floor(np.where(on, up, 0.0)).astype(np.int64) - dc.WIN // 2 + 1, 0)
    y0 = np.where(on, np.floor(np.where(on, vp, 0.0)).astype(np.int64) - dc.WIN // 2 + 1, 0)
    return on, x0, y0


def _one_binade(uc, vc):
    with np.errstate(invalid="ignore"):
        return ((uc >= 6.0) & (vc >= 6.0) & (dc._binade(uc - 6.0) == dc._binade(uc + 6.0)) &
                (dc._binade(vc - 6.0) == dc._binade(vc + 6.0)))


def _direct(c, lv, pose, pred):
    """The same scalars per point, written out without the pass: the
    projection of direct_cases._project, dPixel/dXi as src/viso.cpp:640-658
    forms it, the class tests of direct_point_rs."""
    P = np.asarray(c["points"], np.float64)
    ws, hs = dc.level_dims(c["w"], c["h"])
    w, h = ws[lv], hs[lv]
    s = dc.SCALES[lv]
    uc, vc = dc._project(pose, c["K"], P, s)
    R, t = np.asarray(pose[:9]), np.asarray(pose[9:])
    x, y, z = [((R[3 * a] * P[:, 0] + R[3 * a + 1] * P[:, 1]) + R[3 * a + 2] * P[:, 2]) + t[a] for a in range(3)]
    fx, fy = c["K"][0] * s, c["K"][1] * s
    zz, xy = z * z, x * y
    J = np.stack([fx / z, -fx * x / zz, -fx * xy / zz, fx + fx * x * x / zz, -fx * y / z, fy / z, -fy * y / zz,
                  -fy - fy * y * y / zz, fy * xy / zz, fy * x / z], 1)
    inside = dc._inside(uc - 4, vc - 4, w, h) & dc._inside(uc + 4, vc + 4, w, h)
    fu = np.floor(np.where(inside, uc, 0.0)).astype(np.int64)
    fv = np.floor(np.where(inside, vc, 0.0)).astype(np.int64)
    on, x0, y0 = _window(c, lv, pred, P)
    whole = on & (fu - 6 >= x0) & (fu + 5 <= x0 + dc.WIN - 2) & (fv - 6 >= y0) & (fv + 5 <= y0 + dc.WIN - 2)
    cls = np.where(~inside, CLS_OUT, np.where(~whole, CLS_SAMPLE, np.where(_one_binade(uc, vc), CLS_SHARED,
                                                                           CLS_STRADDLE)))
    return dict(uc=uc, vc=vc, J=J, cls=cls, fu=fu, fv=fv, on=on, x0=x0, y0=y0)


def test_model_of_the_pass_matches_the_oracle_projection_class_and_weights():
    c = dc.case("gentle")
    n = len(c["points"])
    start, _, _ = dc.walk_levels(c)
    seen, compared = set(), 0
    for lv in range(dc.LEVELS):
        pred = start[lv + 1] if lv + 1 < dc.LEVELS else np.asarray(c["pose_init"], np.float64)
        m = model_pass(c, lv, start[lv], pred)
        d = _direct(c, lv, start[lv], pred)
        assert m["covered"].all()  # T = 10: every tile runs the pass, every point is published once
        assert np.array_equal(m["uc"], d["uc"]) and np.array_equal(m["vc"], d["vc"])
        assert np.array_equal(m["q"][:, 2:], d["J"])
        assert np.array_equal(m["cls"], d["cls"])
        live = m["cls"] != CLS_OUT
        assert np.array_equal(m["fu"][live], d["fu"][live]) and np.array_equal(m["fv"][live], d["fv"][live])
        sh = m["cls"] == CLS_SHARED
        xx, yy = d["uc"] - np.floor(d["uc"]), d["vc"] - np.floor(d["vc"])
        wts = np.stack([(1 - xx) * (1 - yy), xx * (1 - yy), (1 - xx) * yy, xx * yy], 1)
        assert np.array_equal(m["s"][sh], wts[sh])
        assert np.array_equal(m["s"][~sh][:, 0], d["uc"][~sh]) and np.array_equal(m["s"][~sh][:, 1], d["vc"][~sh])
        # against the census: `good` is the `last` side and the pass's side
        cen = dc.classify_level(c, lv, start[lv], pred)
        ws, hs = dc.level_dims(c["w"], c["h"])
        ur, vr = dc._project(c["pose_last"], c["K"], np.asarray(c["points"]), dc.SCALES[lv])
        ref_ok = dc._inside(ur - 4, vr - 4, ws[lv], hs[lv]) & dc._inside(ur + 4, vr + 4, ws[lv], hs[lv])
        assert np.array_equal(ref_ok & live, cen["good"])
        # and its classes where its clamped window origin is the kernel's
        same = cen["good"] & d["on"] & (d["x0"] == np.clip(d["x0"], 0, max(ws[lv] - dc.WIN, 0))) & \
            (d["y0"] == np.clip(d["y0"], 0, max(hs[lv] - dc.WIN, 0)))
        compared += int(same.sum())
        for name, code in (("shared", CLS_SHARED), ("straddle", CLS_STRADDLE), ("per_sample", CLS_SAMPLE)):
            assert np.array_equal(cen[name][same], (m["cls"] == code)[same]), (lv, name)
        seen |= set(np.unique(m["cls"][ref_ok]).tolist())
    # (the window is not clamped, so this pair's small steps leave no point to sample_cw: big_step_t10 below)
    assert seen == {CLS_OUT, CLS_SHARED, CLS_STRADDLE}
    assert compared > n  # (small levels clamp most windows; levels 0 and 1 carry the comparison)


def test_model_applies_the_tile_rule_per_workgroup():
    """Split tiling (tile_range with `split`) gives workgroups of different
    counts within one map: the pass runs in those of 9 and 10 points only."""
    start, _, _ = dc.walk_levels(dc.case("gentle"))
    for n, counts in ((2465, {9, 10}), (2300, {8, 9}), (2700, {10, 11})):
        c = dc.sweep_case(n)
        tiles = _tiles(n, True)
        assert {t for _, t in tiles} == counts
        want = np.zeros(n, bool)
        for f, t in tiles:
            want[f:f + t] = 8 < t <= 10
        m = model_pass(c, 0, start[0], start[1], split=True)
        assert np.array_equal(m["covered"], want) and 0 < want.sum()
        d = _direct(c, 0, start[0], start[1])
        assert np.array_equal(m["uc"][want], d["uc"][want]) and np.array_equal(m["cls"][want], d["cls"][want])
    # the canonical tiling: all or nothing
    for n in N_ON:
        assert model_pass(dc.sweep_case(n), 0, start[0], start[1])["covered"].all()
    for n in N_OFF:
        assert not model_pass(dc.sweep_case(n), 0, start[0], start[1])["covered"].any()


# ------------------------------------------------------------------ GPU, stage
_ctx: dict = {}


def _context(K, on):
    """A context created with the switch set (the library reads it then)."""
    import viso_amd
    key = (tuple(K), on)
    if key not in _ctx:
        old = os.environ.get(SWITCH)
        os.environ[SWITCH] = "1" if on else "0"
        try:
            _ctx[key] = viso_amd.Context(viso_amd.default_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3]))
        finally:
            if old is None:
                del os.environ[SWITCH]
            else:
                os.environ[SWITCH] = old
    return _ctx[key]


def _rel_frob(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _stage(key, on):
    c = _get(key)
    return _context(c["K"], on).direct_pose(c["last"], c["cur"], c["w"], c["h"], c["points"], c["pose_last"],
                                            c["pose_init"])


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(N_ON) + list(N_OFF) + list(NAMED) + ["big_step_t10"])
def test_gpu_stage_matches_oracle_and_the_switch_changes_no_bit(key):
    exp = _oracle_pose(key)
    got = _stage(key, True)
    rel = _rel_frob(got, exp)
    print(f"direct pose {key}: rel Frobenius {rel:.3e} (bar 1e-12)")
    assert np.isfinite(got).all() and rel < 1e-12, f"{key}: rel {rel:.3e}"
    off = _stage(key, False)
    assert np.array_equal(got, off), (key, _rel_frob(got, off))


# ------------------------------------------------------------------ GPU, pipeline
_PIPE = dict(W=1242, H=375, n=9)


def _pipeline_gpu(left, right, seq, on, monkeypatch):
    import torch

    import viso_amd
    W, H, n = _PIPE["W"], _PIPE["H"], _PIPE["n"]
    monkeypatch.setenv(SWITCH, "1" if on else "0")
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    torch.cuda.synchronize()
    v = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=16, max_poses=64)
    v.set_stereo(seq.p.baseline, 128, 1)
    v.set_frame_log(True)
    v.process_device(dl.data_ptr(), dr.data_ptr(), n, W * H)  # one call: initialisation + 8 tracking frames
    v.synchronize()
    assert v.state == 1
    out = (v.poses, v.GetPoints(), v.frame_log(), v.alignment())
    v.close()
    return out


@pytest.mark.gpu
def test_gpu_pipeline_one_ingest_call_matches_oracle_and_the_switch_changes_no_bit(monkeypatch):
    from viso_amd.synth import Sequence
    W, H, n = _PIPE["W"], _PIPE["H"], _PIPE["n"]
    seq = Sequence(W, H, seed=0)
    left = np.stack([seq.image(f, 0) for f in range(n)])
    right = np.stack([seq.image(f, 1) for f in range(n)])
    gP, gp, glog, gal = _pipeline_gpu(left, right, seq, True, monkeypatch)
    ov = oracle_lib.Viso(seq.K, W, H, enable_tracking=1)
    ov.set_stereo(seq.p.baseline, 128, 1)
    ov.on_new_stereo(left[0], right[0])
    olog = []
    for f in range(1, n):
        ov.on_new_frame(left[f])
        s = ov.stats()
        olog.append((s[9], s[10]))
    olog = np.array(olog)
    oP, op = ov.poses(), ov.points()
    assert ov.state == 1 and np.array_equal(gp, op)
    assert 8 < dc.map_tile(len(op)) <= 10, len(op)  # the map's tiles run the pass
    assert gP.shape == oP.shape == (n - 1, 12)
    rel = np.linalg.norm(gP - oP, axis=1) / np.linalg.norm(oP, axis=1)
    print(f"pipeline, {n - 1} tracking frames, {len(op)} points: poses rel max {rel.max():.3e} (bar 1e-10)")
    assert rel.max() <= 1e-10
    assert np.array_equal(glog[:, 0], olog[:, 0]), np.nonzero(glog[:, 0] != olog[:, 0])
    assert (olog[:, 0] > 0).all()
    pk, sc, ub, ua = gal
    opk, osc, oub, oua = ov.alignment()
    assert np.array_equal(pk, opk) and np.array_equal(sc, osc) and len(pk) > 0
    print(f"  level-0 cost: max |gpu - oracle| {np.abs(glog[:, 1] - olog[:, 1]).max():.3e}; last alignment: "
          f"{len(pk)} pairs, max |uv_before| diff {np.abs(ub - oub).max():.3e}, |uv_after| diff "
          f"{np.abs(ua - oua).max():.3e}")
    assert np.array_equal(glog[:, 1], olog[:, 1])
    assert np.array_equal(ub, oub) and np.array_equal(ua, oua)
    # the switch at 0: the same bits everywhere
    fP, fp, flog, fal = _pipeline_gpu(left, right, seq, False, monkeypatch)
    assert np.array_equal(gP, fP) and np.array_equal(gp, fp) and np.array_equal(glog, flog)
    for a, b in zip(gal, fal):
        assert np.array_equal(a, b)
