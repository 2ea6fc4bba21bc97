"""The direct pose's level partials in the paired layout [14][4][2][64]
(viso_amd/csrc/direct.hip: partial_index, load_partials_paired): element
[k][w][h][j] is sum k + 14 h of tile 64 w + j, so one paired load instruction
of the next launch's prologue reads one contiguous 1 KB run per wave.  The
tile phase of direct_level_kernel writes that layout, the prologue of L(2..0),
of the merged L(3) and of F reads it; the continuation's scratch and the rig's
stay k-major.

Context.direct_pose is held to the oracle (relative Frobenius < 1e-12, the
stage's bar) and to the parent commit's bits
(tests/golden/direct_partials_parent.npz, recorded with the library of the
commit before the layout change by tests/golden/make_direct_partials.py) on

* 1, 2, 3 and 5 tiles: the unpaired last tile and a half-empty pair;
* every wave edge of the 256-thread loader: 63, 64, 65 tiles (dc.make cases of
  one point per tile: the product's tiling, T = ceil(n / 256), gives a tile
  of more than one point only from 129 tiles on), 129 tiles of two points
  (n = 258; n = 257 is 129 tiles with a one-point last tile), and 255, 256,
  257 points of the tile sweep;
* a case that takes the cost == 0 continuation (the current image is the last
  one, so every residual is 0 and cost / lastCost is 0 / 0): the k-major
  continuation scratch and the paired level scratch meet in one launch;
* a two-frame process_device call after a three-frame one: the merged L(3) of
  the second frame and the standalone F launch both read the paired layout.
  The frame path is held to the parent's bits and to the oracle at the frame
  path's bar (1e-10, tests/test_stereo_init.py).
"""
import os

import numpy as np
import pytest

from tests import direct_cases as dc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "direct_partials_parent.npz")
SMALL = (1, 2, 3, 5)
EDGE_MAKE = (63, 64, 65, 258)
EDGE_SWEEP = (255, 256, 257)
REPEAT_N = 65
KEYS = tuple(f"n{n}" for n in SMALL + EDGE_MAKE + EDGE_SWEEP) + ("repeat",)
FRAMES = 5  # 3 + 2


def make_cases():
    out = {}
    w, h, shift, seed, scale, near = dc.SWEEP_ARGS
    for n in SMALL + EDGE_MAKE:
        out[f"n{n}"] = dc.make(w, h, shift, n, seed, scale, near)
    for n in EDGE_SWEEP:
        out[f"n{n}"] = dc.get(n)
    out["repeat"] = dc.make(w, h, (0, 0), REPEAT_N, seed, scale, near)
    return out


@pytest.fixture(scope="module")
def cases():
    return make_cases()


def n_tiles(n):
    t = dc.map_tile(n)
    return (n + t - 1) // t


def test_tile_counts():
    assert [n_tiles(n) for n in SMALL] == [1, 2, 3, 5]
    assert [(n_tiles(n), dc.map_tile(n)) for n in EDGE_MAKE] == [(63, 1), (64, 1), (65, 1), (129, 2)]
    assert [(n_tiles(n), dc.map_tile(n)) for n in EDGE_SWEEP] == [(255, 1), (256, 1), (129, 2)]


def test_repeat_case_continues_with_zero_cost(cases):
    """The oracle's level statistics of the repeat case: cost exactly 0 with
    good points at every level (the loop's 0 / 0 keeps it going)."""
    c = cases["repeat"]
    assert np.array_equal(c["last"], c["cur"])
    _, stats, pose = dc.walk_levels(c)
    for lv in range(dc.LEVELS):
        assert stats[lv][0] > 0 and stats[lv][1] == 0.0, (lv, stats[lv][:2])
    assert np.isfinite(pose).all()


_oracle: dict = {}


def oracle_pose(c, key):
    if key not in _oracle:
        from tests import oracle_lib
        _oracle[key] = oracle_lib.direct_pose(c["last"], c["cur"], c["w"], c["h"], c["K"], c["points"],
                                              c["pose_last"], c["pose_init"])
    return _oracle[key]


def direct_pose(c):
    import viso_amd
    ctx = viso_amd.default_context(K=c["K"])
    return ctx.direct_pose(c["last"], c["cur"], c["w"], c["h"], c["points"], c["pose_last"], c["pose_init"])


def two_frame_poses():
    """(poses of the batched run: frames 0..2 in one process_device call, then
    frames 3 and 4 in a two-frame call; the lefts / rights used)."""
    import torch

    import viso_amd
    from tests import seqdata
    W, H = seqdata.W, seqdata.H
    lefts = np.stack([seqdata.image(f) for f in range(FRAMES)])
    rights = np.stack([seqdata.image(f, cam=1) for f in range(FRAMES)])
    seq = seqdata.sequence(0)
    dl = torch.from_numpy(lefts).cuda()
    dr = torch.from_numpy(rights).cuda()
    torch.cuda.synchronize()
    v = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=3)
    v.set_stereo(seq.p.baseline, 128, 1)
    v.process_device(dl.data_ptr(), dr.data_ptr(), 3, W * H)
    v.process_device(dl.data_ptr() + 3 * W * H, dr.data_ptr() + 3 * W * H, 2, W * H)
    v.synchronize()
    assert v.state == 1
    return np.ascontiguousarray(v.poses, np.float64), lefts, rights


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_gpu_direct_pose_against_oracle_and_parent_bits(key, cases):
    c = cases[key]
    exp = oracle_pose(c, key)
    got = np.ascontiguousarray(direct_pose(c), np.float64).reshape(12)
    with np.load(GOLDEN) as g:
        par = g[key]
    rel = _rel(got, exp)
    diff = np.flatnonzero(got.view(np.uint64) != par)
    print(f"direct pose {key}: rel Frobenius vs oracle {rel:.3e} (bar 1e-12); {len(diff)} of 12 doubles differ "
          f"from the parent's bits")
    assert np.isfinite(got).all() and rel < 1e-12, (key, rel)
    assert len(diff) == 0, (key, [(int(i), hex(int(got.view(np.uint64)[i])), hex(int(par[i]))) for i in diff])


@pytest.mark.gpu
def test_gpu_two_frame_call_against_oracle_and_parent_bits():
    from tests import oracle_lib, seqdata
    got, lefts, rights = two_frame_poses()
    seq = seqdata.sequence(0)
    ov = oracle_lib.Viso(seq.K, seqdata.W, seqdata.H, enable_tracking=1)
    ov.set_stereo(seq.p.baseline, 128, 1)
    for k in range(FRAMES):
        ov.on_new_stereo(lefts[k], rights[k])
    exp = ov.poses()
    with np.load(GOLDEN) as g:
        par = g["two_frame"]
    assert got.shape == exp.shape and len(exp) == FRAMES - 1
    rel = _rel(got, exp)
    ndiff = int((got.view(np.uint64).ravel() != par.ravel()).sum())
    print(f"two-frame call: rel Frobenius vs oracle {rel:.3e} (bar 1e-10); {ndiff} of {got.size} doubles differ "
          f"from the parent's bits")
    assert rel < 1e-10
    assert ndiff == 0
