"""CPU pins of the crafted FAST images (tests/fast_patterns.py) and of the
frame-path references, on the oracle alone: each pattern must reach the edge
of the device detector it is built for.  The GPU cases of
tests/test_fast_geometry.py and tests/test_fast_frame_path.py rest on these."""
import numpy as np
import pytest

from oracle import numpy_ref as nr
from tests import fast_patterns as fp
from tests import images, oracle_lib

SWEEP, SMALLEST = fp.SWEEP, fp.SMALLEST


def _same(got, exp):
    return len(got[0]) == len(exp[0]) and all(np.array_equal(g, e) for g, e in zip(got, exp))


# ------------------------------------------------------------------ seams
@pytest.mark.parametrize("h,w", SWEEP + [fp.DENSE_SHAPE, (43, 253)])
def test_seam_survivors_match_oracle(h, w):
    """The oracle keeps exactly the hand-derived survivors: the deeper dot of
    an adjacent pair, neither of an equal pair, nothing outside the candidate
    range; and the list touches the first and last candidate column and row."""
    img, keep, groups = fp.seams(h, w)
    exp = fp.as_arrays(keep)
    got = oracle_lib.fast(img, fp.SEAM_THRESH)
    assert _same(got, exp)
    assert len(keep) > 0 and exp[2].min() >= fp.SEAM_THRESH  # (every dot is deeper than the threshold)
    if (h, w) in SMALLEST:
        assert keep == SMALLEST[(h, w)]
    else:
        assert exp[0].min() == 3 and exp[0].max() == w - 4 and exp[1].min() == 3 and exp[1].max() == h - 4
    # dots in column 2 / w - 3 and row 2 / h - 3 are in the image, and not reported
    kinds = [k for k, _ in groups]
    if min(h, w) >= 12:
        assert kinds.count("outside") >= 2
    assert np.all((exp[0] >= 3) & (exp[0] <= w - 4) & (exp[1] >= 3) & (exp[1] <= h - 4))


def test_seam_pattern_covers_every_seam():
    """Every tile seam and band seam inside the candidate range carries the
    three kinds of pair (the pair on both seams stands for the diagonal of its
    tile seam), at the sizes with room for them."""
    for h, w in [(19, 4096), (19, 4033), (19, 379), fp.DENSE_SHAPE, (33, 131)]:
        _, _, groups = fp.seams(h, w)
        tile = [X for X in range(126, w, 126) if X <= w - 4]
        band = [Y for Y in range(8, h, 8) if Y <= h - 4]
        assert ("both", ()) in groups
        for kind in ("tile-deeper", "tile-equal", "tile-diagonal"):
            have = [key[0] for k, key in groups if k == kind]
            # (the seam under the pair on both seams has that pair for its diagonal)
            missing = [X for X in tile if X not in have]
            assert len(missing) <= (1 if kind == "tile-diagonal" else 0), (h, w, kind, missing)
        for kind in ("band-deeper", "band-equal", "band-diagonal"):
            assert [key[0] for k, key in groups if k == kind] == band, (h, w, kind)
    # 19 x 4096: 32 tile seams (ntx = 33), each with a deeper and an equal pair
    _, keep, groups = fp.seams(19, 4096)
    assert [k for k, _ in groups].count("tile-deeper") == 32 and [k for k, _ in groups].count("tile-equal") == 32
    assert max(x for x, _, _ in keep) // 126 == 32


def test_seam_survivors_match_numpy_restatement():
    img, keep, _ = fp.seams(19, 131)
    assert _same(nr.fast(img, fp.SEAM_THRESH), fp.as_arrays(keep))
    assert _same(oracle_lib.fast(img, fp.SEAM_THRESH), fp.as_arrays(keep))


@pytest.mark.parametrize("x,y", [(3, 3), (4, 3), (3, 4), (4, 4)])
def test_minimum_size_single_dot(x, y):
    """8 x 8 has candidate columns and rows 3 and 4 only; a dot of 10 on 230 is
    reported with score 230 - 10 - 1 = 219."""
    img = np.full((8, 8), 230, np.uint8)
    img[y, x] = 10
    assert [tuple(int(v[0]) for v in oracle_lib.fast(img, 50))] == [(x, y, 219)]
    assert _same(nr.fast(img, 50), oracle_lib.fast(img, 50))


# ------------------------------------------------------------------ density
@pytest.mark.parametrize("x0,total", [(0, 1683), (1, 1692)])
def test_full_slots_reach_63(x0, total):
    h, w = fp.DENSE_SHAPE
    xs, ys, sc = oracle_lib.fast(fp.full_slots(h, w, x0), fp.FULL_SLOT_THRESH)
    c = fp.slot_counts(xs, ys, h, w)
    assert c.max() == fp.SLOT_CAP - 1
    assert len(xs) == total and sc.min() >= 80 and sc.max() <= 229


def test_no_pattern_exceeds_63_per_slot():
    """Strict NMS keeps at most one of two adjacent pixels, so at most 63 of a
    tile's 126 columns: the argument the 64-entry slot rests on, checked on
    the images of the GPU modules."""
    h, w = fp.DENSE_SHAPE
    cases = [(fp.full_slots(h, w, 0), 50), (fp.full_slots(h, w, 1), 50), (fp.full_rows(h, w, 1), 10),
             (fp.full_rows(19, 4096, 1, phase=1), 10), (fp.seams(h, w)[0], 50), (fp.seams(19, 4096)[0], 50)]
    for hh, ww in [(43, 381), (37, 255), (19, 4033)]:
        for kind in ("mixed", "noise"):
            cases += [(getattr(images, kind)(hh, ww, seed=5), t) for t in (0, 20)]
    for img, t in cases:
        xs, ys, _ = oracle_lib.fast(img, t)
        assert fp.slot_counts(xs, ys, *img.shape).max() <= fp.SLOT_CAP - 1


def test_full_rows_fill_the_candidate_list():
    h, w = fp.DENSE_SHAPE
    img = fp.full_rows(h, w, 1)
    wc = fp.window_counts(fp.score_map(img, fp.FULL_ROW_THRESH))
    xs, ys, sc = oracle_lib.fast(img, fp.FULL_ROW_THRESH)
    assert wc.max() >= 120
    assert len(xs) > 1000
    assert len(set(sc.tolist())) > 8
    # (this seed: all 128 columns of the window in 18 (row, tile) windows,
    # 2094 corners, 16 distinct scores)
    assert wc.max() == 128 and len(xs) == 2094 and len(set(sc.tolist())) == 16
    # the natural images stay far below: one 64-batch at a time
    n = fp.window_counts(fp.score_map(images.noise(h, w, seed=5), 0))
    assert n.max() < 128


def test_full_rows_wide_fill_the_second_order_slot():
    """19 x 4096: ntx = 33, so a band has 8 * 33 = 264 > 256 (row, tile) slots;
    with the dense rows on the band's last row, the slots past 256 hold
    corners, and the candidate list is as full as at 43 x 381."""
    img = fp.full_rows(19, 4096, 1, phase=1)
    xs, ys, _ = oracle_lib.fast(img, fp.FULL_ROW_THRESH)
    c = fp.slot_counts(xs, ys, 19, 4096)
    assert c.shape[1] == 33
    band0, band1 = c[:8].reshape(-1), c[8:16].reshape(-1)
    assert band0[256:].min() > 0 and band1[256:].min() > 0 and band0[:256].sum() > 0
    assert fp.window_counts(fp.score_map(img, fp.FULL_ROW_THRESH)).max() == 128


# ------------------------------------------------------------------ frame path
K = (517.3, 516.5, 325.1, 249.7)


@pytest.mark.parametrize("h,w,n", [(43, 253, 270), (19, 129, 54)])
def test_oracle_viso_detection_frame_equals_fast(h, w, n):
    img = images.mixed(h, w, seed=4)
    xs, ys, _ = oracle_lib.fast(img, 20)
    assert len(xs) == n
    ov = oracle_lib.Viso(K, w, h, fast_thresh=20)
    ov.on_new_frame(img)
    k1, k2, s = ov.tracks()
    assert np.array_equal(k1, np.stack([xs, ys], 1).astype(np.float32))
    assert np.array_equal(k1, k2) and len(s) == n and not s.any()
