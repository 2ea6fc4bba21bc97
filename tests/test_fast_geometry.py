"""FAST stage parity (viso_fast against the C++ oracle) at the edges of the
device detector's fixed geometry (viso_amd/csrc/image.hip): tile seams every
126 columns, band seams every 8 rows, last tiles and bands that hold only
border pixels, the minimum size, 33 tiles per row (widths above 4032), full
64-keypoint slots, a candidate list drained twice in a row, the capacity
argument and a reused scratch block.

Everything is integer: x, y, score, count and order are compared exactly.
tests/test_fast_patterns.py pins on the CPU that the crafted images
(tests/fast_patterns.py) reach these edges."""
import ctypes

import numpy as np
import pytest

from tests import fast_patterns as fp
from tests import images, oracle_lib

pytestmark = pytest.mark.gpu


def _gpu_fast(ctx, img, thresh, cap=1 << 20):
    """viso_fast: (xs, ys, scores) of min(n, cap) corners, and n."""
    from viso_amd import _lib
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    m = max(cap, 1)
    xs, ys, sc = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.full(m, -1, np.int32)
    n = ctypes.c_size_t(0)
    _lib.call("viso_fast", ctx.h, img.ctypes.data, w, h, thresh, xs.ctypes.data, ys.ctypes.data, sc.ctypes.data,
              cap, ctypes.byref(n))
    k = min(int(n.value), cap)
    assert np.all(xs[k:] == -1) and np.all(ys[k:] == -1) and np.all(sc[k:] == -1)  # nothing past the prefix
    return (xs[:k].copy(), ys[:k].copy(), sc[:k].copy()), int(n.value)


def _check(ctx, img, thresh, exp=None, ref_thresh=None):
    exp = oracle_lib.fast(img, thresh if ref_thresh is None else ref_thresh) if exp is None else exp
    got, n = _gpu_fast(ctx, img, thresh)
    assert n == len(exp[0])
    for name, g, e in zip("xys", got, exp):
        assert np.array_equal(g, e), name
    return exp


@pytest.fixture(scope="module")
def ctx():
    from viso_amd import default_context
    return default_context()


# ------------------------------------------------------------------ geometry sweep
@pytest.mark.parametrize("h,w", fp.SWEEP)
def test_gpu_fast_seam_sweep(ctx, h, w):
    img, keep, _ = fp.seams(h, w)
    exp = oracle_lib.fast(img, fp.SEAM_THRESH)
    # the reference meets the case's condition (pinned on the CPU as well)
    assert len(exp[0]) > 0 and all(np.array_equal(a, b) for a, b in zip(exp, fp.as_arrays(keep)))
    if (h, w) in fp.SMALLEST:
        assert keep == fp.SMALLEST[(h, w)]
    else:
        assert exp[0].min() == 3 and exp[0].max() == w - 4 and exp[1].min() == 3 and exp[1].max() == h - 4
    _check(ctx, img, fp.SEAM_THRESH, exp)


@pytest.mark.parametrize("x,y", [(3, 3), (4, 3), (3, 4), (4, 4)])
def test_gpu_fast_minimum_size(ctx, x, y):
    img = np.full((8, 8), 230, np.uint8)
    img[y, x] = 10
    exp = _check(ctx, img, 50)
    assert [tuple(int(v[0]) for v in exp)] == [(x, y, 219)]


def test_gpu_fast_minimum_size_noise(ctx):
    for seed in range(8):
        _check(ctx, images.noise(8, 8, seed=seed), 0)
        _check(ctx, images.noise(9, 8, seed=seed), 0)
        _check(ctx, images.noise(8, 9, seed=seed), 0)


# ------------------------------------------------------------------ natural images at odd widths
@pytest.mark.parametrize("thresh", [0, 1, 20, 254])
@pytest.mark.parametrize("h,w", [(43, 381), (37, 255), (19, 4033)])
@pytest.mark.parametrize("kind", ["mixed", "noise"])
def test_gpu_fast_odd_widths(ctx, kind, h, w, thresh):
    exp = _check(ctx, getattr(images, kind)(h, w, seed=5), thresh)
    assert (len(exp[0]) > 0) == (thresh < 254)


# ------------------------------------------------------------------ dense cases
@pytest.mark.parametrize("x0", [0, 1])
def test_gpu_fast_full_slots(ctx, x0):
    h, w = fp.DENSE_SHAPE
    exp = _check(ctx, fp.full_slots(h, w, x0), fp.FULL_SLOT_THRESH)
    assert fp.slot_counts(exp[0], exp[1], h, w).max() == fp.SLOT_CAP - 1


@pytest.mark.parametrize("h,w,phase", [fp.DENSE_SHAPE + (0,), fp.DENSE_SHAPE + (1,), (19, 4096, 0), (19, 4096, 1)])
def test_gpu_fast_full_candidate_rows(ctx, h, w, phase):
    img = fp.full_rows(h, w, 1, phase=phase)
    assert fp.window_counts(fp.score_map(img, fp.FULL_ROW_THRESH)).max() == 128
    exp = _check(ctx, img, fp.FULL_ROW_THRESH)
    assert len(exp[0]) > 1000 and len(set(exp[2].tolist())) > 8
    if (w, phase) == (4096, 1):  # the band's (row, tile) slots past 256 hold corners
        assert fp.slot_counts(exp[0], exp[1], h, w)[:8].reshape(-1)[256:].min() > 0


# ------------------------------------------------------------------ threshold clamp
@pytest.mark.parametrize("thresh,clamped", [(-7, 0), (300, 255)])
def test_gpu_fast_threshold_clamp(ctx, thresh, clamped):
    img = images.mixed(37, 255, seed=5)
    exp = _check(ctx, img, thresh, ref_thresh=clamped)
    assert (len(exp[0]) > 0) == (clamped == 0)


# ------------------------------------------------------------------ capacity
def test_gpu_fast_capacity(ctx):
    """The returned prefix is the reference's, and n the uncapped total."""
    h, w = fp.DENSE_SHAPE
    img = fp.full_slots(h, w, 0)
    exp = oracle_lib.fast(img, fp.FULL_SLOT_THRESH)
    total = len(exp[0])
    first_band = int((exp[1] < 8).sum())
    assert 63 < first_band < total - 1  # (30 is inside the first (row, tile) slot of 63)
    for cap in [1, 30, first_band, total - 1, total, total + 1]:
        got, n = _gpu_fast(ctx, img, fp.FULL_SLOT_THRESH, cap)
        assert n == total
        assert len(got[0]) == min(cap, total)
        for g, e in zip(got, exp):
            assert np.array_equal(g, e[:cap]), cap


# ------------------------------------------------------------------ scratch reuse
def test_gpu_fast_scratch_reuse():
    """cnt / tot / lst live in a scratch block that is reused, not cleared:
    a sparse image after a dense one, and other sizes after it, in one
    context."""
    from viso_amd.api import Context
    h, w = fp.DENSE_SHAPE
    with Context(width=w, height=h) as c:
        assert len(_check(c, fp.full_slots(h, w, 0), fp.FULL_SLOT_THRESH)[0]) == 1683
        assert len(_check(c, np.full((h, w), 230, np.uint8), fp.FULL_SLOT_THRESH)[0]) == 0
        assert len(_check(c, fp.seams(h, w)[0], fp.SEAM_THRESH)[0]) == len(fp.seams(h, w)[1]) > 0
        assert len(_check(c, fp.seams(19, 131)[0], fp.SEAM_THRESH)[0]) > 0
        assert len(_check(c, fp.full_rows(19, 131, 1), fp.FULL_ROW_THRESH)[0]) > 0
        assert len(_check(c, fp.seams(33, 4096)[0], fp.SEAM_THRESH)[0]) > 0
        _check(c, fp.full_slots(h, w, 1), fp.FULL_SLOT_THRESH)
