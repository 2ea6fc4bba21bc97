"""Host model of the direct pose's current-image window and of the branch a
point takes on it (viso_amd/csrc/direct.hip win_issue / direct_point_rs /
sample_cw).

The 20 x 20 window is a window of the level's continuous buffer: origin
(x0, y0) = (floor(up), floor(vp)) - 9 for the projection (up, vp) under the
predicted pose, not clamped to the image, byte (r, c) =
buf[(y0 + r) w + x0 + c] or 0 outside the buffer.  This checks, for patches at
and next to every border of the image (the input classes edge_lt / edge_r /
edge_b of tests/direct_cases.py, which after this change take the whole-patch
kernel branches), that

* for a prediction that is off by -3..+4 px the whole-patch test holds and
  every one of the patch's 5 x 64 samples, read from the window, equals
  GetPixelValue (include/common.h:35-42: int() base, floor() weights, taps
  outside the continuous buffer read 0) bit for bit;
* the shared-weights branch is never chosen when any sample coordinate is
  negative (int() != floor() in (-1, 0)), and where it is chosen its five
  values equal the per-sample ones;
* for a prediction that is off by more, whatever sample_cw still serves from
  the window equals GetPixelValue.
"""
import numpy as np

WIN = 20
PX = np.array([(l >> 3) - 4 for l in range(64)], np.float64)
PY = np.array([(l & 7) - 4 for l in range(64)], np.float64)
# the five samples of a lane: value, x + 1, x - 1, y + 1, y - 1
FIVE = ((0.0, 0.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0))


def _taps(buf, n, idx):
    ok = (idx >= 0) & (idx < n)
    return np.where(ok, buf[np.clip(idx, 0, n - 1)], 0).astype(np.float64)


def _bilinear(x, y, d0, d1, d2, d3):
    xx, yy = x - np.floor(x), y - np.floor(y)
    return (1 - xx) * (1 - yy) * d0 + xx * (1 - yy) * d1 + (1 - xx) * yy * d2 + xx * yy * d3


def _get_pixel(buf, w, h, x, y):
    n = w * h
    base = np.trunc(y).astype(np.int64) * w + np.trunc(x).astype(np.int64)
    return _bilinear(x, y, _taps(buf, n, base), _taps(buf, n, base + 1), _taps(buf, n, base + w),
                     _taps(buf, n, base + w + 1))


def _window(buf, w, h, x0, y0):
    idx = (y0 + np.arange(WIN))[:, None] * w + x0 + np.arange(WIN)[None, :]
    return _taps(buf, w * h, idx)


def _served(x0, y0, x, y):
    """sample_cw's test: all four taps of the sample lie in the window."""
    ix, iy = np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64)
    return (ix >= x0) & (ix + 1 < x0 + WIN) & (iy >= y0) & (iy + 1 < y0 + WIN)


def _win_sample(win, x0, y0, x, y):
    """The per-sample form (direct_point_rs `smp`, sample_cw): int() base."""
    c, r = np.trunc(x).astype(np.int64) - x0, np.trunc(y).astype(np.int64) - y0
    return _bilinear(x, y, win[r, c], win[r, c + 1], win[r + 1, c], win[r + 1, c + 1])


def _binade(v):
    return np.float64(v).view(np.int64) >> 52


def _whole(uc, vc, x0, y0):
    fu, fv = int(np.floor(uc)), int(np.floor(vc))
    return fu - 6 >= x0 and fu + 5 <= x0 + WIN - 2 and fv - 6 >= y0 and fv + 5 <= y0 + WIN - 2


def _shared(uc, vc):
    return bool(uc >= 6.0 and vc >= 6.0 and _binade(uc - 6.0) == _binade(uc + 6.0)
                and _binade(vc - 6.0) == _binade(vc + 6.0))


def _shared_samples(win, x0, y0, uc, vc):
    """The shared-weights branch: floor() bases, one set of weights."""
    fu, fv = int(np.floor(uc)), int(np.floor(vc))
    xx, yy = uc - np.floor(uc), vc - np.floor(vc)
    w00, w10, w01, w11 = (1 - xx) * (1 - yy), xx * (1 - yy), (1 - xx) * yy, xx * yy
    c0, r0 = fu + PX.astype(np.int64) - x0, fv + PY.astype(np.int64) - y0
    out = []
    for dx, dy in FIVE:
        c, r = c0 + int(dx), r0 + int(dy)
        out.append(w00 * win[r, c] + w10 * win[r, c + 1] + w01 * win[r + 1, c] + w11 * win[r + 1, c + 1])
    return out


def _centres(rng, w, h):
    cs = [(rng.uniform(4, w - 4), rng.uniform(4, h - 4)) for _ in range(400)]
    eps = 1e-9
    lo, xr, yb = 4.0, w - 4 - eps, h - 4 - eps
    cs += [(lo, lo), (xr, lo), (lo, yb), (xr, yb)]                      # the corners
    cs += [(4.5, 20.3), (4.999, 4.25), (17.7, 4.5)]                     # a tap coordinate in (-1, 0)
    cs += [(w - 4.75, 20.3), (w - 5.0, 9.5)]                            # tap column w: the next row
    cs += [(w - 4.5, h - 4.5), (w - 4.25, h - 5.0), (30.2, h - 4.125)]  # index reaches w h: zero taps
    cs += [(40.25, 24.5), (75.0, 23.125)]                               # one binade in both axes
    return cs


def test_buffer_window_serves_getpixelvalue_at_every_border():
    rng = np.random.default_rng(11)
    w, h = 97, 41
    buf = rng.integers(0, 256, w * h).astype(np.uint8)
    n_shared = n_neg = n_wrap = n_zero = 0
    for uc, vc in _centres(rng, w, h):
        fu, fv = int(np.floor(uc)), int(np.floor(vc))
        xs = [uc + PX + dx for dx, _ in FIVE]
        ys = [vc + PY + dy for _, dy in FIVE]
        exp = [_get_pixel(buf, w, h, x, y) for x, y in zip(xs, ys)]
        negative = min(x.min() for x in xs) < 0 or min(y.min() for y in ys) < 0
        n_neg += negative
        n_wrap += fu + 5 >= w
        n_zero += (fv + 5 >= h) and (fu + 5 >= w)
        offs = [(d, d) for d in range(-3, 5)] + [(-3, 4), (4, -3), (0, 4), (-3, 0)]
        for ox, oy in offs:  # floor(uc) - floor(up), floor(vc) - floor(vp)
            x0, y0 = fu - ox - 9, fv - oy - 9
            win = _window(buf, w, h, x0, y0)
            assert _whole(uc, vc, x0, y0), (uc, vc, ox, oy)
            per = []
            for x, y, e in zip(xs, ys, exp):
                assert _served(x0, y0, x, y).all(), (uc, vc, ox, oy)
                got = _win_sample(win, x0, y0, x, y)
                assert np.array_equal(got, e), (uc, vc, ox, oy)
                per.append(got)
            if _shared(uc, vc):
                assert not negative, (uc, vc)
                for got, e in zip(_shared_samples(win, x0, y0, uc, vc), per):
                    assert np.array_equal(got, e), (uc, vc, ox, oy)
                n_shared += (ox, oy) == (0, 0)
        # a prediction that misses by more: sample_cw serves what it can
        for ox, oy in ((-5, 0), (6, 0), (0, -5), (0, 6), (-9, 7), (25, 25)):
            x0, y0 = fu - ox - 9, fv - oy - 9
            assert not _whole(uc, vc, x0, y0)
            win = _window(buf, w, h, x0, y0)
            for x, y, e in zip(xs, ys, exp):
                s = _served(x0, y0, x, y)
                if s.any():
                    assert np.array_equal(_win_sample(win, x0, y0, x[s], y[s]), e[s]), (uc, vc, ox, oy)
    # the inputs reach what they are here for
    assert n_shared >= 10 and n_neg >= 10 and n_wrap >= 10 and n_zero >= 3, (n_shared, n_neg, n_wrap, n_zero)


def test_shared_branch_needs_non_negative_coordinates():
    """floor() bases differ from int() bases exactly when a coordinate lies in
    (-1, 0): uc in (4, 5) puts the left gradient sample of the patch's first
    column there, and the explicit uc >= 6 keeps such a point (and every
    point whose uc - 6 is negative) out of the shared branch."""
    for uc in (4.0, 4.5, 4.999, 5.0, 5.5, 5.999):
        assert not _shared(uc, 30.0) and not _shared(30.0, uc)
    assert _shared(40.0, 24.0)
    x = np.array([4.5 - 4 - 1])  # uc = 4.5, px = -4, the x - 1 sample
    assert np.trunc(x)[0] == 0 and np.floor(x)[0] == -1
