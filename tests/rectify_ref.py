"""TEST INFRASTRUCTURE ONLY — numpy restatement of the rectification rule
(viso_set_rectify / viso_rectify, include/viso/viso_c.h).  The
repo's own spec: no reference counterpart (src/main.cpp:14-17 hard-codes ideal
pinhole intrinsics).

Output image w x h with intrinsics K = (fx, fy, cx, cy); raw image rw x rh with
intrinsics Kr.  Every floating-point operation is an fp64 numpy operation of
its own, in the order the header states (the device is built with
-ffp-contract=off), so the device's bytes equal these.

The second half (``distort``, ``undistort``, ``warp_to_raw``) is NOT the rule:
it is the independent formula the geometry and usefulness tests build raw
images with."""
from __future__ import annotations

import numpy as np

OFF, RADTAN, TABLE = 0, 1, 2
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def radtan_coords(K, size, Kr, dist, R=IDENT):
    """(u, v, front): raw coordinates of every output pixel, and Z > 0."""
    w, h = size
    fx, fy, cx, cy = (np.float64(t) for t in K)
    fxr, fyr, cxr, cyr = (np.float64(t) for t in Kr)
    k1, k2, p1, p2, k3 = (np.float64(t) for t in dist)
    R = [np.float64(t) for t in np.asarray(R, np.float64).reshape(9)]
    two = np.float64(2.0)
    a = ((np.arange(w, dtype=np.float64) - cx) / fx)[None, :]
    b = ((np.arange(h, dtype=np.float64) - cy) / fy)[:, None]
    X = (R[0] * a + R[1] * b) + R[2]
    Y = (R[3] * a + R[4] * b) + R[5]
    Z = (R[6] * a + R[7] * b) + R[8]
    front = Z > 0
    with np.errstate(all="ignore"):
        xn = X / Z
        yn = Y / Z
        r2 = xn * xn + yn * yn
        xy = xn * yn
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = xn * rad + ((two * p1) * xy + p2 * (r2 + two * (xn * xn)))
        yd = yn * rad + (p1 * (r2 + two * (yn * yn)) + (two * p2) * xy)
        u = fxr * xd + cxr
        v = fyr * yd + cyr
    return u, v, front


def table_coords(table):
    """(u, v, front) of a TABLE map (h, w, 2) float32: widened to fp64."""
    t = np.asarray(table, np.float32)
    return t[..., 0].astype(np.float64), t[..., 1].astype(np.float64), np.ones(t.shape[:2], bool)


def sample(raw, u, v, front, fill):
    """The sampling rule.  Returns (out u8, outside mask, clipped mask)."""
    raw = np.asarray(raw, np.uint8)
    rh, rw = raw.shape
    with np.errstate(invalid="ignore"):
        inside = front & (u > -1) & (u < rw) & (v > -1) & (v < rh)  # a NaN compares false
    uu = np.where(inside, u, 0.0)
    vv = np.where(inside, v, 0.0)
    qu = np.floor(uu * 32 + 0.5).astype(np.int64)
    qv = np.floor(vv * 32 + 0.5).astype(np.int64)
    x0, ax = qu >> 5, qu & 31
    y0, ay = qv >> 5, qv & 31
    fill = int(fill)

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < rw) & (yy >= 0) & (yy < rh)
        val = raw[np.clip(yy, 0, rh - 1), np.clip(xx, 0, rw - 1)].astype(np.int64)
        return np.where(ok, val, fill), ok

    t00, o00 = tap(x0, y0)
    t01, o01 = tap(x0 + 1, y0)
    t10, o10 = tap(x0, y0 + 1)
    t11, o11 = tap(x0 + 1, y0 + 1)
    w00, w01, w10, w11 = (32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay
    val = (t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11 + 512) >> 10
    out = np.where(inside, val, fill).astype(np.uint8)
    tap_out = (~o00 & (w00 != 0)) | (~o01 & (w01 != 0)) | (~o10 & (w10 != 0)) | (~o11 & (w11 != 0))
    outside = ~inside
    return out, outside, outside | tap_out


def rectify(raw, K, size, model=RADTAN, fill=0, Kr=None, dist=(0, 0, 0, 0, 0), R=IDENT, table=None):
    """raw (rh, rw) or (n, rh, rw) u8 -> (out of the same rank, (outside, clipped))."""
    raw = np.asarray(raw, np.uint8)
    stack = raw if raw.ndim == 3 else raw[None]
    if model == TABLE:
        u, v, front = table_coords(table)
        assert u.shape == (size[1], size[0])
    else:
        u, v, front = radtan_coords(K, size, Kr, dist, R)
    outs = []
    for img in stack:
        out, outside, clipped = sample(img, u, v, front, fill)
        outs.append(out)
    counts = (int(outside.sum()), int(clipped.sum()))
    return (np.stack(outs) if raw.ndim == 3 else outs[0]), counts


# ---------------------------------------------------------------------------
# Not the rule: the independent forward / inverse lens formulas the tests build
# raw images with (the textbook Brown-Conrady model, written pointwise).
def distort(xn, yn, dist):
    """Ideal normalised coordinates -> distorted normalised coordinates."""
    k1, k2, p1, p2, k3 = dist
    r2 = xn ** 2 + yn ** 2
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return (xn * radial + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn ** 2),
            yn * radial + p1 * (r2 + 2 * yn ** 2) + 2 * p2 * xn * yn)


def undistort(xd, yd, dist, iters=60):
    """The inverse of `distort` by fixed-point iteration (converges for the
    mild distortions the tests use; the residual is asserted by the caller)."""
    k1, k2, p1, p2, k3 = dist
    x, y = np.array(xd, np.float64), np.array(yd, np.float64)
    for _ in range(iters):
        r2 = x ** 2 + y ** 2
        radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2)
        dy = p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
        x, y = (xd - dx) / radial, (yd - dy) / radial
    return x, y


def bilinear(img, x, y, fill=0.0):
    """Float bilinear sample of img at (x, y); `fill` outside."""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = x - x0, y - y0
    ok = (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
    x0c, y0c = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
    val = (img[y0c, x0c] * (1 - fx) * (1 - fy) + img[y0c, x0c + 1] * fx * (1 - fy) +
           img[y0c + 1, x0c] * (1 - fx) * fy + img[y0c + 1, x0c + 1] * fx * fy)
    return np.where(ok, val, fill)


def warp_to_raw(pinhole, K, Kr, raw_size, dist, fill=0):
    """The raw image a lens with `dist` would have delivered, from the pinhole
    image: every raw pixel's ideal ray by the iterative inverse, sampled
    bilinearly from `pinhole`."""
    rw, rh = raw_size
    u, v = np.meshgrid(np.arange(rw, dtype=np.float64), np.arange(rh, dtype=np.float64))
    xn, yn = undistort((u - Kr[2]) / Kr[0], (v - Kr[3]) / Kr[1], dist)
    val = bilinear(pinhole, K[0] * xn + K[2], K[1] * yn + K[3], fill)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)
