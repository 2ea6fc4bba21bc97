"""Rectification parameters and map helpers (viso_set_rectify / viso_rectify,
include/viso/viso_c.h).

``params(...)`` fills a ``viso_rectify_params``; ``radtan_map`` and
``equidistant_map`` make the float32 ``[h][w][2]`` tables of the TABLE model
on the host in numpy (a fisheye or any other lens goes through a table: the
device kernel then needs no transcendental function).
"""
from __future__ import annotations

import numpy as np

from . import _lib

OFF, RADTAN, TABLE = _lib.RECTIFY_OFF, _lib.RECTIFY_RADTAN, _lib.RECTIFY_TABLE
_IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def params(model: int = RADTAN, raw_size=None, fill: int = 0, K_raw=None, dist=(0.0, 0.0, 0.0, 0.0, 0.0), R=None,
           map=None):
    """A ``viso_rectify_params`` and the array that its ``map`` pointer needs
    alive (None for RADTAN).  raw_size = (raw_width, raw_height); K_raw = the raw
    image's (fx, fy, cx, cy); dist = (k1, k2, p1, p2, k3), OpenCV's order; R =
    9 or 3x3 row-major, rays of the rectified camera into the raw camera (the
    transpose of OpenCV's R1 / R2; default identity); map: TABLE's
    (h, w, 2) float32 coordinates."""
    p = _lib.viso_rectify_params()
    p.model = int(model)
    if raw_size is not None:
        p.raw_width, p.raw_height = int(raw_size[0]), int(raw_size[1])
    p.fill = int(fill)
    if K_raw is not None:
        p.fx, p.fy, p.cx, p.cy = (float(v) for v in K_raw)
    p.k1, p.k2, p.p1, p.p2, p.k3 = (float(v) for v in dist)
    r = np.asarray(_IDENT if R is None else R, np.float64).reshape(9)
    for i in range(9):
        p.R[i] = float(r[i])
    keep = None
    if map is not None:
        keep = np.ascontiguousarray(map, dtype=np.float32)
        if keep.ndim != 3 or keep.shape[2] != 2:
            raise ValueError("map must be (h, w, 2)")
        p.map = keep.ctypes.data
    return p, keep


def _rays(K_out, size_out, R):
    """Normalised raw-camera coordinates (xn, yn) and Z of every output pixel."""
    w, h = int(size_out[0]), int(size_out[1])
    fx, fy, cx, cy = (float(v) for v in K_out)
    r = np.asarray(_IDENT if R is None else R, np.float64).reshape(9)
    a = ((np.arange(w, dtype=np.float64) - cx) / fx)[None, :]
    b = ((np.arange(h, dtype=np.float64) - cy) / fy)[:, None]
    X = (r[0] * a + r[1] * b) + r[2]
    Y = (r[3] * a + r[4] * b) + r[5]
    Z = (r[6] * a + r[7] * b) + r[8]
    with np.errstate(divide="ignore", invalid="ignore"):
        return X / Z, Y / Z, Z


def _table(u, v, Z):
    m = np.stack([u, v], axis=-1)
    m[~(Z > 0)] = np.nan  # behind the raw camera: outside
    return m.astype(np.float32)


def radtan_map(K_out, size_out, K_raw, dist, R=None) -> np.ndarray:
    """The RADTAN model's coordinates as a TABLE map (float32: the table
    carries them rounded to 24 bits, the analytic model keeps fp64)."""
    xn, yn, Z = _rays(K_out, size_out, R)
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    fx, fy, cx, cy = (float(v) for v in K_raw)
    r2 = xn * xn + yn * yn
    xy = xn * yn
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = xn * rad + ((2 * p1) * xy + p2 * (r2 + 2 * (xn * xn)))
    yd = yn * rad + (p1 * (r2 + 2 * (yn * yn)) + (2 * p2) * xy)
    return _table(fx * xd + cx, fy * yd + cy, Z)


def equidistant_map(K_out, size_out, K_raw, k=(0.0, 0.0, 0.0, 0.0), R=None) -> np.ndarray:
    """Kannala-Brandt (OpenCV fisheye) coordinates as a TABLE map: theta =
    atan(r), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 +
    k4 theta^8), the ray scaled by theta_d / r."""
    xn, yn, Z = _rays(K_out, size_out, R)
    k1, k2, k3, k4 = (float(v) for v in k)
    fx, fy, cx, cy = (float(v) for v in K_raw)
    r = np.sqrt(xn * xn + yn * yn)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(r > 1e-12, thd / r, 1.0)
    return _table(fx * (xn * s) + cx, fy * (yn * s) + cy, Z)
