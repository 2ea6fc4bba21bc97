"""Rectification (viso_set_rectify / viso_get_rectify / viso_rectify,
include/viso/viso_c.h): raw camera frames are undistorted and
rectified on the device ahead of the pyramid.  The repo's own spec, restated
in tests/rectify_ref.py (no reference counterpart: src/main.cpp:14-17
hard-codes ideal pinhole intrinsics).

CPU: known answers of the restatement; its geometry against an independent
lens formula; its usefulness on the CPU oracle; the exports.
GPU: every byte and count of the stage entry and every getter of the frame
path equal the restatement's (array_equal, no tolerance)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import images, oracle_lib, rectify_ref as rr, seqdata

IDENT = rr.IDENT
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return tuple((Rz @ Ry @ Rx).ravel())


# ------------------------------------------------------------------ CPU 1: known answers
# power-of-two focal lengths: (x - cx) / fx * fx + cx is exact
KE = (64.0, 32.0, 20.0, 12.0)


@pytest.mark.parametrize("w,h", [(64, 48), (640, 480), (1242, 375)])
def test_ref_identity_is_the_input(w, h):
    K = (0.8 * w, 0.8 * w, w / 2 - 0.5, h / 2 - 0.5)
    raw = images.noise(h, w, seed=w)
    u, v, front = rr.radtan_coords(K, (w, h), K, ZERO)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    assert front.all() and np.abs(u - x).max() <= 6e-14 and np.abs(v - y).max() <= 6e-14
    out, counts = rr.rectify(raw, K, (w, h), Kr=K, dist=ZERO, fill=99)
    assert np.array_equal(out, raw) and counts == (0, 0)


def test_ref_principal_point_shift():
    w, h = 40, 24
    raw = images.noise(h, w, seed=1)
    out, counts = rr.rectify(raw, KE, (w, h), Kr=(KE[0], KE[1], KE[2] + 3, KE[3]), dist=ZERO, fill=77)
    assert np.array_equal(out[:, :w - 3], raw[:, 3:])
    assert (out[:, w - 3:] == 77).all()  # u = x + 3 >= rw: outside
    assert counts == (3 * h, 3 * h)


def _table(w, h, u, v):
    t = np.zeros((h, w, 2), np.float32)
    t[..., 0] = u
    t[..., 1] = v
    return t


def test_ref_half_pixel_table_and_ties():
    w, h = 16, 8
    raw = images.noise(h, w + 1, seed=2).astype(np.int64)
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    out, counts = rr.rectify(raw.astype(np.uint8), None, (w, h), model=rr.TABLE, table=_table(w, h, x + 0.5, y))
    assert np.array_equal(out, (raw[:, :-1] + raw[:, 1:] + 1) >> 1) and counts == (0, 0)
    # ties of 32 u + 0.5 go up: u = x + 1/64 is weight 1 of 32, not 0;
    # u = x + 1/64 - 1/2048 stays at weight 0
    row = np.array([[0, 64, 0, 64]], np.uint8)
    up, _ = rr.rectify(row, None, (3, 1), model=rr.TABLE, table=_table(3, 1, np.arange(3) + 1 / 64, 0.0))
    assert up.tolist() == [[(0 * 31 * 32 + 64 * 1 * 32 + 512) >> 10, (64 * 31 * 32 + 512) >> 10, 2]]
    dn, _ = rr.rectify(row, None, (3, 1), model=rr.TABLE, table=_table(3, 1, np.arange(3) + 1 / 64 - 1 / 2048, 0.0))
    assert dn.tolist() == [[0, 64, 0]]


def test_ref_boundary_coordinates_and_fill():
    rw, rh, fill = 9, 5, 200
    raw = np.full((rh, rw), 40, np.uint8)
    us = [-1.0, -1 + 1 / 64, -1 + 3 / 64, -0.5, 0.0, rw - 1.0, rw - 1 + 1 / 64, rw - 0.5, rw - 1 / 64, float(rw),
          np.nan, np.inf, -np.inf]
    w = len(us)
    out, counts = rr.rectify(raw, None, (w, 1), model=rr.TABLE, fill=fill, table=_table(w, 1, us, 2.0))
    mix = lambda a_fill: (fill * a_fill * 32 + 40 * (32 - a_fill) * 32 + 512) >> 10  # noqa: E731
    assert out[0].tolist() == [
        fill,       # u = -1 is not > -1: outside
        mix(31),    # qu = -31: x0 = -1 (fill, weight 31), x0 + 1 = 0 (weight 1)
        mix(30),    # -1 + 3/64: qu = -30
        mix(16),
        40,         # u = 0: one tap
        40,         # u = rw - 1: tap rw has weight 0
        mix(1),     # the tap at rw is fill
        mix(16),
        fill,       # qu = 32 rw: x0 = rw, ax = 0: fill alone, yet inside
        fill,       # u = rw: outside
        fill, fill, fill]
    # outside: -1, rw, NaN, +Inf, -Inf; clipped: those and every fill-weighted tap
    assert counts == (5, 5 + 6)
    # the same along v, and the fill value of an outside pixel is `fill`
    outv, cv = rr.rectify(raw, None, (1, 4), model=rr.TABLE, fill=3,
                          table=_table(1, 4, 1.0, np.array([[-1.0], [-1 + 1 / 64], [rh - 1.0], [float(rh)]])))
    assert outv[:, 0].tolist() == [3, (3 * 31 * 32 + 40 * 32 + 512) >> 10, 40, 3] and cv == (2, 3)


def test_ref_behind_the_camera_is_outside():
    w, h = 32, 16
    K = (8.0, 8.0, 16.0, 8.0)  # a wide view: a in [-2, 2)
    R = _rot(0.0, np.radians(60), 0.0)
    u, v, front = rr.radtan_coords(K, (w, h), K, ZERO, R)
    assert 0 < (~front).sum() < w * h
    out, counts = rr.rectify(np.full((h, w), 9, np.uint8), K, (w, h), Kr=K, dist=ZERO, R=R, fill=123)
    assert (out[~front] == 123).all() and counts[0] >= (~front).sum()


# ------------------------------------------------------------------ CPU 2: geometry
def _texture(X, Y):
    return 127.5 + 60 * np.cos(2 * np.pi * X / 40) * np.cos(2 * np.pi * Y / 56) + 40 * np.sin(2 * np.pi * (X + Y) / 97)


def test_ref_geometry_against_the_forward_lens_formula():
    """An analytic texture on the pinhole image plane, rendered (a) directly
    and (b) through the lens — every raw pixel's ideal ray by the iterative
    inverse of the textbook forward formula — and then rectified.

    Bound 3 grey levels, from: the rounding of the raw bytes, of the output
    and of the direct render (0.5 each); the bilinear error (Hxx + Hyy) / 8 =
    (1.65 + 0.92) / 8 = 0.32 in pinhole pixels, times the lens's squared
    magnification (< 1.4); the 1/64-pixel coordinate quantisation times the
    gradient sum (12.0 + 9.3) / 64 = 0.33, times the magnification (< 1.2):
    2.35 in all.  Measured: max 1, mean 0.19."""
    W, H, RW, RH = 320, 240, 352, 264
    K, Kr = (260.0, 255.0, 158.3, 121.7), (270.0, 268.0, 177.2, 130.4)
    dist = (-0.15, 0.02, 0.0008, -0.0005, 0.001)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    direct = np.rint(_texture(x, y)).astype(np.int64)
    u, v = np.meshgrid(np.arange(RW, dtype=np.float64), np.arange(RH, dtype=np.float64))
    xd, yd = (u - Kr[2]) / Kr[0], (v - Kr[3]) / Kr[1]
    xn, yn = rr.undistort(xd, yd, dist)
    bx, by = rr.distort(xn, yn, dist)
    assert max(np.abs(bx - xd).max(), np.abs(by - yd).max()) < 1e-14  # the inverse has converged
    raw = np.clip(np.rint(_texture(K[0] * xn + K[2], K[1] * yn + K[3])), 0, 255).astype(np.uint8)
    out, counts = rr.rectify(raw, K, (W, H), Kr=Kr, dist=dist)
    assert counts == (0, 0)
    err = np.abs(out.astype(np.int64) - direct)
    print("rectified vs direct render: max", err.max(), "mean", err.mean())
    assert err.max() <= 3


# ------------------------------------------------------------------ CPU 3: usefulness
UW, UH, UN = 620, 188, 12
UDIST = (-0.15, 0.01125, 0.0008, -0.0005, 0.0)


def _T(p12):
    M = np.eye(4)
    M[:3, :3] = np.asarray(p12[:9]).reshape(3, 3)
    M[:3, 3] = p12[9:]
    return M


def _oracle_translation_error(seq, frames):
    v = oracle_lib.Viso(seq.K, UW, UH, enable_tracking=1)
    v.set_stereo(seq.p.baseline, 128, 1)
    for left, right in frames:
        v.on_new_stereo(left, right)
    P = v.poses()
    assert len(P) == UN - 1
    T0inv = np.linalg.inv(_T(seq.pose(0)))
    err = []
    for k, p in enumerate(P):  # camera centres, metres (tests/test_keyframes.py)
        G, E = _T(seq.pose(k + 1)) @ T0inv, _T(p)
        err.append(np.linalg.norm(-G[:3, :3].T @ G[:3, 3] + E[:3, :3].T @ E[:3, 3]))
    return float(np.mean(err))


def test_oracle_tracks_rectified_frames_better_than_raw_ones():
    """The CPU oracle (stereo initialisation, 11 tracked poses at 620 x 188)
    on the renderer's pinhole frames, on those frames seen through a lens (k1
    = -0.15, barrel: 10 px at the corners), and on the lens frames after
    rectify_ref.  Mean camera-centre error against the renderer's truth,
    measured: pinhole 0.0200 m, raw 0.2221 m, rectified 0.0165 m — the raw run
    is 13 times worse than the rectified one.  Asserted: rectified < raw, with
    a gap of at least 5 times."""
    seq = seqdata.sequence(0, UW, UH)
    K = seq.K
    pin = [seq.frame(f) for f in range(UN)]
    raw = [tuple(rr.warp_to_raw(im, K, K, (UW, UH), UDIST) for im in fr) for fr in pin]
    rect = [tuple(rr.rectify(np.stack(fr), K, (UW, UH), Kr=K, dist=UDIST)[0]) for fr in raw]
    e_pin, e_raw, e_rect = (_oracle_translation_error(seq, fr) for fr in (pin, raw, rect))
    print(f"translation error: pinhole {e_pin:.4f} raw {e_raw:.4f} rectified {e_rect:.4f}")
    assert e_rect < e_raw
    assert 5 * e_rect < e_raw
    assert e_rect < 2 * e_pin  # rectification gives the pinhole run back


# ------------------------------------------------------------------ CPU 4: exports
def test_exports_and_prototypes():
    from viso_amd import _lib
    lib = _lib.load()
    for name in ("viso_set_rectify", "viso_get_rectify", "viso_rectify"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.KERNEL_IDS["rectify"] == 16
    assert ctypes.sizeof(_lib.viso_rectify_params) == 4 * 4 + 9 * 8 + 9 * 8 + 8 + 4 * 4


def test_map_helpers_match_the_analytic_model():
    from viso_amd import rectify as vr
    w, h = 96, 64
    K, Kr = (70.0, 72.0, 47.0, 31.0), (75.0, 74.0, 50.0, 33.0)
    dist = (-0.2, 0.05, 0.001, -0.002, 0.01)
    R = _rot(0.01, -0.02, 0.005)
    u, v, front = rr.radtan_coords(K, (w, h), Kr, dist, R)
    m = vr.radtan_map(K, (w, h), Kr, dist, R)
    assert m.dtype == np.float32 and m.shape == (h, w, 2) and front.all()
    assert np.array_equal(m[..., 0], u.astype(np.float32)) and np.array_equal(m[..., 1], v.astype(np.float32))
    # the equidistant model: theta_d = theta (k = 0) is r_d = atan(r); a point on
    # the axis stays, and the map is the pinhole one to first order
    e = vr.equidistant_map(K, (w, h), Kr, (0.0, 0.0, 0.0, 0.0))
    xn, yn = (np.arange(w) - K[2]) / K[0], (31 - K[3]) / K[1]
    assert np.allclose(e[31, :, 0], Kr[0] * np.arctan(np.abs(xn)) * np.sign(xn) + Kr[2], atol=1e-4)
    assert np.allclose(e[31, 47], [Kr[2], Kr[3]], atol=1e-5) and yn == 0
    # behind the raw camera: NaN (outside)
    back = vr.radtan_map((8.0, 8.0, 16.0, 8.0), (32, 16), Kr, ZERO, _rot(0.0, np.radians(60), 0.0))
    assert np.isnan(back).any() and not np.isnan(back).all()


def test_kitti_sequence_passes_parameters_on():
    from viso_amd import kitti

    class Recorder:
        def __init__(self):
            self.calls = []

        def set_rectify(self, cam, **kw):
            self.calls.append((cam, kw))

    ks = kitti.KittiSequence.__new__(kitti.KittiSequence)  # (no directory needed for this)
    ks.width, ks.height = 1392, 512
    ks.rectify = (dict(K_raw=(980.0, 975.0, 690.0, 250.0), dist=(-0.37, 0.2, 0.001, -0.001, -0.07)), None)
    rec = Recorder()
    ks.configure(rec)
    assert rec.calls == [(0, dict(raw_size=(1392, 512), K_raw=(980.0, 975.0, 690.0, 250.0),
                                 dist=(-0.37, 0.2, 0.001, -0.001, -0.07)))]


def test_cpp_facade_compiles_and_links(tmp_path):
    out = subprocess.run([_build_cpp(tmp_path)], capture_output=True, text=True, check=True)
    assert "rectify facade ok" in out.stdout


def _build_cpp(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "rectify_check")
    libdir = os.path.join(root, "viso_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "rectify_check.cpp"), "-L", libdir, "-lviso_amd",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    return exe


# ------------------------------------------------------------------ GPU 5: the stage entry
@functools.lru_cache(maxsize=1)
def _ctx():
    import viso_amd
    return viso_amd.default_context(64, 48)


def _stage_cases(w, h):
    """(name, raw size, kwargs of rectify_ref.rectify beyond K and size,
    expects outside pixels: yes / no / None = either).  K: the output
    intrinsics of every case."""
    K = (0.9 * w, 0.8 * w, w / 2 - 0.3, h / 2 + 0.2)
    rw, rh = w + 5, h + 3  # raw sizes differ from the output's
    Kr = (K[0] * 1.05, K[1] * 1.1, rw / 2 + 0.4, rh / 2 - 0.1)
    cases = [
        ("identity", (w, h), dict(Kr=K, dist=ZERO, fill=9), False),
        ("int shift", (rw, rh), dict(Kr=(K[0], K[1], K[2] + 3, K[3] - 2), dist=ZERO, fill=0), True),
        ("frac shift", (rw, rh), dict(Kr=(K[0], K[1], K[2] + 0.3, K[3] + 0.71), dist=ZERO, fill=200), False),
        ("rotation", (rw, rh), dict(Kr=Kr, dist=(0.01, 0.0, 0.001, -0.001, 0.0), R=_rot(0.03, -0.05, 0.1), fill=0),
         None),
    ]
    Kw = (w / 4, w / 4, K[2], K[3])  # a wide output view (a in about [-2, 2)) for "behind" and the strong lenses
    # R = Ry(60 deg): Z = 0.5 - 0.866 a <= 0 for a >= 0.577, part of the wide view
    cases.append(("behind", (rw, rh), dict(K=Kw, Kr=(w / 4, w / 4, rw / 2, rh / 2), dist=ZERO,
                                           R=_rot(0.0, np.radians(60), 0.0), fill=200), True))
    for fill in (0, 200):
        cases.append((f"barrel {fill}", (rw, rh), dict(K=Kw, Kr=Kr, dist=(-0.9, 0.3, 0.002, 0.001, -0.05), fill=fill),
                      True))
        cases.append((f"pincushion {fill}", (rw, rh), dict(K=Kw, Kr=Kr, dist=(0.6, 0.4, -0.003, 0.002, 0.1),
                                                           fill=fill), True))
    return K, cases


def _special_table(w, h, rw, rh):
    """A smooth table with NaN, +-Inf and the boundary coordinates poked in."""
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    t = _table(w, h, x * (rw / w) + 0.37 + 0.01 * y, y * (rh / h) - 0.21 + 0.02 * x)
    su = [np.nan, np.inf, -np.inf, -1.0, -1 + 1 / 64, -1 + 1 / 32, rw - 1.0, rw - 1 + 1 / 64, rw - 1 / 64, float(rw),
          -0.5, 0.0]
    sv = [np.nan, np.inf, -np.inf, -1.0, -1 + 1 / 64, -1 + 1 / 32, rh - 1.0, rh - 1 + 1 / 64, rh - 1 / 64, float(rh),
          -0.5, 0.0]
    flat = t.reshape(-1, 2)
    k = 0
    for a in su:  # u special, v ordinary, and the reverse, spread over the image
        flat[(7 * k + 1) % len(flat), 0] = a
        k += 1
    for a in sv:
        flat[(7 * k + 1) % len(flat), 1] = a
        k += 1
    for a, b in zip(su, sv):  # both special
        flat[(7 * k + 1) % len(flat)] = (a, b)
        k += 1
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("w", [8, 61, 64, 65, 255, 256, 257])
def test_gpu_stage_entry_matches_ref(w):
    ctx = _ctx()
    for h in (8, 9, 17):
        K, cases = _stage_cases(w, h)
        for name, (rw, rh), kw, some_outside in cases:
            raw = images.noise(rh, rw, seed=w + h)
            Ko = kw.pop("K", K)
            exp, ecnt = rr.rectify(raw, Ko, (w, h), **kw)
            got, gcnt = ctx.rectify(raw, Ko, (w, h), model=rr.RADTAN, fill=kw["fill"], K_raw=kw["Kr"], dist=kw["dist"],
                                    R=kw.get("R"))
            assert np.array_equal(got[0], exp), (name, w, h)
            assert gcnt == ecnt, (name, w, h, gcnt, ecnt)
            assert some_outside is None or (ecnt[0] > 0) == some_outside, (name, w, h, ecnt)
            if name == "identity":
                assert ecnt == (0, 0) and np.array_equal(exp, raw)
            if name == "behind":  # part of the image, not all of it, is at Z <= 0
                front = rr.radtan_coords(Ko, (w, h), kw["Kr"], kw["dist"], kw["R"])[2]
                assert 0 < (~front).sum() < w * h, (w, h)
            # the same coordinates through a table (rounded to float32; Z <= 0 is NaN there)
            if name in ("rotation", "pincushion 200", "behind"):
                from viso_amd import rectify as vr
                tab = vr.radtan_map(Ko, (w, h), kw["Kr"], kw["dist"], kw.get("R"))
                exp_t, ecnt_t = rr.rectify(raw, None, (w, h), model=rr.TABLE, table=tab, fill=kw["fill"])
                got_t, gcnt_t = ctx.rectify(raw, Ko, (w, h), model=rr.TABLE, fill=kw["fill"], map=tab)
                assert np.array_equal(got_t[0], exp_t) and gcnt_t == ecnt_t, (name, w, h)
        rw, rh = w + 5, h + 3
        raw = images.noise(rh, rw, seed=3 * w + h)
        for fill in (0, 200):
            tab = _special_table(w, h, rw, rh)
            exp, ecnt = rr.rectify(raw, None, (w, h), model=rr.TABLE, table=tab, fill=fill)
            got, gcnt = ctx.rectify(raw, K, (w, h), model=rr.TABLE, fill=fill, map=tab)
            assert np.array_equal(got[0], exp) and gcnt == ecnt, ("table", w, h, fill)
            assert ecnt[0] >= 5 and ecnt[1] > ecnt[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 128, 129])  # 128: the kernel's batch (kRectBatch)
def test_gpu_stage_entry_batches(n):
    w, h, rw, rh = 61, 9, 70, 13
    K, cases = _stage_cases(w, h)
    name, _, kw, _ = cases[4]  # part of every image at Z <= 0
    assert name == "behind"
    Ko = kw.pop("K")
    raw = np.stack([images.noise(rh, rw, seed=100 + i) for i in range(n)])
    exp, ecnt = rr.rectify(raw, Ko, (w, h), **kw)
    got, gcnt = _ctx().rectify(raw, Ko, (w, h), fill=kw["fill"], K_raw=kw["Kr"], dist=kw["dist"], R=kw["R"])
    assert np.array_equal(got, exp) and gcnt == ecnt
    assert 0 < (~rr.radtan_coords(Ko, (w, h), kw["Kr"], kw["dist"], kw["R"])[2]).sum() < w * h
    tab = _special_table(w, h, rw, rh)
    exp, ecnt = rr.rectify(raw, None, (w, h), model=rr.TABLE, table=tab, fill=5)
    got, gcnt = _ctx().rectify(raw, K, (w, h), model=rr.TABLE, fill=5, map=tab)
    assert np.array_equal(got, exp) and gcnt == ecnt


# the frame path's cameras: the renderer's frames, treated as raw
W, H = seqdata.W, seqdata.H
# (mild lenses: the frames are not what such a camera would have seen, and the
# monocular initialisation still has to accept their geometry)
CAM0 = dict(Kr_scale=(1.004, 1.006), c_off=(1.3, -0.6), dist=(-0.01, 0.002, 0.0003, -0.0002, 0.0),
            R=_rot(0.0005, -0.0008, 0.001), fill=0)
CAM1 = dict(Kr_scale=(0.997, 1.006), c_off=(-0.7, -0.6), dist=(-0.008, 0.001, -0.0002, 0.0003, 0.0005),
            R=_rot(0.0005, 0.0004, 0.001), fill=16)


def _cam(K, cam, raw_size, out_size):
    """(rectify_ref kwargs, viso_amd.rectify.params kwargs) of a frame-path camera."""
    sx, sy = raw_size[0] / out_size[0], raw_size[1] / out_size[1]
    Kr = (K[0] * sx * cam["Kr_scale"][0], K[1] * sy * cam["Kr_scale"][1], K[2] * sx + cam["c_off"][0],
          K[3] * sy + cam["c_off"][1])
    ref = dict(Kr=Kr, dist=cam["dist"], R=cam["R"], fill=cam["fill"])
    dev = dict(model=rr.RADTAN, raw_size=raw_size, K_raw=Kr, dist=cam["dist"], R=cam["R"], fill=cam["fill"])
    return ref, dev


@pytest.mark.gpu
def test_gpu_stage_entry_full_frame():
    seq = seqdata.sequence(0)
    raw = np.stack([seqdata.image(0), seqdata.image(0, cam=1)])
    ref, dev = _cam(seq.K, CAM0, (W, H), (W, H))
    exp, ecnt = rr.rectify(raw, seq.K, (W, H), **ref)
    dev.pop("raw_size")
    got, gcnt = _ctx().rectify(raw, seq.K, (W, H), **dev)
    assert np.array_equal(got, exp) and gcnt == ecnt
    from viso_amd import rectify as vr
    tab = vr.radtan_map(seq.K, (W, H), ref["Kr"], ref["dist"], ref["R"])
    exp, ecnt = rr.rectify(raw, None, (W, H), model=rr.TABLE, table=tab, fill=3)
    got, gcnt = _ctx().rectify(raw, seq.K, (W, H), model=rr.TABLE, fill=3, map=tab)
    assert np.array_equal(got, exp) and gcnt == ecnt


@pytest.mark.gpu
def test_gpu_stage_entry_runs_through_the_timed_launch():
    ctx = _ctx()
    ctx.timing_enable(True)
    try:
        before = ctx.timing("rectify")[0]
        ctx.rectify(images.noise(20, 30, seed=0), (30.0, 30.0, 15.0, 10.0), (30, 20), K_raw=(30.0, 30.0, 15.0, 10.0))
        assert ctx.timing("rectify")[0] == before + 1
    finally:
        ctx.timing_enable(False)


# ------------------------------------------------------------------ GPU 6-8: the frame path
def _getters(v):
    v.synchronize()
    k1, k2, s = v.tracks()
    pk, sc, ub, ua = v.alignment()
    return {"state": np.array([v.state]), "poses": v.poses, "points": v.GetPoints(), "kp1": k1, "kp2": k2,
            "success": s, "lk_pair": pk, "lk_success": sc, "uv_before": ub, "uv_after": ua, "frame_log": v.frame_log(),
            "stats": v.stats()}


def _same(a, b):
    for key in a:
        assert a[key].shape == b[key].shape, key
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def _viso(seq, size=(W, H), stereo=False, **kw):
    import viso_amd
    # the output camera: the renderer's intrinsics scaled to the output size
    K = tuple(seq.K) if size == (W, H) else (seq.K[0] * size[0] / W, seq.K[1] * size[1] / H, seq.K[2] * size[0] / W,
                                             seq.K[3] * size[1] / H)
    v = viso_amd.Viso(*K, width=size[0], height=size[1], enable_tracking=1, **kw)
    if stereo:
        v.set_stereo(seq.p.baseline, 128, 1)
    v.set_frame_log(True)
    return v, K


def _run(v, lefts, rights, path):
    if path == "host":
        for im in lefts:
            v.OnNewFrame(im)
    elif path == "stereo":
        for l, r in zip(lefts, rights):
            v.process(l, r)
    else:
        import torch
        dl = torch.from_numpy(np.stack(lefts)).cuda()
        dr = torch.from_numpy(np.stack(rights)).cuda()
        torch.cuda.synchronize()
        v.process_device(dl.data_ptr(), dr.data_ptr(), len(lefts), lefts[0].size)
        v.synchronize()
    return _getters(v)


@pytest.mark.gpu
@pytest.mark.parametrize("path,size,n", [("host", (W, H), 16), ("stereo", (W, H), 8), ("device", (W, H), 12),
                                         ("host", (1200, 360), 12), ("device", (1200, 360), 8)])
def test_gpu_frame_path_equals_prerectified_frames(path, size, n):
    """A context with the mode on, fed raw frames, gives the bits of a context
    with the mode off fed rectify_ref's output."""
    seq = seqdata.sequence(0)
    stereo = path != "host"
    raw_l = [seqdata.image(f) for f in range(n)]
    raw_r = [seqdata.image(f, cam=1) for f in range(n)]
    on, K = _viso(seq, size, stereo)
    off, _ = _viso(seq, size, stereo)
    ref0, dev0 = _cam(K, CAM0, (W, H), size)
    ref1, dev1 = _cam(K, CAM1, (W, H), size)
    on.set_rectify(0, **dev0)
    exp_l, cnt0 = rr.rectify(np.stack(raw_l), K, size, **ref0)
    if stereo:
        on.set_rectify(1, **dev1)
        exp_r, cnt1 = rr.rectify(np.stack(raw_r), K, size, **ref1)
    else:
        exp_r = exp_l
    on.ctx.timing_enable(True)
    a = _run(on, raw_l, raw_r, path)
    b = _run(off, list(exp_l), list(exp_r), path)
    assert a["state"][0] == 1 and len(a["poses"]) >= 3  # through initialisation into tracking
    _same(a, b)
    info = on.rectify_info(0)
    assert info[:6].tolist() == [rr.RADTAN, W, H, ref0["fill"], cnt0[0], cnt0[1]] and info[7] == n
    launches = on.ctx.timing("rectify")[0]
    if path == "device":
        assert info[6] == 1 and launches == 1  # one batched launch for the chunk, both cameras
    else:
        assert info[6] == n and launches == (2 * n if stereo else n)
    if stereo:
        i1 = on.rectify_info(1)
        assert i1[:6].tolist() == [rr.RADTAN, W, H, ref1["fill"], cnt1[0], cnt1[1]] and i1[7] == n
    assert off.rectify_info(0)[0] == 0


@pytest.mark.gpu
def test_gpu_right_camera_off_passes_through_and_table_camera():
    """Camera 0 through a table, camera 1 off: the right image is used as given."""
    from viso_amd import rectify as vr
    seq = seqdata.sequence(0)
    n = 6
    raw_l = [seqdata.image(f) for f in range(n)]
    right = [seqdata.image(f, cam=1) for f in range(n)]
    on, K = _viso(seq, (W, H), True)
    off, _ = _viso(seq, (W, H), True)
    ref0, _ = _cam(K, CAM0, (W, H), (W, H))
    tab = vr.radtan_map(K, (W, H), ref0["Kr"], ref0["dist"], ref0["R"])
    on.set_rectify(0, model=rr.TABLE, raw_size=(W, H), fill=4, map=tab)
    exp_l, cnt = rr.rectify(np.stack(raw_l), None, (W, H), model=rr.TABLE, table=tab, fill=4)
    _same(_run(on, raw_l, right, "device"), _run(off, list(exp_l), right, "device"))
    assert on.rectify_info(0)[[0, 4, 5, 6, 7]].tolist() == [rr.TABLE, cnt[0], cnt[1], 1, n]
    assert on.rectify_info(1)[0] == 0


@pytest.mark.gpu
def test_gpu_identity_rectification_and_off():
    """Identity parameters give the bits of the mode off; off, no rectify
    launch is counted over a tracked run and the getter reports model 0."""
    seq = seqdata.sequence(0)
    n = 14
    frames = [seqdata.image(f) for f in range(n)]
    ident, K = _viso(seq)
    off, _ = _viso(seq)
    ident.set_rectify(0, model=rr.RADTAN, raw_size=(W, H), K_raw=K, fill=0)
    assert ident.rectify_info(0)[4:6].tolist() == [0, 0]
    off.ctx.timing_enable(True)
    a, b = _run(ident, frames, frames, "host"), _run(off, frames, frames, "host")
    assert b["state"][0] == 1 and len(b["poses"]) >= 3
    _same(a, b)
    assert off.ctx.timing("rectify") == (0, 0.0)
    assert off.rectify_info(0).tolist() == [0] * 8 and off.rectify_info(1).tolist() == [0] * 8
    # switching off again before the first frame: the plain path
    again, _ = _viso(seq)
    again.set_rectify(0, model=rr.RADTAN, raw_size=(W + 8, H), K_raw=K, fill=0)
    again.set_rectify(0)
    _same(_run(again, frames[:6], frames[:6], "host"), _run(_viso(seq)[0], frames[:6], frames[:6], "host"))


# ------------------------------------------------------------------ GPU 9: arguments
@pytest.mark.gpu
def test_gpu_arguments():
    import viso_amd
    from viso_amd import _lib, rectify as vr
    lib = _lib.load()
    v = viso_amd.Viso(300.0, 300.0, 160.0, 48.0, width=320, height=96, enable_tracking=1)
    h = v.ctx.h
    good = dict(model=rr.RADTAN, raw_size=(320, 96), fill=0, K_raw=(300.0, 300.0, 160.0, 48.0))

    def rc(cam=0, **bad):
        p, keep = vr.params(**{**good, **bad})
        return lib.viso_set_rectify(h, cam, ctypes.byref(p))

    assert rc() == 0 and rc(cam=1) == 0
    assert rc(cam=-1) == -1 and rc(cam=2) == -1
    assert rc(model=3) == -1 and rc(model=-1) == -1
    for size in ((15, 96), (320, 15), (4097, 96), (320, 4097), (0, 96), (320, -1)):
        assert rc(raw_size=size) == -1, size
    assert rc(raw_size=(16, 16)) == 0 and rc(raw_size=(4096, 4096)) == 0
    assert rc(fill=-1) == -1 and rc(fill=256) == -1 and rc(fill=255) == 0
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(4):
            K = list(good["K_raw"])
            K[i] = bad
            assert rc(K_raw=K) == -1
        for i in range(5):
            d = [0.0] * 5
            d[i] = bad
            assert rc(dist=d) == -1
        for i in range(9):
            R = list(IDENT)
            R[i] = bad
            assert rc(R=R) == -1
    assert rc(K_raw=(0.0, 300.0, 160.0, 48.0)) == -1 and rc(K_raw=(300.0, -1.0, 160.0, 48.0)) == -1
    assert rc(model=rr.TABLE) == -1  # a null map
    assert rc(model=rr.TABLE, map=np.zeros((96, 320, 2), np.float32)) == 0
    assert lib.viso_set_rectify(None, 0, None) == -1
    info = np.zeros(8, np.int64)
    assert lib.viso_get_rectify(h, 2, info.ctypes.data) == -1 and lib.viso_get_rectify(h, 0, None) == -1
    # NULL and model 0 switch the camera off
    assert lib.viso_set_rectify(h, 0, None) == 0 and v.rectify_info(0)[0] == 0
    assert rc() == 0 and rc(model=0) == 0 and v.rectify_info(0)[0] == 0
    assert lib.viso_set_rectify(h, 1, None) == 0
    # the stage entry
    p, _ = vr.params(**good)
    Ko = np.array(good["K_raw"])
    raw, out = np.zeros((96, 320), np.uint8), np.zeros((96, 320), np.uint8)
    args = [h, ctypes.byref(p), Ko.ctypes.data, 320, 96, raw.ctypes.data, 1, out.ctypes.data, None]
    assert lib.viso_rectify(*args) == 0
    for i, bad in ((0, None), (1, None), (2, None), (3, 0), (3, 4097), (4, 0), (5, None), (6, 0), (7, None)):
        a = list(args)
        a[i] = bad
        assert lib.viso_rectify(*a) == -1, i
    Kbad = np.array([300.0, np.nan, 160.0, 48.0])
    assert lib.viso_rectify(h, ctypes.byref(p), Kbad.ctypes.data, 320, 96, raw.ctypes.data, 1, out.ctypes.data,
                            None) == -1
    pbad, _ = vr.params(**{**good, "fill": 300})
    assert lib.viso_rectify(h, ctypes.byref(pbad), Ko.ctypes.data, 320, 96, raw.ctypes.data, 1, out.ctypes.data,
                            None) == -1
    # a frame of the wrong size for the camera, then VISO_ERR_STATE after the first frame
    assert rc(raw_size=(330, 100)) == 0
    img = images.mixed(96, 320, seed=1)
    assert lib.viso_process_frame(h, img.ctypes.data, 320, 96, 320) == -1
    assert rc() == 0
    assert lib.viso_process_frame(h, img.ctypes.data, 320, 96, 320) == 0
    assert rc() == -4 and lib.viso_set_rectify(h, 0, None) == -4 and rc(cam=1) == -4
    assert v.rectify_info(0)[[0, 6, 7]].tolist() == [rr.RADTAN, 1, 1]


# ------------------------------------------------------------------ GPU 10: the C++ facade
@pytest.mark.gpu
def test_gpu_cpp_facade_runs(tmp_path):
    out = subprocess.run([_build_cpp(tmp_path), "run"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "rectify facade ok" in out.stdout, out.stdout + out.stderr
