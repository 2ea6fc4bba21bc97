"""Python host mirror of the reference interface over the C ABI.

``Context`` wraps one ``viso_ctx`` (one HIP device + stream).  The stage
functions (``pyramid``, ``fast``, ``klt``, ...) mirror the reference's
functions for the parity tests; ``Viso`` / ``Keyframe`` / ``FrameSequence``
(viso_amd/frontend.py) mirror the reference's classes.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

_ctx_cache: dict = {}


def _p(a: np.ndarray | None):
    return None if a is None else a.ctypes.data


def pyramid_dims(width: int, height: int):
    dims = np.zeros(8, np.int32)
    total = ctypes.c_size_t(0)
    _lib.call("viso_pyramid_dims", width, height, _p(dims), ctypes.byref(total))
    return [(int(dims[2 * l]), int(dims[2 * l + 1])) for l in range(4)], int(total.value)


def default_params(fx=517.3, fy=516.5, cx=325.1, cy=249.7, width=640, height=480, **kw):
    """Defaults = include/viso.h:20-26 and the intrinsics of src/main.cpp:14-17."""
    p = _lib.viso_params()
    _lib.call("viso_default_params", ctypes.byref(p), fx, fy, cx, cy, width, height)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


class Context:
    """One viso_ctx: device memory + a HIP stream for one sequence."""

    def __init__(self, params=None, device: int = 0, **kw):
        self.params = params if params is not None else default_params(**kw)
        self.device = device
        h = ctypes.c_void_p()
        _lib.call("viso_create", ctypes.byref(self.params), device, ctypes.byref(h))
        self.h = h

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            _lib.load().viso_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------ stages
    def pyramid(self, images: np.ndarray) -> np.ndarray:
        """Keyframe pyramid (include/keyframe.h:28-46) of n images (n,h,w) ->
        (n, total_bytes) levels concatenated."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        if images.ndim == 2:
            images = images[None]
        n, h, w = images.shape
        _, total = pyramid_dims(w, h)
        out = np.zeros((n, total), np.uint8)
        _lib.call("viso_pyramid", self.h, _p(images), n, w, h, _p(out))
        return out

    def fast(self, image: np.ndarray, thresh: int = 50, cap: int = 1 << 20):
        """cv::FAST(img, kps, thresh) + NMS (src/viso.cpp:104): row-major
        (xs, ys, scores)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape
        xs = np.zeros(cap, np.int32)
        ys = np.zeros(cap, np.int32)
        sc = np.zeros(cap, np.int32)
        n = ctypes.c_size_t(0)
        _lib.call("viso_fast", self.h, _p(image), w, h, thresh, _p(xs), _p(ys), _p(sc), cap,
                  ctypes.byref(n))
        m = min(n.value, cap)
        return xs[:m].copy(), ys[:m].copy(), sc[:m].copy()

    def klt(self, ref_pyr: np.ndarray, cur_pyr: np.ndarray, width: int, height: int,
            kp1: np.ndarray, kp2: np.ndarray):
        """OpticalFlowMultiLevel(..., inverse=true) (src/viso.cpp:353-391).
        kp1, kp2: (n,2) float32; returns (kp2_out, success)."""
        kp1 = np.ascontiguousarray(kp1, dtype=np.float32)
        kp2 = np.ascontiguousarray(kp2, dtype=np.float32).copy()
        n = kp1.shape[0]
        succ = np.zeros(n, np.uint8)
        _lib.call("viso_klt", self.h, _p(np.ascontiguousarray(ref_pyr)),
                  _p(np.ascontiguousarray(cur_pyr)), width, height, _p(kp1), _p(kp2), _p(succ), n)
        return kp2, succ

    def direct_pose(self, last_pyr, cur_pyr, width, height, points, pose_last, pose_init):
        """DirectPoseEstimationMultiLayer (src/viso.cpp:760-766); poses 12 doubles."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        pl = np.ascontiguousarray(pose_last, dtype=np.float64).reshape(12)
        pio = np.ascontiguousarray(pose_init, dtype=np.float64).reshape(12).copy()
        _lib.call("viso_direct_pose", self.h, _p(np.ascontiguousarray(last_pyr)),
                  _p(np.ascontiguousarray(cur_pyr)), width, height, _p(pts), pts.shape[0],
                  _p(pl), _p(pio))
        return pio

    def direct_solve(self, sums, n_good, state):
        """viso_direct_solve: the faithful Gauss-Newton solve of one level
        (first iteration) on 28 sums, nGood and T21 (7).  Returns (stats (50,)
        = [nGood, cost, H (36), b (6), update (6)], state_out (7,))."""
        s = np.ascontiguousarray(sums, dtype=np.float64).reshape(28)
        st = np.ascontiguousarray(state, dtype=np.float64).reshape(7)
        stats = np.zeros(50, np.float64)
        out = np.zeros(7, np.float64)
        _lib.call("viso_direct_solve", self.h, _p(s), int(n_good), _p(st), _p(stats), _p(out))
        return stats, out

    def lk_align(self, kf_pyrs, kf_poses, cur_pyr, cur_pose, width, height, points):
        """LKAlignment (src/viso.cpp:768-843): dense per-map-point outputs
        (pair_kf, success, uv_before (n,2), uv_after (n,2))."""
        kfp = np.ascontiguousarray(np.stack(kf_pyrs) if isinstance(kf_pyrs, (list, tuple))
                                   else kf_pyrs, dtype=np.uint8)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        pk = np.zeros(n, np.int32)
        sc = np.zeros(n, np.uint8)
        ub = np.zeros((n, 2), np.float64)
        ua = np.zeros((n, 2), np.float64)
        cp = np.ascontiguousarray(cur_pose, dtype=np.float64).reshape(12)
        _lib.call("viso_lk_align", self.h, _p(kfp), _p(kposes), kposes.shape[0],
                  _p(np.ascontiguousarray(cur_pyr)), _p(cp), width, height, _p(pts), n, _p(pk),
                  _p(sc), _p(ub), _p(ua))
        return pk, sc, ub, ua

    def lk_align_warped(self, kf_pyrs, kf_poses, cur_pyr, cur_pose, width, height, points,
                        max_area_ratio: float = 64.0):
        """viso_lk_align_warped: ``lk_align`` by the warped kernel
        (viso_set_lk_warp).  Returns (pair_kf, success, uv_before, uv_after,
        A (n, 4), shift (n,) int8, status (n,) uint8)."""
        kfp = np.ascontiguousarray(np.stack(kf_pyrs) if isinstance(kf_pyrs, (list, tuple))
                                   else kf_pyrs, dtype=np.uint8)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        pk = np.zeros(n, np.int32)
        sc = np.zeros(n, np.uint8)
        ub = np.zeros((n, 2), np.float64)
        ua = np.zeros((n, 2), np.float64)
        A = np.zeros((n, 4), np.float64)
        sh = np.zeros(n, np.int8)
        st = np.zeros(n, np.uint8)
        cp = np.ascontiguousarray(cur_pose, dtype=np.float64).reshape(12)
        _lib.call("viso_lk_align_warped", self.h, _p(kfp), _p(kposes), kposes.shape[0],
                  _p(np.ascontiguousarray(cur_pyr)), _p(cp), width, height, _p(pts), n, float(max_area_ratio),
                  _p(pk), _p(sc), _p(ub), _p(ua), _p(A), _p(sh), _p(st))
        return pk, sc, ub, ua, A, sh, st

    def lk_align_illum(self, kf_pyrs, kf_poses, cur_pyr, cur_pose, width, height, points,
                       max_area_ratio: float = 64.0, max_gain: float = 4.0, warp_rows: bool = True,
                       gain_rows: bool = True):
        """viso_lk_align_illum: ``lk_align_warped`` by the illumination-
        invariant form (viso_set_lk_illum).  Returns (pair_kf, success,
        uv_before, uv_after, A (n, 4), shift, status, gain_offset (n, 2));
        with ``warp_rows`` / ``gain_rows`` false those outputs are passed as
        NULL and returned as None."""
        kfp = np.ascontiguousarray(np.stack(kf_pyrs) if isinstance(kf_pyrs, (list, tuple))
                                   else kf_pyrs, dtype=np.uint8)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        pk = np.zeros(n, np.int32)
        sc = np.zeros(n, np.uint8)
        ub = np.zeros((n, 2), np.float64)
        ua = np.zeros((n, 2), np.float64)
        A = np.zeros((n, 4), np.float64) if warp_rows else None
        sh = np.zeros(n, np.int8) if warp_rows else None
        st = np.zeros(n, np.uint8) if warp_rows else None
        go = np.zeros((n, 2), np.float64) if gain_rows else None
        cp = np.ascontiguousarray(cur_pose, dtype=np.float64).reshape(12)
        opt = lambda a: None if a is None else _p(a)
        _lib.call("viso_lk_align_illum", self.h, _p(kfp), _p(kposes), kposes.shape[0],
                  _p(np.ascontiguousarray(cur_pyr)), _p(cp), width, height, _p(pts), n, float(max_area_ratio),
                  float(max_gain), _p(pk), _p(sc), _p(ub), _p(ua), opt(A), opt(sh), opt(st), opt(go))
        return pk, sc, ub, ua, A, sh, st, go

    # depth seeds (viso_depth_seeds_*).  Seed rows travel as a
    # dict: h (n,) int32, uv (n, 2), mu (n,), s2 (n,), cnt (n, 4) int32 =
    # (good, bad, lost, status).
    @staticmethod
    def _seed_rows(rows):
        r = {"h": np.ascontiguousarray(rows["h"], dtype=np.int32).reshape(-1).copy(),
             "uv": np.ascontiguousarray(rows["uv"], dtype=np.float64).reshape(-1, 2).copy(),
             "mu": np.ascontiguousarray(rows["mu"], dtype=np.float64).reshape(-1).copy(),
             "s2": np.ascontiguousarray(rows["s2"], dtype=np.float64).reshape(-1).copy(),
             "cnt": np.ascontiguousarray(rows["cnt"], dtype=np.int32).reshape(-1, 4).copy()}
        n = r["h"].shape[0]
        if not all(v.shape[0] == n for v in r.values()):
            raise ValueError("seed rows: one entry per seed in every column")
        return r, n

    def depth_seeds_create(self, image, pose, points, cell: int = 16, host: int = 0, depth_min: float = 2.0,
                           depth_max: float = 60.0, n_live: int = 0, cap: int | None = None):
        """viso_depth_seeds_create: the seeds a new keyframe adds (image its
        level 0, pose 12 doubles Tcw, points (n, 3) the map).  Returns
        (rows, counts [cell winners, seeds appended])."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        pc = np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        cells = -(-w // cell) * -(-h // cell) if cell > 0 else 1
        cap = cells if cap is None else int(cap)
        m = max(cap, 1)
        r = {"h": np.zeros(m, np.int32), "uv": np.zeros((m, 2)), "mu": np.zeros(m), "s2": np.zeros(m),
             "cnt": np.zeros((m, 4), np.int32)}
        n = ctypes.c_size_t(0)
        counts = np.zeros(2, np.int32)
        _lib.call("viso_depth_seeds_create", self.h, _p(image), w, h, _p(pc), _p(pts), pts.shape[0], int(cell),
                  int(host), float(depth_min), float(depth_max), int(n_live), _p(r["h"]), _p(r["uv"]), _p(r["mu"]),
                  _p(r["s2"]), _p(r["cnt"]), cap, ctypes.byref(n), _p(counts))
        k = min(int(n.value), cap)
        return {key: v[:k].copy() for key, v in r.items()}, [int(c) for c in counts]

    def depth_seeds_update(self, rows, kf_pyrs, kf_poses, cur_pyr, cur_pose, width, height, max_steps: int = 32,
                           depth_min: float = 2.0, depth_max: float = 60.0, max_score: float = 57600.0,
                           uniqueness: float = 1.5):
        """viso_depth_seeds_update: one frame's update of the seed rows.
        Returns (rows, level_step (n, 2) int32: search level, best step)."""
        r, n = self._seed_rows(rows)
        kfp = np.ascontiguousarray(np.stack(kf_pyrs) if isinstance(kf_pyrs, (list, tuple)) else kf_pyrs,
                                   dtype=np.uint8)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        cp = np.ascontiguousarray(cur_pose, dtype=np.float64).reshape(12)
        ls = np.full((max(n, 1), 2), -1, np.int32)
        _lib.call("viso_depth_seeds_update", self.h, _p(kfp), _p(kposes), kposes.shape[0],
                  _p(np.ascontiguousarray(cur_pyr, dtype=np.uint8)), _p(cp), width, height, n, int(max_steps),
                  float(depth_min), float(depth_max), float(max_score), float(uniqueness), _p(r["h"]), _p(r["uv"]),
                  _p(r["mu"]), _p(r["s2"]), _p(r["cnt"]), _p(ls))
        return r, ls[:n]

    def depth_seeds_promote(self, rows, kf_poses, room: int, min_good: int = 3, conv_rel: float = 0.05,
                            max_bad: int = 4, max_lost: int = 4):
        """viso_depth_seeds_promote: one promotion.  Returns dict(points
        (promoted, 3) world, host (promoted,), rows (the survivors), counts
        [converged, promoted, dropped, survivors])."""
        r, n = self._seed_rows(rows)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        m = max(min(int(room), n), 1)
        pts = np.zeros((m, 3), np.float64)
        hosts = np.zeros(m, np.int32)
        counts = np.zeros(4, np.int32)
        _lib.call("viso_depth_seeds_promote", self.h, _p(kposes), kposes.shape[0], n, int(min_good), float(conv_rel),
                  int(max_bad), int(max_lost), int(room), _p(r["h"]), _p(r["uv"]), _p(r["mu"]), _p(r["s2"]),
                  _p(r["cnt"]), _p(pts), _p(hosts), _p(counts))
        np_, ns = int(counts[1]), int(counts[3])
        return {"points": pts[:np_].copy(), "host": hosts[:np_].copy(),
                "rows": {key: v[:ns].copy() for key, v in r.items()}, "counts": [int(c) for c in counts]}

    def pose_2d2d(self, p1: np.ndarray, p2: np.ndarray, R0=None, T0=None):
        """PoseEstimation2d2d + SelectMotion (src/viso.cpp:178-256, 520-638) on
        normalised (n,3) points.  Returns dict(R, T, inliers, points3d,
        candidates, stats)."""
        p1 = np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 3)
        p2 = np.ascontiguousarray(p2, dtype=np.float64).reshape(-1, 3)
        n = p1.shape[0]
        R = np.ascontiguousarray(np.eye(3) if R0 is None else R0, dtype=np.float64).reshape(9).copy()
        T = np.ascontiguousarray(np.zeros(3) if T0 is None else T0, dtype=np.float64).reshape(3).copy()
        inl = np.zeros(max(n, 1), np.uint8)
        pts = np.zeros((max(n, 1), 3), np.float64)
        cand = np.zeros((5, 12), np.float64)
        st = np.zeros(8, np.float64)
        _lib.call("viso_pose_2d2d", self.h, _p(p1), _p(p2), n, _p(R), _p(T), _p(inl), _p(pts),
                  _p(cand), _p(st))
        return {"R": R.reshape(3, 3), "T": T, "inliers": inl[:n], "points3d": pts[:n],
                "candidates": cand[:int(st[2])], "stats": st}

    def stereo_match(self, left, right, xs, ys, max_disp: int = 128):
        """North-star stereo SAD stage: (disparity, sad) per left keypoint."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        h, w = left.shape
        xs = np.ascontiguousarray(xs, dtype=np.int32)
        ys = np.ascontiguousarray(ys, dtype=np.int32)
        n = len(xs)
        d = np.zeros(n, np.int32)
        s = np.zeros(n, np.int32)
        _lib.call("viso_stereo_match", self.h, _p(left), _p(right), w, h, _p(xs), _p(ys), n,
                  max_disp, _p(d), _p(s))
        return d, s

    def mono_points(self, cur_pyr, kf_pyr, width: int, height: int, pose_c, pose_k, points, cell: int = 16,
                    min_parallax_deg: float = 0.25, cap: int | None = None):
        """viso_mono_points: the new points of one monocular keyframe
        insertion (viso_set_mono_keyframes) of frame c against keyframe k.
        Pyramids as ``pyramid`` returns them, poses 12 doubles (Tcw), points
        (n, 3) the map.  Returns dict(points (min(kept, cap), 3) world, n kept,
        xy (winners, 2), accept (winners,), counts [corners, winners, KLT
        successes, kept])."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        pc = np.ascontiguousarray(pose_c, dtype=np.float64).reshape(12)
        pk = np.ascontiguousarray(pose_k, dtype=np.float64).reshape(12)
        cells = -(-width // cell) * -(-height // cell) if cell > 0 else 1
        cap = cells if cap is None else int(cap)
        out = np.zeros((max(cap, 1), 3), np.float64)
        xy = np.zeros((max(cells, 1), 2), np.int32)
        acc = np.zeros(max(cells, 1), np.uint8)
        counts = np.zeros(4, np.int32)
        n = ctypes.c_size_t(0)
        _lib.call("viso_mono_points", self.h, _p(np.ascontiguousarray(cur_pyr, dtype=np.uint8)),
                  _p(np.ascontiguousarray(kf_pyr, dtype=np.uint8)), width, height, _p(pc), _p(pk), _p(pts),
                  pts.shape[0], int(cell), float(min_parallax_deg), _p(out), _p(xy), _p(acc), cap,
                  ctypes.byref(n), _p(counts))
        nw = int(counts[1])
        return {"points": out[:min(n.value, cap)].copy(), "n": int(n.value), "xy": xy[:nw].copy(),
                "accept": acc[:nw].copy(), "counts": [int(c) for c in counts]}

    def map_retire(self, width: int, height: int, pose_c, kf_poses, points, host, cell: int = 16):
        """viso_map_retire: one retirement of the sliding-window map
        (viso_set_map_window) on host data: keyframe 0 of kf_poses (k, 12)
        leaves, c is the check frame.  points (n, 3) world, host (n,) keyframe
        indices.  Returns dict(points (kept, 3), host (kept,), keep (n,), n
        kept, counts [retired-host, of those seen by c, candidates,
        survivors])."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        hst = np.ascontiguousarray(host, dtype=np.int32).reshape(-1)
        pc = np.ascontiguousarray(pose_c, dtype=np.float64).reshape(12)
        kp = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        n = pts.shape[0]
        if hst.shape[0] != n:
            raise ValueError("map_retire: one host per point")
        out = np.zeros((max(n, 1), 3), np.float64)
        oh = np.zeros(max(n, 1), np.int32)
        keep = np.zeros(max(n, 1), np.uint8)
        counts = np.zeros(4, np.int32)
        m = ctypes.c_size_t(0)
        _lib.call("viso_map_retire", self.h, width, height, _p(pc), _p(kp), kp.shape[0], _p(pts), _p(hst), n,
                  int(cell), _p(out), _p(oh), _p(keep), ctypes.byref(m), _p(counts))
        return {"points": out[:m.value].copy(), "host": oh[:m.value].copy(), "keep": keep[:n].copy(),
                "n": int(m.value), "counts": [int(c) for c in counts]}

    def refine_pose(self, points, pair_kf, success, uv_before, uv_after, pose_in, iterations: int = 5,
                    huber_px: float = 1.0, max_shift_px: float = 8.0):
        """viso_refine_pose: one pose refinement (viso_set_pose_refine) on
        host data with the context's intrinsics: points (n, 3) world, the LK
        row as ``lk_align`` returns it, pose_in 12 doubles (Tcw).  Returns
        (pose (12,), report (8,))."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        pk = np.ascontiguousarray(pair_kf, dtype=np.int32).reshape(-1)
        sc = np.ascontiguousarray(success, dtype=np.uint8).reshape(-1)
        ub = np.ascontiguousarray(uv_before, dtype=np.float64).reshape(-1, 2)
        ua = np.ascontiguousarray(uv_after, dtype=np.float64).reshape(-1, 2)
        if not (pk.shape[0] == sc.shape[0] == ub.shape[0] == ua.shape[0] == n):
            raise ValueError("refine_pose: one LK entry per point")
        pin = np.ascontiguousarray(pose_in, dtype=np.float64).reshape(12)
        out = np.zeros(12, np.float64)
        rep = np.zeros(8, np.float64)
        _lib.call("viso_refine_pose", self.h, _p(pts), _p(pk), _p(sc), _p(ub), _p(ua), n, _p(pin), int(iterations),
                  float(huber_px), float(max_shift_px), _p(out), _p(rep))
        return out, rep

    def point_tracks_update(self, points, pair_kf, success, uv_after, pose, tracks, reproj_px: float = 2.0):
        """viso_point_tracks_update: one track-record update
        (viso_set_point_cull) on host data with the context's intrinsics:
        points (n, 3) world, the LK row as ``lk_align`` returns it, pose 12
        doubles (Tcw), tracks (n, 4) int32.  Returns (tracks (n, 4), counts
        [paired, good, failed, longest fail_run])."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        pk = np.ascontiguousarray(pair_kf, dtype=np.int32).reshape(-1)
        sc = np.ascontiguousarray(success, dtype=np.uint8).reshape(-1)
        ua = np.ascontiguousarray(uv_after, dtype=np.float64).reshape(-1, 2)
        tr = np.array(tracks, dtype=np.int32, order="C").reshape(-1, 4)  # (a copy: updated in place)
        if not (pk.shape[0] == sc.shape[0] == ua.shape[0] == tr.shape[0] == n):
            raise ValueError("point_tracks_update: one LK entry and one record per point")
        T = np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        counts = np.zeros(4, np.int32)
        _lib.call("viso_point_tracks_update", self.h, _p(pts), _p(pk), _p(sc), _p(ua), n, _p(T), float(reproj_px),
                  _p(tr), _p(counts))
        return tr, [int(c) for c in counts]

    def cull_points(self, points, host, tracks, max_fail_run: int = 3, min_points: int = 50):
        """viso_points_cull: one cull (viso_set_point_cull) on host data:
        points (n, 3), host (n,), tracks (n, 4) int32.  Returns dict(points
        (kept, 3), host (kept,), tracks (kept, 4), keep (n,), n kept, counts
        [candidates, survivors, kept, abandoned])."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        hst = np.ascontiguousarray(host, dtype=np.int32).reshape(-1)
        tr = np.ascontiguousarray(tracks, dtype=np.int32).reshape(-1, 4)
        if not (hst.shape[0] == tr.shape[0] == n):
            raise ValueError("cull_points: one host and one record per point")
        out = np.zeros((max(n, 1), 3), np.float64)
        oh = np.zeros(max(n, 1), np.int32)
        ot = np.zeros((max(n, 1), 4), np.int32)
        keep = np.zeros(max(n, 1), np.uint8)
        counts = np.zeros(4, np.int32)
        m = ctypes.c_size_t(0)
        _lib.call("viso_points_cull", self.h, _p(pts), _p(hst), _p(tr), n, int(max_fail_run), int(min_points),
                  _p(out), _p(oh), _p(ot), _p(keep), ctypes.byref(m), _p(counts))
        return {"points": out[:m.value].copy(), "host": oh[:m.value].copy(), "tracks": ot[:m.value].copy(),
                "keep": keep[:n].copy(), "n": int(m.value), "counts": [int(c) for c in counts]}

    def point_obs_record(self, pair_kf, success, uv_before, uv_after, max_shift_px: float = 8.0):
        """viso_point_obs_record: one frame's record into the observation ring
        (viso_set_point_refine) on host data: the LK row as ``lk_align``
        returns it.  Returns (valid (n,) uint8, uv (n, 2))."""
        pk = np.ascontiguousarray(pair_kf, dtype=np.int32).reshape(-1)
        n = pk.shape[0]
        sc = np.ascontiguousarray(success, dtype=np.uint8).reshape(-1)
        ub = np.ascontiguousarray(uv_before, dtype=np.float64).reshape(-1, 2)
        ua = np.ascontiguousarray(uv_after, dtype=np.float64).reshape(-1, 2)
        if not (sc.shape[0] == ub.shape[0] == ua.shape[0] == n):
            raise ValueError("point_obs_record: one LK entry per point")
        valid = np.zeros(max(n, 1), np.uint8)
        uv = np.zeros((max(n, 1), 2), np.float64)
        _lib.call("viso_point_obs_record", self.h, _p(pk), _p(sc), _p(ub), _p(ua), n, float(max_shift_px),
                  _p(valid), _p(uv))
        return valid[:n].copy(), uv[:n].copy()

    def refine_points(self, points, anchor_kf, kf_poses, frame_poses, obs_valid, obs_uv, iterations: int = 3,
                      huber_px: float = 1.0, min_obs: int = 3, max_rel_sigma: float = 0.05):
        """viso_points_refine: one point refinement (viso_set_point_refine) on
        host data with the context's intrinsics: points (n, 3) world,
        anchor_kf (n,) keyframe indices (< 0: none), kf_poses (k, 12),
        frame_poses (m, 12) the live ring slots, obs_valid (m, n), obs_uv
        (m, n, 2).  Returns dict(points (n, 3), status (n,), steps (n,), costs
        (n, 2), counts [eligible, moved, status 4, status 2])."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = pts.shape[0]
        an = np.ascontiguousarray(anchor_kf, dtype=np.int32).reshape(-1)
        kp = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        fp = np.ascontiguousarray(frame_poses, dtype=np.float64).reshape(-1, 12)
        m = fp.shape[0]
        ov = np.ascontiguousarray(obs_valid, dtype=np.uint8).reshape(m, -1)
        uv = np.ascontiguousarray(obs_uv, dtype=np.float64).reshape(m, -1, 2)
        if not (an.shape[0] == ov.shape[1] == uv.shape[1] == n):
            raise ValueError("refine_points: one anchor and m observations per point")
        out = np.zeros((max(n, 1), 3), np.float64)
        status = np.zeros(max(n, 1), np.uint8)
        steps = np.zeros(max(n, 1), np.uint8)
        costs = np.zeros((max(n, 1), 2), np.float64)
        counts = np.zeros(4, np.int32)
        _lib.call("viso_points_refine", self.h, _p(pts), _p(an), n, _p(kp), kp.shape[0], _p(fp), m, _p(ov), _p(uv),
                  int(iterations), float(huber_px), int(min_obs), float(max_rel_sigma), _p(out), _p(status),
                  _p(steps), _p(costs), _p(counts))
        return {"points": out[:n].copy(), "status": status[:n].copy(), "steps": steps[:n].copy(),
                "costs": costs[:n].copy(), "counts": [int(c) for c in counts]}

    # ------------------------------------------------------------ timing
    def photometric_ba(self, kf_images, kf_poses, points, host, iterations: int = 5):
        """viso_photometric_ba: the BA of include/bundle_adjuster.h:22-106 on
        host data; returns (poses (k, 12), points (n, 3), report
        (iterations, 4): cost, candidate cost, damping, accepted)."""
        imgs = [np.ascontiguousarray(x, np.uint8) for x in kf_images]
        P = ctypes.c_void_p * len(imgs)
        poses = np.ascontiguousarray(kf_poses, np.float64).reshape(-1, 12).copy()
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy()
        hst = np.ascontiguousarray(host, np.int32)
        rep = np.zeros((iterations, 4))
        _lib.call("viso_photometric_ba", self.h, P(*[x.ctypes.data for x in imgs]), len(imgs), _p(poses), _p(pts),
                  _p(hst), len(pts), iterations, _p(rep))
        return poses, pts, rep

    def kf_align(self, kf_pyrs, kf_poses, cur_pyr, width, height, points, extra_seed=None, iterations: int = 10,
                 max_points: int = 512, max_cost: float = 57600.0, min_good_permille: int = 500):
        """viso_kf_align: one relocalisation attempt (viso_set_relocalise;
        DESIGN.md §19) on host data with the context's intrinsics.  Candidate
        (1 + n_extra) k + s aligns keyframe k to the current frame from its own
        pose (s = 0) or from extra_seed (s = 1).  Returns dict(poses (n_cand,
        12), report (n_cand, 20), winner)."""
        kfp = np.ascontiguousarray(np.stack(kf_pyrs) if isinstance(kf_pyrs, (list, tuple)) else kf_pyrs,
                                   dtype=np.uint8)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        seed = None if extra_seed is None else np.ascontiguousarray(extra_seed, dtype=np.float64).reshape(12)
        n_kf = kposes.shape[0]
        n_cand = n_kf * (1 if seed is None else 2)
        poses = np.zeros((n_cand, 12), np.float64)
        report = np.zeros((n_cand, 20), np.float64)
        winner = ctypes.c_int32(-1)
        _lib.call("viso_kf_align", self.h, _p(kfp), _p(kposes), n_kf, _p(np.ascontiguousarray(cur_pyr, dtype=np.uint8)),
                  width, height, _p(pts), pts.shape[0], _p(seed), 0 if seed is None else 1, int(iterations),
                  int(max_points), float(max_cost), int(min_good_permille), _p(poses), _p(report),
                  ctypes.byref(winner))
        return {"poses": poses, "report": report, "winner": int(winner.value)}

    def kf_align_illum(self, kf_pyrs, kf_poses, cur_pyr, width, height, points, extra_seed=None, iterations: int = 10,
                       max_points: int = 512, max_cost: float = 57600.0, min_good_permille: int = 500,
                       max_gain: float = 4.0):
        """viso_kf_align_illum: ``kf_align`` with an affine brightness map
        (g, o) estimated per candidate (viso_set_reloc_illum);
        status 5 rejects a gain outside [1 / max_gain, max_gain].  Returns
        dict(poses (n_cand, 12), report (n_cand, 20), gain_offset (n_cand, 2),
        winner)."""
        kfp = np.ascontiguousarray(np.stack(kf_pyrs) if isinstance(kf_pyrs, (list, tuple)) else kf_pyrs,
                                   dtype=np.uint8)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        seed = None if extra_seed is None else np.ascontiguousarray(extra_seed, dtype=np.float64).reshape(12)
        n_kf = kposes.shape[0]
        n_cand = n_kf * (1 if seed is None else 2)
        poses = np.zeros((n_cand, 12), np.float64)
        report = np.zeros((n_cand, 20), np.float64)
        gain_offset = np.zeros((n_cand, 2), np.float64)
        winner = ctypes.c_int32(-1)
        _lib.call("viso_kf_align_illum", self.h, _p(kfp), _p(kposes), n_kf,
                  _p(np.ascontiguousarray(cur_pyr, dtype=np.uint8)), width, height, _p(pts), pts.shape[0], _p(seed),
                  0 if seed is None else 1, int(iterations), int(max_points), float(max_cost), int(min_good_permille),
                  float(max_gain), _p(poses), _p(report), _p(gain_offset), ctypes.byref(winner))
        return {"poses": poses, "report": report, "gain_offset": gain_offset, "winner": int(winner.value)}

    def set_reloc_illum(self, mode: int, max_gain: float = 4.0) -> None:
        """viso_set_reloc_illum: while the relocalisation is
        on, every attempt of a lost frame estimates (T, g, o); 0 = off."""
        _lib.call("viso_set_reloc_illum", self.h, int(mode), float(max_gain))

    def get_reloc_illum(self) -> np.ndarray:
        """viso_get_reloc_illum: int64[8] = mode, attempts run in this form,
        recoveries through it, the last such attempt's winner (-1), 0, 0, 0, 0."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_reloc_illum", self.h, _p(info))
        return info

    def reloc_illum_rows(self) -> np.ndarray:
        """viso_get_reloc_illum_rows: the (g, o) rows (n_cand, 2) of the last
        attempt run in this form."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_reloc_illum_rows", self.h, None, 0, ctypes.byref(n))
        rows = np.zeros((max(int(n.value), 1), 2))
        if n.value:
            _lib.call("viso_get_reloc_illum_rows", self.h, _p(rows), n.value, ctypes.byref(n))
        return rows[:n.value]

    def track_affine(self, last_pyr, cur_pyr, width, height, points, pose_last, seed, iterations: int = 10):
        """viso_track_affine: the brightness-compensated tracking stage
        (viso_set_brightness) on host data with the context's
        intrinsics: the pose of the current frame together with the affine
        brightness map (g, o) from the last frame to it.  Returns (pose (12,),
        report (24,))."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        L = np.ascontiguousarray(pose_last, dtype=np.float64).reshape(12)
        S = np.ascontiguousarray(seed, dtype=np.float64).reshape(12)
        pose, report = np.zeros(12), np.zeros(24)
        _lib.call("viso_track_affine", self.h, _p(np.ascontiguousarray(last_pyr, dtype=np.uint8)),
                  _p(np.ascontiguousarray(cur_pyr, dtype=np.uint8)), width, height, _p(pts), pts.shape[0], _p(L), _p(S),
                  int(iterations), _p(pose), _p(report))
        return pose, report

    def set_brightness(self, iterations: int = 10) -> None:
        """viso_set_brightness; iterations 0 = off."""
        _lib.call("viso_set_brightness", self.h, int(iterations))

    def get_brightness(self) -> np.ndarray:
        """viso_get_brightness: int64[8] = iterations, frames tracked with the
        mode on, passes applied in all, frames whose level 0 ended with exit 4,
        then of the last frame: its level-0 exit, its steps, its level-0 n, 0."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_brightness", self.h, _p(info))
        return info

    def brightness_log(self) -> np.ndarray:
        """viso_get_brightness_log: (poses, 4) = g, o, level-0 exit, steps over
        all levels; NaN rows for frames tracked with the mode off."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_brightness_log", self.h, None, 0, ctypes.byref(n))
        rows = np.zeros((max(int(n.value), 1), 4))
        if n.value:
            _lib.call("viso_get_brightness_log", self.h, _p(rows), n.value, ctypes.byref(n))
        return rows[:n.value]

    def brightness_report(self) -> np.ndarray:
        """viso_get_brightness_report: the last frame's report (24,)."""
        report = np.zeros(24)
        _lib.call("viso_get_brightness_report", self.h, _p(report))
        return report

    def track_robust(self, last_pyr, cur_pyr, width, height, points, pose_last, seed, iterations: int = 10,
                     huber_k: float = 9.0, weights: bool = True):
        """viso_track_robust: track_affine's stage with a Huber weight per
        patch pixel (viso_set_robust); huber_k in grey levels.
        Returns (pose (12,), report (28,), weights (n,): the weight mass per
        point of the last pass evaluated on level 0, or None with
        weights=False)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        L = np.ascontiguousarray(pose_last, dtype=np.float64).reshape(12)
        S = np.ascontiguousarray(seed, dtype=np.float64).reshape(12)
        pose, report = np.zeros(12), np.zeros(28)
        w = np.zeros(max(pts.shape[0], 1)) if weights else None
        _lib.call("viso_track_robust", self.h, _p(np.ascontiguousarray(last_pyr, dtype=np.uint8)),
                  _p(np.ascontiguousarray(cur_pyr, dtype=np.uint8)), width, height, _p(pts), pts.shape[0], _p(L), _p(S),
                  int(iterations), float(huber_k), _p(pose), _p(report), _p(w))
        return pose, report, None if w is None else w[:pts.shape[0]]

    def set_robust(self, huber_k: float = 9.0) -> None:
        """viso_set_robust: Huber weights in every frame the
        brightness chain tracks; huber_k 0 = off."""
        _lib.call("viso_set_robust", self.h, float(huber_k))

    def get_robust(self) -> np.ndarray:
        """viso_get_robust: int64[8] = on, frames tracked robustly, then of the
        last such frame: its down-weighted pixels, its level-0 n, 0..."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_robust", self.h, _p(info))
        return info

    def robust_report(self) -> np.ndarray:
        """viso_get_robust_report: the last robust frame's report (28,)."""
        report = np.zeros(28)
        _lib.call("viso_get_robust_report", self.h, _p(report))
        return report

    def robust_weights(self) -> np.ndarray:
        """viso_get_robust_weights: the last robust frame's weight mass per map
        point, in the map's order when that frame was tracked."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_robust_weights", self.h, None, 0, ctypes.byref(n))
        w = np.zeros(max(int(n.value), 1))
        if n.value:
            _lib.call("viso_get_robust_weights", self.h, _p(w), n.value, ctypes.byref(n))
        return w[:n.value]

    def robust_log(self) -> np.ndarray:
        """viso_get_robust_log: (poses, 2) = mean weight (report 24 / (64 x
        level-0 n)), down-weighted pixels; NaN rows for frames not tracked
        robustly."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_robust_log", self.h, None, 0, ctypes.byref(n))
        rows = np.zeros((max(int(n.value), 1), 2))
        if n.value:
            _lib.call("viso_get_robust_log", self.h, _p(rows), n.value, ctypes.byref(n))
        return rows[:n.value]

    def set_reloc_seed(self, hypotheses: int = 256, max_hamming: int = 48, ratio_permille: int = 800,
                       inlier_px: float = 2.0, min_inliers: int = 30, seed: int = 0) -> None:
        """viso_set_reloc_seed; hypotheses 0 = off."""
        _lib.call("viso_set_reloc_seed", self.h, int(hypotheses), int(max_hamming), int(ratio_permille),
                  float(inlier_px), int(min_inliers), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def get_reloc_seed(self) -> np.ndarray:
        """viso_get_reloc_seed: int64[8] = on, seed stages run, stages with
        status 0, recoveries through a seed, then of the last stage: M, its
        best score, its k*, its status."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_reloc_seed", self.h, _p(info))
        return info

    def reloc_seed_report(self):
        """viso_get_reloc_seed_report: (report (12,), pose (12,))."""
        report, pose = np.zeros(12), np.zeros(12)
        _lib.call("viso_get_reloc_seed_report", self.h, _p(report), _p(pose))
        return report, pose

    def reloc_seed(self, kf_pyrs, kf_poses, cur_pyr, width, height, points, hosts, start, hypotheses: int = 256,
                   max_hamming: int = 48, ratio_permille: int = 800, inlier_px: float = 2.0, min_inliers: int = 30,
                   seed: int = 0):
        """viso_reloc_seed: one seed stage on host data with the
        context's intrinsics, FAST threshold and corner cap.  Returns
        dict(report (12,), pose (12,), matches (M, 3) = point, kept corner,
        distance, inliers (M,))."""
        kfp = np.ascontiguousarray(np.stack(kf_pyrs) if isinstance(kf_pyrs, (list, tuple)) else kf_pyrs,
                                   dtype=np.uint8)
        kposes = np.ascontiguousarray(kf_poses, dtype=np.float64).reshape(-1, 12)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        hst = np.ascontiguousarray(hosts, dtype=np.int32).reshape(-1)
        if hst.shape[0] != pts.shape[0]:
            raise ValueError("hosts must have one entry per point")
        S = np.ascontiguousarray(start, dtype=np.float64).reshape(12)
        cap = max(pts.shape[0], 1)
        report, pose = np.zeros(12), np.zeros(12)
        matches, inliers = np.zeros((cap, 3), np.int32), np.zeros(cap, np.uint8)
        n = ctypes.c_size_t(0)
        _lib.call("viso_reloc_seed", self.h, _p(kfp), _p(kposes), kposes.shape[0],
                  _p(np.ascontiguousarray(cur_pyr, dtype=np.uint8)), width, height, _p(pts), _p(hst), pts.shape[0],
                  _p(S), int(hypotheses), int(max_hamming), int(ratio_permille), float(inlier_px), int(min_inliers),
                  int(seed) & 0xFFFFFFFFFFFFFFFF, _p(report), _p(pose), _p(matches), _p(inliers), cap, ctypes.byref(n))
        m = min(int(n.value), cap)
        return {"report": report, "pose": pose, "matches": matches[:m].copy(), "inliers": inliers[:m].copy()}

    def rectify(self, raw, K_out, size_out, counts: bool = True, **kw):
        """viso_rectify: n raw images (n, rh, rw) or (rh, rw) -> rectified
        (n, h, w) with the output intrinsics K_out = (fx, fy, cx, cy) and
        size_out = (w, h), by the frame path's launch.  kw: the arguments of
        viso_amd.rectify.params (model, fill, K_raw, dist, R, map; raw_size is
        taken from the images).  Returns (out, (outside, clipped)) or, with
        counts=False, out."""
        from . import rectify as _rect
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        if raw.ndim == 2:
            raw = raw[None]
        n, rh, rw = raw.shape
        w, h = int(size_out[0]), int(size_out[1])
        p, keep = _rect.params(raw_size=(rw, rh), **kw)
        if keep is not None and keep.shape[:2] != (h, w):
            raise ValueError("map must be (h, w, 2) of the output size")
        Ko = np.ascontiguousarray(K_out, dtype=np.float64).reshape(4)
        out = np.zeros((n, h, w), np.uint8)
        cnt = np.zeros(2, np.int64)
        _lib.call("viso_rectify", self.h, ctypes.byref(p), _p(Ko), w, h, _p(raw), n, _p(out),
                  _p(cnt) if counts else None)
        return (out, (int(cnt[0]), int(cnt[1]))) if counts else out

    def timing_enable(self, on: bool = True):
        _lib.call("viso_timing_enable", self.h, 1 if on else 0)

    def timing_select(self, kernels=None):
        """Time only the named kernels (None: all)."""
        mask = 0xFFFFFFFF if kernels is None else sum(1 << _lib.kernel_id(k) for k in kernels)
        _lib.call("viso_timing_select", self.h, mask)

    def timing(self, kernel: str):
        launches = ctypes.c_int64(0)
        ms = ctypes.c_double(0.0)
        _lib.call("viso_timing_get", self.h, _lib.kernel_id(kernel), ctypes.byref(launches),
                  ctypes.byref(ms))
        return int(launches.value), float(ms.value)

    def synchronize(self):
        _lib.call("viso_synchronize", self.h)


def mono_points(cur_pyr, kf_pyr, width, height, pose_c, pose_k, points, cell=16, min_parallax_deg=0.25,
                cap=None, K=None, device: int = 0):
    """``Context.mono_points`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).mono_points(cur_pyr, kf_pyr, width, height, pose_c, pose_k,
                                                                points, cell, min_parallax_deg, cap)


def map_retire(width, height, pose_c, kf_poses, points, host, cell=16, K=None, device: int = 0):
    """``Context.map_retire`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).map_retire(width, height, pose_c, kf_poses, points, host, cell)


def refine_pose(points, pair_kf, success, uv_before, uv_after, pose_in, iterations=5, huber_px=1.0,
                max_shift_px=8.0, width=640, height=480, K=None, device: int = 0):
    """``Context.refine_pose`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).refine_pose(points, pair_kf, success, uv_before, uv_after,
                                                                pose_in, iterations, huber_px, max_shift_px)


def kf_align(kf_pyrs, kf_poses, cur_pyr, width, height, points, extra_seed=None, iterations=10, max_points=512,
             max_cost=57600.0, min_good_permille=500, K=None, device: int = 0):
    """``Context.kf_align`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).kf_align(kf_pyrs, kf_poses, cur_pyr, width, height, points,
                                                              extra_seed, iterations, max_points, max_cost,
                                                              min_good_permille)


def kf_align_illum(kf_pyrs, kf_poses, cur_pyr, width, height, points, extra_seed=None, iterations=10, max_points=512,
                   max_cost=57600.0, min_good_permille=500, max_gain=4.0, K=None, device: int = 0):
    """``Context.kf_align_illum`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).kf_align_illum(kf_pyrs, kf_poses, cur_pyr, width, height, points,
                                                                    extra_seed, iterations, max_points, max_cost,
                                                                    min_good_permille, max_gain)


def track_affine(last_pyr, cur_pyr, width, height, points, pose_last, seed, iterations=10, K=None, device: int = 0):
    """``Context.track_affine`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).track_affine(last_pyr, cur_pyr, width, height, points, pose_last,
                                                                  seed, iterations)


def track_robust(last_pyr, cur_pyr, width, height, points, pose_last, seed, iterations=10, huber_k=9.0, K=None,
                 device: int = 0):
    """``Context.track_robust`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).track_robust(last_pyr, cur_pyr, width, height, points, pose_last,
                                                                  seed, iterations, huber_k)


def point_tracks_update(points, pair_kf, success, uv_after, pose, tracks, reproj_px=2.0, width=640, height=480,
                        K=None, device: int = 0):
    """``Context.point_tracks_update`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).point_tracks_update(points, pair_kf, success, uv_after, pose,
                                                                        tracks, reproj_px)


def cull_points(points, host, tracks, max_fail_run=3, min_points=50, width=640, height=480, K=None,
                device: int = 0):
    """``Context.cull_points`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).cull_points(points, host, tracks, max_fail_run, min_points)


def point_obs_record(pair_kf, success, uv_before, uv_after, max_shift_px=8.0, width=640, height=480, K=None,
                     device: int = 0):
    """``Context.point_obs_record`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).point_obs_record(pair_kf, success, uv_before, uv_after,
                                                                     max_shift_px)


def refine_points(points, anchor_kf, kf_poses, frame_poses, obs_valid, obs_uv, iterations=3, huber_px=1.0,
                  min_obs=3, max_rel_sigma=0.05, width=640, height=480, K=None, device: int = 0):
    """``Context.refine_points`` on the cached context of intrinsics K."""
    return default_context(width, height, device, K).refine_points(points, anchor_kf, kf_poses, frame_poses,
                                                                  obs_valid, obs_uv, iterations, huber_px, min_obs,
                                                                  max_rel_sigma)


def default_context(width: int = 640, height: int = 480, device: int = 0, K=None) -> Context:
    """A cached context per (device, intrinsics).  The stage functions that
    project points (direct_pose, lk_align, pose_2d2d) use the context's K,
    as the reference's Viso members do (include/viso.h:28-29)."""
    K = tuple(K) if K is not None else (517.3, 516.5, 325.1, 249.7)
    key = (device, K)
    c = _ctx_cache.get(key)
    if c is None or c.h is None:  # absent or closed by a caller
        c = Context(default_params(fx=K[0], fy=K[1], cx=K[2], cy=K[3], width=width,
                                   height=height), device=device)
        _ctx_cache[key] = c
    return c
