"""Host mirror of the reference's classes over the C ABI.

* ``Viso(fx, fy, cx, cy, ...)`` — include/viso.h:11-125: ``OnNewFrame``,
  ``poses``, ``GetPoints()``; plus the north-star ``process(left, right)``.
* ``Keyframe(image)`` — include/keyframe.h:28-46 (pyramid built on device by
  ``OnNewFrame``; ``Pyramids()`` computes it on demand for inspection).
* ``FrameSequence(location, handler)`` — include/frame_sequence.h:11-43:
  ``RunOnce()`` loads ``<location><next_id+1>.png`` and calls
  ``handler.OnNewFrame``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from .api import Context, default_params


class Keyframe:
    """A grey frame handed to ``FrameHandler.OnNewFrame``."""

    next_id_ = 0  # Keyframe::next_id_ (src/keyframe.cpp:7)

    def __init__(self, mat: np.ndarray):
        mat = np.ascontiguousarray(mat, dtype=np.uint8)
        if mat.ndim != 2:
            raise ValueError("Keyframe expects a single-channel (grey) image")
        self.mat_ = mat
        self.id_ = Keyframe.next_id_
        Keyframe.next_id_ += 1

    @classmethod
    def GetNextId(cls) -> int:
        return cls.next_id_

    def GetId(self) -> int:
        return self.id_

    def Mat(self) -> np.ndarray:
        return self.mat_


class FrameHandler:
    """FrameSequence::FrameHandler (include/frame_sequence.h:13-16)."""

    def OnNewFrame(self, keyframe: Keyframe) -> None:  # pragma: no cover - interface
        raise NotImplementedError


class Viso(FrameHandler):
    """Viso (include/viso.h:11): one device context per sequence."""

    def __init__(self, fx: float, fy: float, cx: float, cy: float, width: int = 640,
                 height: int = 480, device: int = 0, **params):
        self.params = default_params(fx=fx, fy=fy, cx=cx, cy=cy, width=width, height=height,
                                     **params)
        self.ctx = Context(self.params, device=device)
        self.width, self.height = width, height

    # ----------------------------------------------------------- reference API
    def OnNewFrame(self, cur_frame) -> None:
        img = cur_frame.Mat() if isinstance(cur_frame, Keyframe) else cur_frame
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape
        _lib.call("viso_process_frame", self.ctx.h, img.ctypes.data, w, h, w)

    @property
    def poses(self) -> np.ndarray:
        """Viso::poses (include/viso.h:54): (n, 3, 4) Tcw."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_poses", self.ctx.h, None, 0, ctypes.byref(n))
        out = np.zeros((n.value, 12), np.float64)
        if n.value:
            _lib.call("viso_get_poses", self.ctx.h, out.ctypes.data, n.value, ctypes.byref(n))
        return out

    def GetPoints(self) -> np.ndarray:
        """Viso::GetPoints (include/viso.h:60-67): (n, 3)."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_points", self.ctx.h, None, 0, ctypes.byref(n))
        out = np.zeros((n.value, 3), np.float64)
        if n.value:
            _lib.call("viso_get_points", self.ctx.h, out.ctypes.data, n.value, ctypes.byref(n))
        return out

    # ----------------------------------------------------------- north-star API
    def process(self, left: np.ndarray, right: np.ndarray) -> None:
        """A stereo pair through the reference path (viso_process_stereo): the
        left image drives OnNewFrame, the right one the stereo initialisation
        (the north-star VisualOdometryStereo is viso_amd.svo)."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        h, w = left.shape
        dims = (ctypes.c_int32 * 3)(w, h, w)
        _lib.call("viso_process_stereo", self.ctx.h, left.ctypes.data, right.ctypes.data, dims)

    def set_stereo(self, baseline: float, max_disp: int = 128, min_disp: int = 1) -> None:
        """Stereo initialisation (viso_set_stereo): with baseline > 0 the first
        frame given with its right image creates a metric map at once."""
        _lib.call("viso_set_stereo", self.ctx.h, float(baseline), int(max_disp), int(min_disp))

    def set_keyframes(self, interval: int, ngood_permille: int = 500) -> None:
        """Stereo keyframe insertion (viso_set_keyframes): every `interval`-th
        tracking frame whose level-0 nGood is below ngood_permille / 1000 of
        the map adds its stereo points and becomes a keyframe."""
        _lib.call("viso_set_keyframes", self.ctx.h, int(interval), int(ngood_permille))

    def set_bundle_adjust(self, iterations: int) -> None:
        """Photometric BA (viso_set_bundle_adjust) after every keyframe
        insertion: `iterations` Levenberg-Marquardt steps over the keyframe
        poses and map points (0 = off)."""
        _lib.call("viso_set_bundle_adjust", self.ctx.h, int(iterations))

    def set_mono_keyframes(self, interval: int, ngood_permille: int = 500, cell: int = 16,
                           min_parallax_deg: float = 0.25) -> None:
        """Monocular keyframe insertion (viso_set_mono_keyframes): the schedule
        and gate of set_keyframes without a right image; the frame's best FAST
        corner of every `cell`-pixel cell no map point projects into is tracked
        into the latest keyframe, triangulated for the known motion and kept
        when it reprojects within projection_error_thresh with at least
        `min_parallax_deg` of parallax.  interval 0 = off."""
        _lib.call("viso_set_mono_keyframes", self.ctx.h, int(interval), int(ngood_permille), int(cell),
                  float(min_parallax_deg))

    def set_map_window(self, window: int, cell: int = 16) -> None:
        """Sliding-window map (viso_set_map_window): the map holds at most
        `window` keyframes (2..8); an insertion into a full window first
        retires the oldest keyframe and culls the points it hosts, keeping
        one per `cell`-pixel cell of the frame that no other point projects
        into and that a remaining keyframe still sees.  window 0 = off."""
        _lib.call("viso_set_map_window", self.ctx.h, int(window), int(cell))

    def map_window(self) -> np.ndarray:
        """viso_get_map_window: int64[8] = window, cell, keyframes retired,
        points culled, then of the last retirement: frames processed before
        its check frame (-1: none yet), retired-host points, survivors, the
        map size after it."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_map_window", self.ctx.h, info.ctypes.data)
        return info

    def point_hosts(self) -> np.ndarray:
        """Every map point's host keyframe index (viso_get_point_hosts)."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_point_hosts", self.ctx.h, None, 0, ctypes.byref(n))
        out = np.zeros(n.value, np.int32)
        if n.value:
            _lib.call("viso_get_point_hosts", self.ctx.h, out.ctypes.data, n.value, ctypes.byref(n))
        return out

    def set_pose_refine(self, iterations: int, huber_px: float = 1.0, max_shift_px: float = 8.0) -> None:
        """Pose refinement (viso_set_pose_refine): every tracking frame's
        direct pose is refined on its LK-aligned features, `iterations`
        Huber-weighted Gauss-Newton steps at most on the reprojection error of
        the successful alignments that moved at most `max_shift_px`.
        iterations 0 = off."""
        _lib.call("viso_set_pose_refine", self.ctx.h, int(iterations), float(huber_px), float(max_shift_px))

    def pose_refine(self) -> np.ndarray:
        """viso_get_pose_refine: float64[8] = observations, steps applied,
        cost at the direct pose, cost at the result, inliers at the result,
        status (0 all passes run, 1 fewer than 6 observations, 2 non-finite
        step, 3 the cost stopped falling), rms at the direct pose, rms at the
        result; NaN before the first refinement."""
        rep = np.zeros(8, np.float64)
        _lib.call("viso_get_pose_refine", self.ctx.h, rep.ctypes.data)
        return rep

    def set_point_cull(self, interval: int, max_fail_run: int = 3, reproj_px: float = 2.0,
                       min_points: int = 50) -> None:
        """Map point culling (viso_set_point_cull): every map point keeps a
        track record {age, seen, found, fail_run} of its LK alignments; every
        `interval`-th tracking frame the points whose alignment failed (or
        landed more than `reproj_px` from their projection) `max_fail_run`
        frames in a row leave the map, unless fewer than `min_points` would
        stay.  interval 0 = off."""
        _lib.call("viso_set_point_cull", self.ctx.h, int(interval), int(max_fail_run), float(reproj_px),
                  int(min_points))

    def point_cull(self) -> np.ndarray:
        """viso_get_point_cull: int64[8] = interval, max_fail_run, culls
        applied, points culled in all, culls abandoned, then of the last
        applied cull: frames processed before its frame (-1: none yet), the
        points it removed, the map size after it."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_point_cull", self.ctx.h, info.ctypes.data)
        return info

    def point_tracks(self) -> np.ndarray:
        """Every map point's track record (viso_get_point_tracks): int32
        (points, 4) = age, seen, found, fail_run."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_point_tracks", self.ctx.h, None, 0, ctypes.byref(n))
        out = np.zeros((n.value, 4), np.int32)
        if n.value:
            _lib.call("viso_get_point_tracks", self.ctx.h, out.ctypes.data, n.value, ctypes.byref(n))
        return out

    def set_point_refine(self, interval: int, window: int = 5, iterations: int = 3, huber_px: float = 1.0,
                         max_shift_px: float = 8.0, min_obs: int = 3, max_rel_sigma: float = 0.05) -> None:
        """Point refinement (viso_set_point_refine): every tracking frame's
        final pose and LK-aligned positions go into a ring of `window` frames;
        every `interval`-th tracking frame each map point's depth along its
        anchor keyframe's ray is refined on them, `iterations` Huber-weighted
        Gauss-Newton steps at most, when at least `min_obs` frames observe it
        and a pixel of error moves the depth by at most `max_rel_sigma`,
        relative.  interval 0 = off."""
        _lib.call("viso_set_point_refine", self.ctx.h, int(interval), int(window), int(iterations), float(huber_px),
                  float(max_shift_px), int(min_obs), float(max_rel_sigma))

    def point_refine(self) -> np.ndarray:
        """viso_get_point_refine: int64[8] = interval, window, refinements
        run, points moved in all, then of the last refinement: frames
        processed before its frame (-1: none yet), its eligible points, the
        points it moved, its status-4 points."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_point_refine", self.ctx.h, info.ctypes.data)
        return info

    def point_refine_status(self):
        """The last refinement's (status, steps) per point, uint8 each
        (viso_get_point_refine_status); empty before the first refinement."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_point_refine_status", self.ctx.h, None, None, 0, ctypes.byref(n))
        status, steps = np.zeros(n.value, np.uint8), np.zeros(n.value, np.uint8)
        if n.value:
            _lib.call("viso_get_point_refine_status", self.ctx.h, status.ctypes.data, steps.ctypes.data, n.value,
                      ctypes.byref(n))
        return status, steps

    def set_depth_seeds(self, interval: int, cell: int = 16, max_steps: int = 32, depth_min: float = 2.0,
                        depth_max: float = 60.0, max_score: float = 57600.0, uniqueness: float = 1.5,
                        min_good: int = 3, conv_rel: float = 0.15, max_bad: int = 4, max_lost: int = 4) -> None:
        """Depth seeds (viso_set_depth_seeds): every corner of a new keyframe
        that the map does not cover becomes a seed with the inverse depth range
        [1 / depth_max, 1 / depth_min]; every tracking frame searches each
        seed's epipolar segment (at most max_steps one-pixel steps) and narrows
        the range; every `interval`-th tracking frame the converged seeds
        become map points and the failed ones are dropped.  0 = off."""
        _lib.call("viso_set_depth_seeds", self.ctx.h, int(interval), int(cell), int(max_steps), float(depth_min),
                  float(depth_max), float(max_score), float(uniqueness), int(min_good), float(conv_rel), int(max_bad),
                  int(max_lost))

    def depth_seeds(self) -> np.ndarray:
        """viso_get_depth_seeds: int64[8] = interval, live seeds, created,
        promoted and dropped in all, then of the live seeds by their last
        update: status 0, status 7-9, status 1-6."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_depth_seeds", self.ctx.h, info.ctypes.data)
        return info

    def depth_seed_rows(self) -> dict:
        """The live seeds' rows (viso_get_depth_seed_rows): h (n,) int32, uv
        (n, 2), mu (n,), s2 (n,), cnt (n, 4) int32 = good, bad, lost, status."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_depth_seed_rows", self.ctx.h, None, None, None, None, None, 0, ctypes.byref(n))
        m = max(int(n.value), 1)
        r = {"h": np.zeros(m, np.int32), "uv": np.zeros((m, 2)), "mu": np.zeros(m), "s2": np.zeros(m),
             "cnt": np.zeros((m, 4), np.int32)}
        if n.value:
            _lib.call("viso_get_depth_seed_rows", self.ctx.h, r["h"].ctypes.data, r["uv"].ctypes.data,
                      r["mu"].ctypes.data, r["s2"].ctypes.data, r["cnt"].ctypes.data, n.value, ctypes.byref(n))
        return {k: v[:n.value] for k, v in r.items()}

    def set_relocalise(self, lost_after: int, max_cost: float = 57600.0, min_good_permille: int = 500,
                       lk_permille: int = 0, iterations: int = 10, max_points: int = 512) -> None:
        """Relocalisation (viso_set_relocalise): a tracking frame is bad when
        its level-0 cost exceeds max_cost, its nGood falls below
        min_good_permille of the map or (lk_permille > 0) its LK successes
        below lk_permille of its pairs; `lost_after` consecutive bad frames
        lose the context, and every lost frame then aligns the keyframes to
        itself (from their own poses and from the last good pose) instead of
        tracking, until one alignment is accepted.  0 = off."""
        _lib.call("viso_set_relocalise", self.ctx.h, int(lost_after), float(max_cost), int(min_good_permille),
                  int(lk_permille), int(iterations), int(max_points))

    def relocalise(self) -> np.ndarray:
        """viso_get_relocalise: int64[8] = lost_after, lost now, losses,
        attempts and recoveries in all, then of the last attempt: frames
        processed before its frame (-1: none), its winner (-1: none), its
        candidates."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_relocalise", self.ctx.h, info.ctypes.data)
        return info

    def relocalise_report(self):
        """The last attempt's candidate rows (viso_get_relocalise_report):
        (poses (n, 12), report (n, 20))."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_relocalise_report", self.ctx.h, None, None, 0, ctypes.byref(n))
        m = max(int(n.value), 1)
        poses, report = np.zeros((m, 12)), np.zeros((m, 20))
        if n.value:
            _lib.call("viso_get_relocalise_report", self.ctx.h, poses.ctypes.data, report.ctypes.data, n.value,
                      ctypes.byref(n))
        return poses[:n.value], report[:n.value]

    def set_reloc_seed(self, hypotheses: int = 256, max_hamming: int = 48, ratio_permille: int = 800,
                       inlier_px: float = 2.0, min_inliers: int = 30, seed: int = 0) -> None:
        """Relocalisation seed (viso_set_reloc_seed; takes effect while
        set_relocalise is on): a lost frame whose attempt has no winner gets a
        pose seed from descriptor matches between the map and its FAST corners,
        and a second attempt from it.  hypotheses 0 = off."""
        self.ctx.set_reloc_seed(hypotheses, max_hamming, ratio_permille, inlier_px, min_inliers, seed)

    def reloc_seed(self) -> np.ndarray:
        """viso_get_reloc_seed: int64[8] = on, seed stages run, stages with
        status 0, recoveries through a seed, then of the last stage: M, its
        best score, its k*, its status."""
        return self.ctx.get_reloc_seed()

    def reloc_seed_report(self):
        """The last seed stage's (report (12,), pose (12,))."""
        return self.ctx.reloc_seed_report()

    def set_reloc_illum(self, mode: int, max_gain: float = 4.0) -> None:
        """Affine brightness per candidate in the relocalisation attempts
        (viso_set_reloc_illum; takes effect while set_relocalise is on): every
        attempt of a lost frame estimates (pose, gain, offset) and rejects a
        gain outside [1 / max_gain, max_gain].  0 = off."""
        self.ctx.set_reloc_illum(mode, max_gain)

    def reloc_illum(self) -> np.ndarray:
        """viso_get_reloc_illum: int64[8] = mode, attempts run in this form,
        recoveries through it, the last such attempt's winner (-1), 0, 0, 0, 0."""
        return self.ctx.get_reloc_illum()

    def reloc_illum_rows(self) -> np.ndarray:
        """The last such attempt's (gain, offset) rows (n_cand, 2)."""
        return self.ctx.reloc_illum_rows()

    def set_brightness(self, iterations: int = 10) -> None:
        """Brightness-compensated tracking (viso_set_brightness): every
        tracking frame's pose is estimated together with an affine brightness
        map (g, o) from the last frame to it, iterated on every pyramid level,
        in place of the direct pose; for cameras whose exposure changes.
        iterations 0 = off."""
        self.ctx.set_brightness(iterations)

    def brightness(self) -> np.ndarray:
        """viso_get_brightness: int64[8] = iterations, frames tracked with the
        mode on, passes applied in all, frames whose level 0 ended with exit 4,
        then of the last frame: its level-0 exit, its steps, its level-0 n, 0."""
        return self.ctx.get_brightness()

    def brightness_log(self) -> np.ndarray:
        """One row per pose: g, o, level-0 exit, steps over all levels (NaN for
        frames tracked with the mode off and for lost frames)."""
        return self.ctx.brightness_log()

    def brightness_report(self) -> np.ndarray:
        """The last frame's report (24,), as Context.track_affine returns it."""
        return self.ctx.brightness_report()

    def set_robust(self, huber_k: float = 9.0) -> None:
        """Robust tracking (viso_set_robust): every frame the brightness chain
        tracks (set_brightness) weights each patch pixel by Huber's rule with
        this k (grey levels), so occluders and wrong map points stop bending the
        pose.  huber_k 0 = off; no effect while set_brightness is off."""
        self.ctx.set_robust(huber_k)

    def robust(self) -> np.ndarray:
        """viso_get_robust: int64[8] = on, frames tracked robustly, then of the
        last such frame: its down-weighted pixels, its level-0 n, 0..."""
        return self.ctx.get_robust()

    def robust_report(self) -> np.ndarray:
        """The last robust frame's report (28,), as Context.track_robust returns it."""
        return self.ctx.robust_report()

    def robust_weights(self) -> np.ndarray:
        """The last robust frame's weight mass per map point (64 = every patch
        pixel at full weight), in the map's order when that frame was tracked."""
        return self.ctx.robust_weights()

    def robust_log(self) -> np.ndarray:
        """One row per pose: mean weight, down-weighted pixels (NaN for frames
        not tracked robustly and for lost frames)."""
        return self.ctx.robust_log()

    def frame_status(self) -> np.ndarray:
        """viso_get_frame_status: one byte per pose: 0 tracked, 1 tracked with
        a bad verdict, 2 lost (the held pose), 3 recovered."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_frame_status", self.ctx.h, None, 0, ctypes.byref(n))
        st = np.zeros(max(int(n.value), 1), np.uint8)
        if n.value:
            _lib.call("viso_get_frame_status", self.ctx.h, st.ctypes.data, n.value, ctypes.byref(n))
        return st[:n.value]

    def set_rectify(self, cam: int = 0, **kw) -> None:
        """Rectification (viso_set_rectify): camera `cam` (0 left or mono, 1
        right) delivers raw frames of raw_size = (raw_width, raw_height), which
        are undistorted and rectified on the device into this context's
        pinhole image ahead of the pyramid.  kw: the arguments of
        viso_amd.rectify.params — model (RADTAN or TABLE), raw_size, fill, K_raw
        (the raw intrinsics), dist (k1, k2, p1, p2, k3), R (rectified -> raw
        rays: the transpose of OpenCV's R1 / R2), map (TABLE).  No kw, or
        model 0: off.  Only before the first frame."""
        from . import rectify as _rect
        if not kw or int(kw.get("model", _rect.RADTAN)) == _rect.OFF:
            _lib.call("viso_set_rectify", self.ctx.h, int(cam), None)
            return
        p, keep = _rect.params(**kw)
        if keep is not None and keep.shape[:2] != (self.height, self.width):
            raise ValueError("map must be (height, width, 2) of this context")
        _lib.call("viso_set_rectify", self.ctx.h, int(cam), ctypes.byref(p))  # (the map is copied)

    def rectify_info(self, cam: int = 0) -> np.ndarray:
        """viso_get_rectify: int64[8] = model, raw width, raw height, fill,
        outside pixels, clipped pixels, rectify launches, images rectified."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_rectify", self.ctx.h, int(cam), info.ctypes.data)
        return info

    def set_lk_warp(self, mode: int, max_area_ratio: float = 64.0) -> None:
        """Warped LK alignment (viso_set_lk_warp): every keyframe patch is
        warped into the current view by the affine map its point's depth and
        the two poses imply, and taken from the pyramid level that matches
        its scale; warps whose area ratio is outside [1 / max_area_ratio,
        max_area_ratio] are rejected.  mode 0 = off."""
        _lib.call("viso_set_lk_warp", self.ctx.h, int(mode), float(max_area_ratio))

    def lk_warp(self) -> np.ndarray:
        """viso_get_lk_warp: int64[8] = mode, frames aligned with it, then of
        the last row: paired, aligned, rejected warps, points with shift < 0,
        with shift > 0, skipped levels."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_lk_warp", self.ctx.h, info.ctypes.data)
        return info

    def lk_warp_rows(self):
        """The last frame's warp rows (viso_get_lk_warp_rows): A (n, 4) =
        A00, A01, A10, A11; shift (n,) int8; status (n,) uint8."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_lk_warp_rows", self.ctx.h, None, None, None, 0, ctypes.byref(n))
        A = np.zeros((n.value, 4), np.float64)
        shift, status = np.zeros(n.value, np.int8), np.zeros(n.value, np.uint8)
        if n.value:
            _lib.call("viso_get_lk_warp_rows", self.ctx.h, A.ctypes.data, shift.ctypes.data, status.ctypes.data,
                      n.value, ctypes.byref(n))
        return A, shift, status

    def set_lk_illum(self, mode: int, max_gain: float = 4.0) -> None:
        """Illumination-invariant LK alignment (viso_set_lk_illum): a
        per-patch gain and offset between the keyframe patch and the current
        image are projected out of the warped alignment; an aligned point
        whose gain is outside [1 / max_gain, max_gain] is failed (status 3).
        Runs while set_lk_warp is on; kept, inert, otherwise.  mode 0 = off."""
        _lib.call("viso_set_lk_illum", self.ctx.h, int(mode), float(max_gain))

    def lk_illum(self) -> np.ndarray:
        """viso_get_lk_illum: int64[8] = mode, frames aligned with it, then of
        the last row: paired, aligned, status-3 points, 0, 0, 0."""
        info = np.zeros(8, np.int64)
        _lib.call("viso_get_lk_illum", self.ctx.h, info.ctypes.data)
        return info

    def lk_illum_rows(self) -> np.ndarray:
        """The last frame's (gain, offset) rows (viso_get_lk_illum_rows):
        (n, 2), NaN where no level-0 iteration was accepted."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_lk_illum_rows", self.ctx.h, None, 0, ctypes.byref(n))
        go = np.zeros((n.value, 2), np.float64)
        if n.value:
            _lib.call("viso_get_lk_illum_rows", self.ctx.h, go.ctypes.data, n.value, ctypes.byref(n))
        return go

    def process_device(self, d_left: int, d_right: int | None, n: int, frame_stride: int):
        """Batched ingest of n frames resident in HBM (device pointers)."""
        _lib.call("viso_process_frames_device", self.ctx.h, d_left, d_right, n, frame_stride)

    # ----------------------------------------------------------- inspection
    @property
    def state(self) -> int:
        s = ctypes.c_int32(0)
        _lib.call("viso_get_state", self.ctx.h, ctypes.byref(s))
        return s.value

    def stats(self) -> np.ndarray:
        out = np.zeros(16)
        _lib.call("viso_get_frame_stats", self.ctx.h, out.ctypes.data)
        return out

    def config(self) -> dict:
        """viso_get_config: background LK, dedicated queues, pool size."""
        info = np.zeros(8, np.int32)
        _lib.call("viso_get_config", self.ctx.h, info.ctypes.data)
        return {"background_lk": int(info[0]), "lk_queue_dedicated": int(info[1]),
                "upload_queue_dedicated": int(info[2]), "slots": int(info[3]), "frame_log": int(info[4]),
                "batch_frames": int(info[5]), "tail_copy_bytes": int(info[6]), "tail_zero_ints": int(info[7])}

    def set_frame_log(self, on: bool = True) -> None:
        """Per-frame log (viso_set_frame_log): every tracking frame's level-0
        nGood / cost and LK pair / success counts, kept on the device."""
        _lib.call("viso_set_frame_log", self.ctx.h, 1 if on else 0)

    def frame_log(self) -> np.ndarray:
        """(poses, 4): level-0 nGood, level-0 cost, LK pairs, LK successes per
        tracking frame (row k = pose k); NaN for frames run with the log off."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_frame_log", self.ctx.h, None, 0, ctypes.byref(n))
        out = np.zeros((n.value, 4), np.float64)
        if n.value:
            _lib.call("viso_get_frame_log", self.ctx.h, out.ctypes.data, n.value, ctypes.byref(n))
        return out

    def keyframe_poses(self) -> np.ndarray:
        """The map's keyframe poses (viso_get_keyframe_poses): (keyframes, 12) Tcw."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_keyframe_poses", self.ctx.h, None, 0, ctypes.byref(n))
        out = np.zeros((n.value, 12), np.float64)
        if n.value:
            _lib.call("viso_get_keyframe_poses", self.ctx.h, out.ctypes.data, n.value, ctypes.byref(n))
        return out

    def tracks(self):
        """init_.kp1, init_.kp2 (float32 (n,2)) and init_.success."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_init_tracks", self.ctx.h, None, None, None, 0, ctypes.byref(n))
        m = n.value
        k1 = np.zeros((m, 2), np.float32)
        k2 = np.zeros((m, 2), np.float32)
        s = np.zeros(m, np.uint8)
        if m:
            _lib.call("viso_get_init_tracks", self.ctx.h, k1.ctypes.data, k2.ctypes.data,
                      s.ctypes.data, m, ctypes.byref(n))
        return k1, k2, s

    def alignment(self):
        """Last LKAlignment (dense per map point)."""
        n = ctypes.c_size_t(0)
        _lib.call("viso_get_alignment", self.ctx.h, None, None, None, None, 0, ctypes.byref(n))
        m = n.value
        pk = np.zeros(m, np.int32)
        sc = np.zeros(m, np.uint8)
        ub = np.zeros((m, 2))
        ua = np.zeros((m, 2))
        if m:
            _lib.call("viso_get_alignment", self.ctx.h, pk.ctypes.data, sc.ctypes.data,
                      ub.ctypes.data, ua.ctypes.data, m, ctypes.byref(n))
        return pk, sc, ub, ua

    def synchronize(self):
        self.ctx.synchronize()

    def close(self):
        self.ctx.close()


class FrameSequence:
    """FrameSequence (include/frame_sequence.h:11-43): reads
    ``<location><Keyframe.GetNextId()+1>.png`` (grey) per RunOnce()."""

    def __init__(self, location: str, handler: FrameHandler):
        self.location_ = location
        self.handler_ = handler

    def RunOnce(self) -> bool:
        path = os.path.join(self.location_, f"{Keyframe.GetNextId() + 1}.png")
        if not os.path.exists(path):
            return False  # the reference silently skips a missing file
        from .kitti import read_png  # cv::imread(path, 0) restated (include/viso/viso_io.h)
        self.handler_.OnNewFrame(Keyframe(read_png(path)))
        return True
