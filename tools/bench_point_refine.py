"""Cost and effect of the point refinement (viso_set_point_refine) at
1242 x 375: the forward-driving synthetic sequence (tests/test_pose_refine.py),
a stereo initialisation at frame 0, then left images only, in runs of equal
length with the refinement off and on.

Per configuration: host timers around viso_process_frame + viso_synchronize
per frame (a refinement frame against a plain frame), then a run with HIP
events on the record / refine launches (VISO_KERNEL_POINTS: a plain frame's
region is the record launch alone, a refinement frame's the record and the
refine launch).  Per refinement: the eligible, moved and status-4 counts
(viso_get_point_refine) and the median cost of the moved points before and
after, from the stage entry (viso_points_refine) on the ring rebuilt on the
host from the frames' poses and LK rows — its counts must equal the frame
path's.  The translation (map units) and rotation (degrees) error of the last
pose is taken against the synthetic ground truth (Sequence.pose, relative to
frame 0, where the stereo initialisation puts the world frame).

Writes profiles/point_refine_cost.json (and prints it as one JSON line).

    python tools/bench_point_refine.py [--frames 61] [--interval 5] [--window 5] [--iterations 3]
                                       [--huber 1.0] [--max-shift 8.0] [--min-obs 3] [--sigma 0.05]
                                       [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_pose_refine import pose_error, t4  # noqa: E402


def run(seq, left, right0, prefine, events, follow):
    """follow: rebuild the ring on the host and run the stage entry beside
    every refinement (no map change happens in these runs: one keyframe, the
    ring is never emptied)."""
    import viso_amd
    h, w = left[0].shape
    v = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    if prefine:
        v.set_point_refine(*prefine)
    v.process(left[0], right0)
    assert v.state == 1
    if events:
        v.ctx.timing_enable(True)
        v.ctx.timing_select(["points"])
    rows, refinements = [], []
    p_prev = (0, 0.0)
    ring, count = {}, 0
    for f in range(1, len(left)):
        before = v.GetPoints() if follow else None
        t0 = time.perf_counter()
        v.OnNewFrame(left[f])
        v.synchronize()
        dt = time.perf_counter() - t0
        row = {"frame": f, "ms": 1e3 * dt}
        if events:
            p = v.ctx.timing("points")
            row.update(points_launches=p[0] - p_prev[0], points_ms=p[1] - p_prev[1])
            p_prev = p
        rows.append(row)
        if follow:
            interval, window, iterations, huber, shift, min_obs, sigma = prefine
            pk, sc, ub, ua = v.alignment()
            valid, uv = v.ctx.point_obs_record(pk, sc, ub, ua, shift)
            ring[count % window] = (v.poses[-1], valid, uv, pk)
            count += 1
            if f % interval == 0:
                m = min(count, window)
                anchor = np.max(np.stack([ring[s][3] for s in range(m)]), 0)  # (a flagged point was paired)
                g = v.ctx.refine_points(before, anchor, v.keyframe_poses(), [ring[s][0] for s in range(m)],
                                        np.stack([ring[s][1] for s in range(m)]),
                                        np.stack([ring[s][2] for s in range(m)]), iterations, huber, min_obs, sigma)
                info = [int(x) for x in v.point_refine()]
                assert info[5:8] == g["counts"][:3], (info, g["counts"])
                assert np.array_equal(g["points"], v.GetPoints())
                mv = g["steps"] >= 1
                refinements.append({
                    "frame": f, "eligible": info[5], "moved": info[6], "status_4": info[7],
                    "status_2": g["counts"][3],
                    "median_cost_moved_before": float(np.median(g["costs"][mv, 0])) if mv.any() else None,
                    "median_cost_moved_after": float(np.median(g["costs"][mv, 1])) if mv.any() else None})
    info = [int(x) for x in v.point_refine()]
    poses = v.poses
    v.close()
    return rows, poses, info, refinements


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--huber", type=float, default=1.0)
    ap.add_argument("--max-shift", type=float, default=8.0)
    ap.add_argument("--min-obs", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_refine_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    left = [seq.image(f) for f in range(a.frames)]
    right0 = seq.image(0, 1)
    prefine = (a.interval, a.window, a.iterations, a.huber, a.max_shift, a.min_obs, a.sigma)
    run(seq, left[:12], right0, prefine, False, False)  # warm-up
    off, poses_off, _, _ = run(seq, left, right0, None, False, False)
    on, poses_on, info, _ = run(seq, left, right0, prefine, False, False)
    on_e, _, _, _ = run(seq, left, right0, prefine, True, False)
    _, poses_f, info_f, refinements = run(seq, left, right0, prefine, False, True)
    assert np.array_equal(poses_f, poses_on) and info_f == info
    truth = t4(seq.pose(a.frames - 1)) @ np.linalg.inv(t4(seq.pose(0)))
    med = statistics.median
    r4 = lambda x: round(x, 4)  # noqa: E731
    is_ref = lambda r: r["frame"] % a.interval == 0  # noqa: E731
    rec = [r["points_ms"] for r in on_e if not is_ref(r)]
    both = [r["points_ms"] for r in on_e if is_ref(r)]
    assert all(r["points_launches"] == (2 if is_ref(r) else 1) for r in on_e)
    e_off, e_on = pose_error(poses_off[-1], truth), pose_error(poses_on[-1], truth)
    out = {
        "bench": "point_refine", "size": [1242, 375], "frames": a.frames, "tracking_frames": a.frames - 1,
        "interval": a.interval, "window": a.window, "iterations": a.iterations, "huber_px": a.huber,
        "max_shift_px": a.max_shift, "min_obs": a.min_obs, "max_rel_sigma": a.sigma,
        "info": info,
        "record_event_ms_per_launch": {"median": r4(med(rec)), "min": r4(min(rec)), "max": r4(max(rec))},
        "record_and_refine_event_ms": {"median": r4(med(both)), "min": r4(min(both)), "max": r4(max(both))},
        "refine_event_ms_less_median_record": {"median": r4(med(both) - med(rec)), "min": r4(min(both) - med(rec)),
                                               "max": r4(max(both) - med(rec))},
        "host_frame_ms_median": {
            "off": r4(med([r["ms"] for r in off])),
            "on_plain_frame": r4(med([r["ms"] for r in on if not is_ref(r)])),
            "on_refinement_frame": r4(med([r["ms"] for r in on if is_ref(r)]))},
        "refinements": refinements,
        "last_pose_error": {"off": {"translation": e_off[0], "rotation_deg": e_off[1]},
                            "on": {"translation": e_on[0], "rotation_deg": e_on[1]}},
        "translation_truth_norm": float(np.linalg.norm(truth[:3, 3])),
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash(),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
