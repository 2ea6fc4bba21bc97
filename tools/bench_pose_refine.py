"""Cost and effect of the pose refinement (viso_set_pose_refine) at 1242 x 375:
the forward-driving synthetic sequence (tests/test_keyframes.py), a stereo
initialisation at frame 0, then left images only, in runs of equal length with
the refinement off and on.

Per configuration: host timers around viso_process_frame + viso_synchronize
per frame; one device-ingest chunk of the same frames (viso_process_frames_
device), wall time per frame; then HIP-event times of the direct pose and of
the refine launch (VISO_KERNEL_REFINE) with the report of every frame.  The
translation (map units) and rotation (degrees) error of the last pose is taken
against the synthetic ground truth (Sequence.pose, relative to frame 0, where
the stereo initialisation puts the world frame).

Writes profiles/pose_refine_cost.json (and prints it as one JSON line).

    python tools/bench_pose_refine.py [--frames 61] [--iterations 5] [--huber 1.0] [--max-shift 8.0]
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


def t4(p):
    m = np.eye(4)
    m[:3, :3] = np.asarray(p[:9]).reshape(3, 3)
    m[:3, 3] = p[9:]
    return m


def pose_error(pose, truth):
    """(translation, rotation in degrees) of pose * truth^-1."""
    d = t4(pose) @ np.linalg.inv(truth)
    c = min(1.0, max(-1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))
    return float(np.linalg.norm(d[:3, 3])), float(np.degrees(np.arccos(c)))


def make(seq, left0, right0, refine):
    import viso_amd
    h, w = left0.shape
    v = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    if refine:
        v.set_pose_refine(*refine)
    v.process(left0, right0)
    assert v.state == 1
    return v


def run_host(seq, left, right0, refine, events):
    v = make(seq, left[0], right0, refine)
    if events:
        v.ctx.timing_enable(True)
        v.ctx.timing_select(["direct", "refine"])
    rows, t_d, t_r = [], 0.0, 0.0
    for f in range(1, len(left)):
        t0 = time.perf_counter()
        v.OnNewFrame(left[f])
        v.synchronize()
        dt = time.perf_counter() - t0
        row = {"frame": f, "ms": 1e3 * dt}
        if events:
            d, r = v.ctx.timing("direct")[1], v.ctx.timing("refine")[1]
            row.update(direct_ms=d - t_d, refine_ms=r - t_r)
            t_d, t_r = d, r
            if refine:
                row["report"] = [float(x) for x in v.pose_refine()]
        rows.append(row)
    launches = v.ctx.timing("refine")[0] if events else 0
    poses, n_pts = v.poses, len(v.GetPoints())
    v.close()
    return rows, poses, n_pts, launches


def run_device(seq, left, right0, refine, d_frames):
    import torch
    v = make(seq, left[0], right0, refine)
    v.synchronize()
    h, w = left[0].shape
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v.process_device(d_frames.data_ptr(), None, len(left) - 1, w * h)
    v.synchronize()
    dt = time.perf_counter() - t0
    poses = v.poses
    v.close()
    return 1e3 * dt / (len(left) - 1), poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--huber", type=float, default=1.0)
    ap.add_argument("--max-shift", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    left = [seq.image(f) for f in range(a.frames)]
    right0 = seq.image(0, 1)
    refine = (a.iterations, a.huber, a.max_shift)
    d_frames = torch.from_numpy(np.stack(left[1:])).cuda()
    run_host(seq, left[:12], right0, refine, False)  # warm-up
    run_device(seq, left[:12], right0, refine, d_frames)
    off, poses_off, n_pts, _ = run_host(seq, left, right0, None, False)
    on, poses_on, _, _ = run_host(seq, left, right0, refine, False)
    off_e, _, _, _ = run_host(seq, left, right0, None, True)
    on_e, _, _, launches = run_host(seq, left, right0, refine, True)
    dev_off, _ = run_device(seq, left, right0, None, d_frames)
    dev_on, dposes_on = run_device(seq, left, right0, refine, d_frames)
    truth = t4(seq.pose(a.frames - 1)) @ np.linalg.inv(t4(seq.pose(0)))
    med = statistics.median
    r4 = lambda x: round(x, 4)  # noqa: E731
    reports = np.array([r["report"] for r in on_e])
    status = [int(s) for s in reports[:, 5]]
    e_off, e_on = pose_error(poses_off[-1], truth), pose_error(poses_on[-1], truth)
    out = {
        "bench": "pose_refine", "size": [1242, 375], "frames": a.frames, "tracking_frames": a.frames - 1,
        "iterations": a.iterations, "huber_px": a.huber, "max_shift_px": a.max_shift, "map_points": n_pts,
        "host_frame_ms_median": {"off": r4(med([r["ms"] for r in off])), "on": r4(med([r["ms"] for r in on]))},
        "device_chunk_ms_per_frame": {"off": r4(dev_off), "on": r4(dev_on)},
        "direct_event_ms_median": {"off": r4(med([r["direct_ms"] for r in off_e])),
                                   "on": r4(med([r["direct_ms"] for r in on_e]))},
        "refine_launches": launches,
        "refine_event_ms_per_launch": {"median": r4(med([r["refine_ms"] for r in on_e])),
                                       "min": r4(min(r["refine_ms"] for r in on_e)),
                                       "max": r4(max(r["refine_ms"] for r in on_e))},
        "observations_per_frame": {"median": int(med(reports[:, 0])), "min": int(reports[:, 0].min()),
                                   "max": int(reports[:, 0].max())},
        "steps_per_frame_median": int(med(reports[:, 1])),
        "status_counts": {str(s): status.count(s) for s in sorted(set(status))},
        "rms_px_median": {"at_direct_pose": r4(med(reports[:, 6])), "at_result": r4(med(reports[:, 7]))},
        "last_pose_error": {"off": {"translation": e_off[0], "rotation_deg": e_off[1]},
                            "on": {"translation": e_on[0], "rotation_deg": e_on[1]}},
        "translation_truth_norm": float(np.linalg.norm(truth[:3, 3])),
        "ingest_forms_bit_equal_on": bool(np.array_equal(poses_on, dposes_on)),
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash(),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
