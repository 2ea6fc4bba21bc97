"""Cost and effect of map point culling (viso_set_point_cull) at 1242 x 375:
the forward-driving synthetic sequence (tests/test_pose_refine.py), a stereo
initialisation at frame 0, then left images only, in runs of equal length with
the culling off and on.

Per configuration: host timers around viso_process_frame + viso_synchronize
per frame (a cull frame against a plain frame), then a run with HIP events on
the direct pose and on the record update / cull launches (VISO_KERNEL_CULL: a
plain frame's region is the update launch alone, a cull frame's the update and
the cull), the map size after every frame and the direct pose's timed
regions per frame (direct_launches_per_frame: one region a frame covers its
level launches, whose number does not depend on the map) with their time as
the map shrinks.  The translation (map units) and rotation (degrees) error of the last
pose is taken against the synthetic ground truth (Sequence.pose, relative to
frame 0, where the stereo initialisation puts the world frame).

Writes profiles/point_cull_cost.json (and prints it as one JSON line).

    python tools/bench_point_cull.py [--frames 61] [--interval 5] [--max-fail-run 3] [--reproj 2.0]
                                     [--min-points 50] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_pose_refine import pose_error, t4  # noqa: E402


def n_points(v):
    from viso_amd import _lib
    n = ctypes.c_size_t(0)
    _lib.call("viso_get_points", v.ctx.h, None, 0, ctypes.byref(n))
    return int(n.value)


def run(seq, left, right0, cull, events):
    import viso_amd
    h, w = left[0].shape
    v = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    if cull:
        v.set_point_cull(*cull)
    v.process(left[0], right0)
    assert v.state == 1
    if events:
        v.ctx.timing_enable(True)
        v.ctx.timing_select(["direct", "cull"])
    rows = []
    d_prev, c_prev = (0, 0.0), (0, 0.0)
    for f in range(1, len(left)):
        t0 = time.perf_counter()
        v.OnNewFrame(left[f])
        v.synchronize()
        dt = time.perf_counter() - t0
        row = {"frame": f, "ms": 1e3 * dt, "map": n_points(v)}
        if events:
            d, c = v.ctx.timing("direct"), v.ctx.timing("cull")
            row.update(direct_launches=d[0] - d_prev[0], direct_ms=d[1] - d_prev[1],
                       cull_launches=c[0] - c_prev[0], cull_ms=c[1] - c_prev[1])
            d_prev, c_prev = d, c
        rows.append(row)
    info = [int(x) for x in v.point_cull()]
    tracks = v.point_tracks() if cull else None
    poses = v.poses
    v.close()
    return rows, poses, info, tracks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--max-fail-run", type=int, default=3)
    ap.add_argument("--reproj", type=float, default=2.0)
    ap.add_argument("--min-points", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_cull_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    left = [seq.image(f) for f in range(a.frames)]
    right0 = seq.image(0, 1)
    cull = (a.interval, a.max_fail_run, a.reproj, a.min_points)
    run(seq, left[:12], right0, cull, False)  # warm-up
    off, poses_off, _, _ = run(seq, left, right0, None, False)
    on, poses_on, info, tracks = run(seq, left, right0, cull, False)
    off_e, _, _, _ = run(seq, left, right0, None, True)
    on_e, _, _, _ = run(seq, left, right0, cull, True)
    truth = t4(seq.pose(a.frames - 1)) @ np.linalg.inv(t4(seq.pose(0)))
    med = statistics.median
    r4 = lambda x: round(x, 4)  # noqa: E731
    is_cull = lambda r: r["frame"] % a.interval == 0  # noqa: E731
    upd = [r["cull_ms"] for r in on_e if not is_cull(r)]
    both = [r["cull_ms"] for r in on_e if is_cull(r)]
    e_off, e_on = pose_error(poses_off[-1], truth), pose_error(poses_on[-1], truth)
    out = {
        "bench": "point_cull", "size": [1242, 375], "frames": a.frames, "tracking_frames": a.frames - 1,
        "interval": a.interval, "max_fail_run": a.max_fail_run, "reproj_px": a.reproj, "min_points": a.min_points,
        "info": info,
        "update_event_ms_per_launch": {"median": r4(med(upd)), "min": r4(min(upd)), "max": r4(max(upd))},
        "update_and_cull_event_ms": {"median": r4(med(both)), "min": r4(min(both)), "max": r4(max(both))},
        "host_frame_ms_median": {
            "off": r4(med([r["ms"] for r in off])),
            "on_plain_frame": r4(med([r["ms"] for r in on if not is_cull(r)])),
            "on_cull_frame": r4(med([r["ms"] for r in on if is_cull(r)]))},
        "map_size_per_frame": {"off": [r["map"] for r in off], "on": [r["map"] for r in on]},
        "direct_launches_per_frame": {"off": [r["direct_launches"] for r in off_e],
                                      "on": [r["direct_launches"] for r in on_e]},
        "direct_event_ms_per_frame": {"off": [r4(r["direct_ms"]) for r in off_e],
                                      "on": [r4(r["direct_ms"]) for r in on_e]},
        "direct_event_ms_median": {"off": r4(med([r["direct_ms"] for r in off_e])),
                                   "on": r4(med([r["direct_ms"] for r in on_e]))},
        "final_records": {"points": int(len(tracks)), "never_found": int((tracks[:, 2] == 0).sum()),
                          "longest_fail_run": int(tracks[:, 3].max()) if len(tracks) else 0},
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
