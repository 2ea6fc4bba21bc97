"""Cost and effect of the warped LK alignment (viso_set_lk_warp) at 1242 x 375:
the forward-driving synthetic sequence (tests/test_pose_refine.py), a stereo
initialisation at frame 0, then left images only, in runs of equal length
with the mode off and on.

* rows: per tracking frame the points paired, the successes and the median
  | uv_after - uv_before | (the distance of the aligned position from the
  point's projection at the frame's pose) over the successes, off and on; with
  the mode on also the rejected warps, the shifted points and skipped levels.
* launch: HIP events around the LK launch of the same frames, off (the batched
  lk_align_kernel) and on (lk_warp_kernel).  Both runs have the point cull on
  with an interval that never comes (it only makes every frame's alignment run
  as a one-frame batched launch on the context stream), so both kernels see the
  same frames at the same poses.
* consumers: with point culling (5, 3, 2.0, 50) and point refinement
  (5, 5, 3, 1.0, 8.0, 3, 0.05) also on, off and on: the map size after the last
  frame and the eligible points of every refinement.
* the last pose against the synthetic ground truth (Sequence.pose), off and on
  (the mode by itself feeds nothing back, so these are equal) and with the
  consumers.

Writes profiles/lk_warp_cost.json (and prints it as one JSON line).

    python tools/bench_lk_warp.py [--frames 61] [--ratio 64] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_pose_refine import pose_error, t4  # noqa: E402

CULL = (5, 3, 2.0, 50)
PREFINE = (5, 5, 3, 1.0, 8.0, 3, 0.05)


def run(seq, left, right0, warp, cull=None, prefine=None, events=False):
    import viso_amd
    h, w = left[0].shape
    v = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    if cull:
        v.set_point_cull(*cull)
    if prefine:
        v.set_point_refine(*prefine)
    if warp:
        v.set_lk_warp(1, warp)
    v.process(left[0], right0)
    assert v.state == 1
    kernel = "lkwarp" if warp else "lkalign"
    if events:
        v.ctx.timing_enable(True)
        v.ctx.timing_select([kernel])
    rows, eligible = [], []
    prev = (0, 0.0)
    for f in range(1, len(left)):
        v.OnNewFrame(left[f])
        pk, sc, ub, ua = v.alignment()
        ok = sc == 1
        d = np.linalg.norm(ua - ub, axis=1)[ok]
        row = {"frame": f, "points": len(pk), "paired": int((pk >= 0).sum()), "success": int(ok.sum()),
               "median_shift_px": round(float(np.median(d)), 4) if ok.any() else None}
        if warp:
            info = [int(x) for x in v.lk_warp()]
            assert info[2] == row["paired"] and info[3] == row["success"]
            row.update(rejected=info[4], shift_neg=info[5], shift_pos=info[6], skipped_levels=info[7])
        if events:
            t = v.ctx.timing(kernel)
            row.update(launches=t[0] - prev[0], ms=t[1] - prev[1])
            prev = t
        if prefine and f % prefine[0] == 0:
            eligible.append(int(v.point_refine()[5]))
        rows.append(row)
    poses, n_map = v.poses, len(v.GetPoints())
    v.close()
    return rows, poses, n_map, eligible


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--ratio", type=float, default=64.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_warp_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    left = [seq.image(f) for f in range(a.frames)]
    right0 = seq.image(0, 1)
    never = (100000,) + CULL[1:]
    run(seq, left[:12], right0, a.ratio)  # warm-up
    run(seq, left[:12], right0, None)
    off, poses_off, _, _ = run(seq, left, right0, None)
    on, poses_on, _, _ = run(seq, left, right0, a.ratio)
    ev_off, p0, _, _ = run(seq, left, right0, None, cull=never, events=True)
    ev_on, p1, _, _ = run(seq, left, right0, a.ratio, cull=never, events=True)
    assert np.array_equal(p0, p1) and np.array_equal(p0, poses_off)
    assert all(r["launches"] == 1 for r in ev_off + ev_on)
    _, cp_off, map_off, el_off = run(seq, left, right0, None, cull=CULL, prefine=PREFINE)
    _, cp_on, map_on, el_on = run(seq, left, right0, a.ratio, cull=CULL, prefine=PREFINE)
    truth = t4(seq.pose(a.frames - 1)) @ np.linalg.inv(t4(seq.pose(0)))
    med = statistics.median
    r4 = lambda x: round(x, 4)  # noqa: E731

    def stat(rows):
        ms = [r["ms"] for r in rows]
        return {"median": r4(med(ms)), "min": r4(min(ms)), "max": r4(max(ms))}

    def err(p):
        e = pose_error(p[-1], truth)
        return {"translation": e[0], "rotation_deg": e[1]}

    s_off, s_on = stat(ev_off), stat(ev_on)
    keep = ("frame", "paired", "success", "median_shift_px", "rejected", "shift_neg", "shift_pos", "skipped_levels")
    out = {
        "bench": "lk_warp", "size": [1242, 375], "frames": a.frames, "tracking_frames": a.frames - 1,
        "max_area_ratio": a.ratio, "map_points": off[0]["points"],
        "rows_off": [{k: r[k] for k in keep if k in r} for r in off],
        "rows_on": [{k: r[k] for k in keep if k in r} for r in on],
        "poses_equal_off_on": bool(np.array_equal(poses_off, poses_on)),
        "lk_align_event_ms_per_frame": s_off, "lk_warp_event_ms_per_frame": s_on,
        "warp_over_align_median": r4(s_on["median"] / s_off["median"]),
        "with_cull_and_point_refine": {
            "cull": list(CULL), "point_refine": list(PREFINE),
            "off": {"map_size_last": map_off, "eligible_per_refinement": el_off, "last_pose_error": err(cp_off)},
            "on": {"map_size_last": map_on, "eligible_per_refinement": el_on, "last_pose_error": err(cp_on)}},
        "last_pose_error": {"off": err(poses_off), "on": err(poses_on)},
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
