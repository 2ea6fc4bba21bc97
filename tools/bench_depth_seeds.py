"""Cost and effect of the depth seeds (viso_set_depth_seeds) at 1242 x 375: the
forward-driving synthetic sequence (tests/test_pose_refine.py), a stereo
initialisation at frame 0, then left images only.

* rows: every 10th tracking frame the live seeds, the points promoted and the
  seeds dropped so far, and the map size with the mode off, on, and on together
  with the warp, the point cull (5, 3, 2.0, 50) and the point refinement
  (5, 5, 3, 1.0, 8.0, 3, 0.05) (beside that combination without the seeds).
  Without an insertion mode the only keyframe is frame 0, whose stereo map
  covers nearly every cell, so the same columns are also taken with the
  monocular insertion (10, 1000, 16, 0.25) on, which creates keyframes, and
  seeds of 8-pixel cells.
* launch: HIP events around the seed launches of every frame (the update; on a
  promotion frame the promotion too), beside lk_warp_kernel's launch on the
  same frames (the warp and the monocular insertion on in that run).
* a check frame that promotes against a plain tracking frame (host time of
  viso_process_frame, synchronised).
* the last pose against the synthetic ground truth, off and on.

Writes profiles/depth_seeds_cost.json (and prints it as one JSON line).

    python tools/bench_depth_seeds.py [--frames 61] [--interval 5] [--out FILE]
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

MONO = (10, 1000, 16, 0.25)
CULL = (5, 3, 2.0, 50)
PREFINE = (5, 5, 3, 1.0, 8.0, 3, 0.05)
WARP = 64.0


def seed_params(interval, cell=16):
    return dict(interval=interval, cell=cell, max_steps=32, depth_min=2.0, depth_max=60.0, max_score=57600.0,
                uniqueness=1.5, min_good=3, conv_rel=0.15, max_bad=4, max_lost=4)


def run(seq, left, right0, seeds=None, combo=False, warp=False, events=False, mono=False):
    import viso_amd
    h, w = left[0].shape
    v = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    if combo:
        v.set_point_cull(*CULL)
        v.set_point_refine(*PREFINE)
    if combo or warp:
        v.set_lk_warp(1, WARP)
    if mono:
        v.set_mono_keyframes(*MONO)
    if seeds:
        v.set_depth_seeds(**seeds)
    v.process(left[0], right0)
    assert v.state == 1
    if events:
        v.ctx.timing_enable(True)
        v.ctx.timing_select(["seeds", "lkwarp"])
    rows = []
    prev = {"seeds": (0, 0.0), "lkwarp": (0, 0.0)}
    for f in range(1, len(left)):
        v.synchronize()
        t0 = time.perf_counter()
        v.OnNewFrame(left[f])
        v.synchronize()
        row = {"frame": f, "host_ms": (time.perf_counter() - t0) * 1e3, "map": len(v.GetPoints())}
        if seeds:
            info = [int(x) for x in v.depth_seeds()]
            row.update(live=info[1], created=info[2], promoted=info[3], dropped=info[4], fused=info[5], bad=info[6],
                       lost=info[7])
        if events:
            for k in prev:
                t = v.ctx.timing(k)
                row[k + "_launches"], row[k + "_ms"] = t[0] - prev[k][0], t[1] - prev[k][1]
                prev[k] = t
        rows.append(row)
    poses = v.poses
    v.close()
    return rows, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_seeds_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    left = [seq.image(f) for f in range(a.frames)]
    right0 = seq.image(0, 1)
    sp = seed_params(a.interval)
    run(seq, left[:12], right0, sp)  # warm-up
    run(seq, left[:12], right0)
    off, poses_off = run(seq, left, right0)
    on, poses_on = run(seq, left, right0, sp)
    combo_off, cp_off = run(seq, left, right0, combo=True)
    combo_on, cp_on = run(seq, left, right0, sp, combo=True)
    sp8 = seed_params(a.interval, 8)
    mono_off, mp_off = run(seq, left, right0, mono=True)
    mono_on, mp_on = run(seq, left, right0, sp8, mono=True)
    mcombo_off, _ = run(seq, left, right0, combo=True, mono=True)
    mcombo_on, _ = run(seq, left, right0, sp8, combo=True, mono=True)
    ev, _ = run(seq, left, right0, sp8, warp=True, events=True, mono=True)
    truth = t4(seq.pose(a.frames - 1)) @ np.linalg.inv(t4(seq.pose(0)))
    med = statistics.median
    r4 = lambda x: round(x, 4)  # noqa: E731

    def stat(xs):
        return {"median": r4(med(xs)), "min": r4(min(xs)), "max": r4(max(xs))} if xs else None

    def err(p):
        e = pose_error(p[-1], truth)
        return {"translation": e[0], "rotation_deg": e[1]}

    promo = [r for r in ev if r["frame"] % a.interval == 0]
    plain = [r for r in ev if r["frame"] % a.interval != 0]
    # (a plain frame's seed launch is the update alone)
    both = [r for r in plain if r["seeds_launches"] == 1 and r["lkwarp_launches"] == 1]
    upd = [r["seeds_ms"] for r in both]
    lkw = [r["lkwarp_ms"] for r in both]
    table = []
    for i in range(9, len(on), 10):
        table.append({"frame": on[i]["frame"], "live": on[i]["live"], "created": on[i]["created"],
                      "promoted": on[i]["promoted"], "dropped": on[i]["dropped"], "map_off": off[i]["map"],
                      "map_on": on[i]["map"], "map_combo_off": combo_off[i]["map"], "map_combo_on": combo_on[i]["map"]})
    table_mono = []
    for i in range(9, len(mono_on), 10):
        r = mono_on[i]
        table_mono.append({"frame": r["frame"], "live": r["live"], "created": r["created"], "promoted": r["promoted"],
                           "dropped": r["dropped"], "fused": r["fused"], "bad": r["bad"], "lost": r["lost"],
                           "map_off": mono_off[i]["map"], "map_on": r["map"], "map_combo_off": mcombo_off[i]["map"],
                           "map_combo_on": mcombo_on[i]["map"], "live_combo_on": mcombo_on[i]["live"],
                           "promoted_combo_on": mcombo_on[i]["promoted"]})
    out = {
        "bench": "depth_seeds", "size": [1242, 375], "frames": a.frames, "tracking_frames": a.frames - 1,
        "seeds": sp, "cull": list(CULL), "point_refine": list(PREFINE), "warp_ratio": WARP, "rows": table,
        "mono_insertion": list(MONO), "seeds_with_mono_insertion": sp8, "rows_with_mono_insertion": table_mono,
        "update_frames_timed": len(both),
        "update_ms_and_seeds_per_frame": [[r["frame"], r["live"], r4(r["seeds_ms"]), r4(r["lkwarp_ms"]),
                                           r["map"]] for r in both],
        "seed_update_event_ms": stat(upd), "lk_warp_event_ms": stat(lkw),
        "update_over_lk_warp_median": r4(med(upd) / med(lkw)) if upd and lkw else None,
        "seeds_at_update_median": int(med([r["live"] for r in both])) if both else 0,
        "map_points_at_update_median": int(med([r["map"] for r in both])) if both else 0,
        "promotion_frame_seed_event_ms": stat([r["seeds_ms"] for r in promo]),
        "host_ms_plain_frame": stat([r["host_ms"] for r in plain]),
        "host_ms_promotion_frame": stat([r["host_ms"] for r in promo]),
        "host_ms_frame_mode_off": stat([r["host_ms"] for r in off]),
        "last_pose_error": {"off": err(poses_off), "on": err(poses_on), "combo_off": err(cp_off),
                            "combo_on": err(cp_on), "mono_off": err(mp_off), "mono_on": err(mp_on)},
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
