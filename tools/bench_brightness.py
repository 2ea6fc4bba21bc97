"""Cost of the brightness-compensated tracking (viso_set_brightness,
viso_track_affine) at 1242 x 375 on the synthetic sequence: a
stereo initialisation at frame 0, then left images only, frame k of them
mapped to g_k I + o_k.

* tracking_on: host wall time per tracking frame and the chain's event time
  (viso:bright, one timed region of 4 (iterations + 1) + 1 launches per frame)
  over --frames frames with the mode on; the passes applied per level (the
  report rows' steps + 1 passes are computed per level) and the launches that
  found the chain finished.
* tracking_off_frames_finished_one_by_one: the same frames with the mode off
  but every frame finished inside its call (a point cull whose interval never
  comes), the comparison the other modes' sections use; tracking_off: the
  default path.
* per_pass: the stage entry at iterations 1..20 on one frame pair, whose chain
  grows by four launches per iteration while the passes applied stay: the
  slope is the cost of a launch that finds the chain finished; the cost of an
  applied pass follows from it.

Prints one JSON line (and appends it to --out).

    python tools/bench_brightness.py [--frames 41] [--repeat 9] [--out FILE]
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

W, H = 1242, 375
ITER = 10
NEVER_CULL = (100000, 3, 2.0, 50)
GO = [(1.0, 10.0), (0.75, 30.0), (0.5, 100.0), (1.0, -3.0), (0.75, -2.0), (0.5, 0.0), (1.0, 15.0), (0.5, 130.0)]


def gained(img, k):
    g, o = GO[k % len(GO)]
    v = (img & np.uint8(0xFC)).astype(np.float64) * g + o
    assert np.array_equal(v, np.rint(v)) and v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def viso(seq, bright=0, cull=None):
    import viso_amd
    v = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    if cull:
        v.set_point_cull(*cull)
    if bright:
        v.set_brightness(bright)
    v.process(seq.image(0), seq.image(0, 1))
    assert v.state == 1
    return v


def stat(ms):
    r4 = lambda x: round(float(x), 4)  # noqa: E731
    return {"median": r4(statistics.median(ms)), "min": r4(min(ms)), "max": r4(max(ms))}


def tracking_times(seq, images, bright, cull):
    name = "bright" if bright else "direct"
    v = viso(seq, bright, cull)
    v.ctx.timing_enable(True)
    v.ctx.timing_select([name])
    v.synchronize()
    wall = []
    for img in images:
        t0 = time.perf_counter()
        v.OnNewFrame(img)
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    v.synchronize()
    tail = (time.perf_counter() - t0) * 1e3
    regions, ms = v.ctx.timing(name)
    out = {"host_wall_ms_per_frame": stat(wall[2:]),
           "host_wall_ms_mean_with_final_sync": round((sum(wall) + tail) / len(wall), 4),
           name + "_event_ms_per_frame": round(ms / max(regions, 1), 4)}
    if bright:
        info, log = [int(x) for x in v.brightness()], v.brightness_log()
        chain = 4 * (bright + 1) + 1
        out.update(launches_per_frame=chain, info=info, steps_applied_per_frame=round(info[2] / max(info[1], 1), 3),
                   gain_offset_first_frames=[[round(float(x), 4) for x in r[:2]] for r in log[:8]],
                   last_report=[round(float(x), 6) for x in v.brightness_report()])
    poses = v.poses
    v.close()
    return out, poses


def per_pass(seq, points, repeat):
    """The stage entry's event time against the chain's length."""
    from viso_amd import api
    ctx = api.Context(api.default_params(*seq.K, width=W, height=H))
    last, cur = ctx.pyramid(seq.image(1))[0], ctx.pyramid(gained(seq.image(2), 2))[0]
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    ctx.timing_enable(True)
    ctx.timing_select(["bright"])
    rows = []
    for it in (1, 2, 5, 10, 15, 20):
        ms, prev = [], ctx.timing("bright")
        for _ in range(repeat + 1):
            _, rep = ctx.track_affine(last, cur, W, H, points, ident, ident, it)
            t = ctx.timing("bright")
            ms.append(t[1] - prev[1])
            prev = t
        steps = [int(x) for x in rep[5::4][:4]]
        # a level computes its applied steps' passes and the pass that ended it; exits 1 and 5 dropped one more
        passes = sum(s + (2 if e in (1, 5) else 1) for s, e in zip(steps, rep[4::4][:4]))
        rows.append({"iterations": it, "launches": 4 * (it + 1) + 1, "passes_computed": int(passes),
                     "steps_applied": steps, "exits": [int(x) for x in rep[4::4][:4]], "event_ms": stat(ms[1:])})
    ctx.close()
    # launches that found the chain finished cost the slope between the two longest chains whose passes agree
    a, b = rows[-2], rows[-1]
    out = {"rows": rows}
    if a["passes_computed"] == b["passes_computed"]:
        skip = (b["event_ms"]["median"] - a["event_ms"]["median"]) / (b["launches"] - a["launches"])
        out["skipped_launch_us"] = round(1e3 * skip, 3)
        out["applied_pass_us"] = round(1e3 * (b["event_ms"]["median"] - skip * (b["launches"] - b["passes_computed"]))
                                       / b["passes_computed"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "brightness_bench.jsonl"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(W, H, seed=0)
    v = viso(seq)
    points = v.GetPoints()
    v.close()
    images = [gained(seq.image(f), f) for f in range(1, a.frames)]
    tracking_times(seq, images[:8], ITER, None)  # warm-up
    tracking_times(seq, images[:8], 0, NEVER_CULL)
    # interleaved: off, one by one, on, twice
    runs = {"tracking_off": [], "tracking_off_frames_finished_one_by_one": [], "tracking_on": []}
    for _ in range(2):
        runs["tracking_off"].append(tracking_times(seq, images, 0, None)[0])
        runs["tracking_off_frames_finished_one_by_one"].append(tracking_times(seq, images, 0, NEVER_CULL)[0])
        runs["tracking_on"].append(tracking_times(seq, images, ITER, None)[0])
    out = {"bench": "brightness", "size": [W, H], "map_points": len(points), "iterations": ITER,
           "tracking_frames": len(images), **runs, "per_pass": per_pass(seq, points, a.repeat),
           "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash()}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
