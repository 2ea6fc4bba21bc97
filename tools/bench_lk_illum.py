"""Cost and effect of the illumination-invariant LK alignment
(viso_set_lk_illum) at 1242 x 375: the forward-driving synthetic sequence of
tools/bench_lk_warp.py, a stereo initialisation at frame 0, then left images
only, every tracking frame's exposure changed (g I + o on bytes that are
multiples of 4, cycling through EXPOSURES), with the brightness chain
(viso_set_brightness) and the warped alignment on, in runs of equal length
with the mode off (lk_warp_kernel<false>) and on (lk_warp_kernel<true>).

* rows: per tracking frame its (g, o), the points paired, the successes and
  the median | uv_after - uv_before | over the successes, off and on; with the
  mode on also the status-3 points and the median gain and offset reported.
* launch: HIP events around the one-frame launch of the warped kernel on the
  same frames at the same poses (the mode feeds nothing back), off and on.

Writes profiles/lk_illum_cost.json (and prints it as one JSON line).

    python tools/bench_lk_illum.py [--frames 61] [--max-gain 4] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXPOSURES = ((1.0, 10.0), (0.75, 30.0), (0.5, 100.0), (1.0, -3.0), (0.75, -2.0), (0.5, 0.0), (1.0, 15.0),
             (0.5, 120.0), (0.75, 12.0), (1.0, 0.0))
RATIO = 64.0
BRIGHT_ITER = 10


def exposed(img, g, o):
    v = (img & np.uint8(0xFC)).astype(np.float64) * g + o
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def run(seq, left, right0, max_gain, events=False):
    import viso_amd
    h, w = left[0].shape
    v = viso_amd.Viso(*seq.K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    v.set_brightness(BRIGHT_ITER)
    v.set_lk_warp(1, RATIO)
    if max_gain:
        v.set_lk_illum(1, max_gain)
    v.process(left[0], right0)
    assert v.state == 1
    if events:
        v.ctx.timing_enable(True)
        v.ctx.timing_select(["lkwarp"])
    rows, prev = [], (0, 0.0)
    for f in range(1, len(left)):
        v.OnNewFrame(left[f])
        pk, sc, ub, ua = v.alignment()
        ok = sc == 1
        d = np.linalg.norm(ua - ub, axis=1)[ok]
        g, o = EXPOSURES[(f - 1) % len(EXPOSURES)]
        row = {"frame": f, "g": g, "o": o, "points": len(pk), "paired": int((pk >= 0).sum()),
               "success": int(ok.sum()), "median_shift_px": round(float(np.median(d)), 4) if ok.any() else None}
        if max_gain:
            info = [int(x) for x in v.lk_illum()]
            assert info[2] == row["paired"] and info[3] == row["success"]
            go = v.lk_illum_rows()[ok]
            row.update(status3=info[4], median_gain=round(float(np.median(go[:, 0])), 4) if ok.any() else None,
                       median_offset=round(float(np.median(go[:, 1])), 2) if ok.any() else None)
        if events:
            t = v.ctx.timing("lkwarp")
            row.update(launches=t[0] - prev[0], ms=t[1] - prev[1])
            prev = t
        rows.append(row)
    poses = v.poses
    v.close()
    return rows, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--max-gain", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lk_illum_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    left = [seq.image(0)] + [exposed(seq.image(f), *EXPOSURES[(f - 1) % len(EXPOSURES)]) for f in range(1, a.frames)]
    right0 = seq.image(0, 1)
    run(seq, left[:12], right0, a.max_gain)  # warm-up
    run(seq, left[:12], right0, None)
    ev_off, p0 = run(seq, left, right0, None, events=True)
    ev_on, p1 = run(seq, left, right0, a.max_gain, events=True)
    assert np.array_equal(p0, p1)
    assert all(r["launches"] == 1 for r in ev_off + ev_on)
    med = statistics.median
    r4 = lambda x: round(x, 4)  # noqa: E731

    def stat(rows):
        ms = [r["ms"] for r in rows]
        return {"median": r4(med(ms)), "min": r4(min(ms)), "max": r4(max(ms))}

    s_off, s_on = stat(ev_off), stat(ev_on)
    keep = ("frame", "g", "o", "paired", "success", "median_shift_px", "status3", "median_gain", "median_offset", "ms")
    out = {
        "bench": "lk_illum", "size": [1242, 375], "frames": a.frames, "tracking_frames": a.frames - 1,
        "max_area_ratio": RATIO, "max_gain": a.max_gain, "brightness_iterations": BRIGHT_ITER,
        "map_points": ev_off[0]["points"],
        "rows_off": [{k: (r4(r[k]) if k == "ms" else r[k]) for k in keep if k in r} for r in ev_off],
        "rows_on": [{k: (r4(r[k]) if k == "ms" else r[k]) for k in keep if k in r} for r in ev_on],
        "poses_equal_off_on": True,
        "lk_warp_false_event_ms_per_frame": s_off, "lk_warp_true_event_ms_per_frame": s_on,
        "true_over_false_median": r4(s_on["median"] / s_off["median"]),
        "success_sum": {"off": sum(r["success"] for r in ev_off), "on": sum(r["success"] for r in ev_on)},
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash(),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
