"""Cost and effect of the sliding-window map (viso_set_map_window) at
1242 x 375: the forward-driving synthetic sequence (tests/test_keyframes.py),
stereo insertion every `interval` frames with the gate always open, once with
the window and once without (the map then saturates at 16,384 points and 8
keyframes and insertion stops).

Two passes per configuration: host timers around viso_process_stereo +
viso_synchronize per frame, then HIP-event times of the direct pose and of the
retirement's launches (VISO_KERNEL_MAPWIN).  Prints one JSON line: per check
frame the windowed (retirement + insertion) and plain (insertion) times, their
difference per frame and its median, the retirement's event time, and the
per-frame tracking time of the last third of the run for both maps.

    python tools/bench_map_window.py [--frames 61] [--interval 5] [--window 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(left, right, K, baseline, interval, window, cell, events):
    import viso_amd
    h, w = left[0].shape
    v = viso_amd.Viso(*K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(baseline, 128, 1)
    v.set_keyframes(interval, 1000)
    if window:
        v.set_map_window(window, cell)
    if events:
        v.ctx.timing_enable(True)
        v.ctx.timing_select(["direct", "mapwin"])
    rows, t_d, t_m = [], 0.0, 0.0
    for f in range(len(left)):
        t0 = time.perf_counter()
        v.process(left[f], right[f])
        v.synchronize()
        dt = time.perf_counter() - t0
        st = v.stats()
        d = m = 0.0
        if events:
            d, m = v.ctx.timing("direct")[1], v.ctx.timing("mapwin")[1]
        rows.append({"frame": f, "ms": 1e3 * dt, "added": int(st[14]), "keyframes": int(st[15]), "ngood": int(st[9]),
                     "direct_ms": d - t_d, "mapwin_ms": m - t_m})
        t_d, t_m = d, m
    info = [int(x) for x in v.map_window()]
    n_pts = len(v.GetPoints())
    v.close()
    return rows, info, n_pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--interval", type=int, default=5)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--cell", type=int, default=16)
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    left = [seq.image(f) for f in range(a.frames)]
    right = [seq.image(f, 1) for f in range(a.frames)]
    args = (left, right, seq.K, seq.p.baseline, a.interval)
    run(left[:22], right[:22], seq.K, seq.p.baseline, a.interval, a.window, a.cell, False)  # warm-up
    win, info, n_win = run(*args, a.window, a.cell, False)
    plain, _, n_plain = run(*args, 0, a.cell, False)
    win_e, _, _ = run(*args, a.window, a.cell, True)
    plain_e, _, _ = run(*args, 0, a.cell, True)
    med = statistics.median
    r4 = lambda x: round(x, 4)  # noqa: E731
    retire_frames = [r["frame"] for r in win_e if r["mapwin_ms"] > 0]
    added = [win[f]["ms"] - plain[f]["ms"] for f in retire_frames]
    tail = range(2 * a.frames // 3, a.frames)
    track = [f for f in tail if f % a.interval]
    out = {
        "bench": "map_window", "size": [1242, 375], "frames": a.frames, "interval": a.interval, "window": a.window,
        "cell": a.cell, "retirement_frames": retire_frames,
        "check_frame_ms_window": [r4(win[f]["ms"]) for f in retire_frames],
        "check_frame_ms_plain": [r4(plain[f]["ms"]) for f in retire_frames],
        "points_added_plain": [plain[f]["added"] for f in retire_frames],
        "added_ms": [r4(x) for x in added], "added_ms_median": r4(med(added)) if added else None,
        "retire_launches_event_ms": [r4(win_e[f]["mapwin_ms"]) for f in retire_frames],
        "retire_launches_event_ms_median": r4(med([win_e[f]["mapwin_ms"] for f in retire_frames])) if retire_frames
        else None,
        "tracking_frames": [track[0], track[-1]],
        "tracking_frame_ms": {"window": r4(med([win[f]["ms"] for f in track])),
                              "plain": r4(med([plain[f]["ms"] for f in track]))},
        "tracking_direct_event_ms": {"window": r4(med([win_e[f]["direct_ms"] for f in track])),
                                     "plain": r4(med([plain_e[f]["direct_ms"] for f in track]))},
        "map_points_last": {"window": n_win, "plain": n_plain},
        "ngood_last": {"window": win[-1]["ngood"], "plain": plain[-1]["ngood"]},
        "map_window_info": info,
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash(),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
