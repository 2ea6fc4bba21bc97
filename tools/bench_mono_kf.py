"""Cost of a monocular keyframe insertion (viso_set_mono_keyframes) at
1242 x 375: host timers around viso_process_frame + viso_synchronize, per
frame, on the forward-driving synthetic sequence (tests/test_keyframes.py).

Three kinds of frame: a plain tracking frame, a check frame whose gate stays
closed (ngood_permille = 0: the nGood read-back alone) and a check frame that
inserts (ngood_permille = 1000).  Prints one JSON line with the medians, the
points added per insertion (the tracker's own poses), the device and the
library's source hash.

    python tools/bench_mono_kf.py [--frames 61] [--interval 10] [--ba 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def run(images, right0, K, interval, permille, cell, parallax, ba):
    import viso_amd
    h, w = images[0].shape
    v = viso_amd.Viso(*K, width=w, height=h, enable_tracking=1, batch_frames=32)
    v.set_stereo(run.baseline, 128, 1)
    v.set_mono_keyframes(interval, permille, cell, parallax)
    if ba:
        v.set_bundle_adjust(ba)
    v.process(images[0], right0)
    v.synchronize()
    rows = []
    for f in range(1, len(images)):
        t0 = time.perf_counter()
        v.OnNewFrame(images[f])
        v.synchronize()
        dt = time.perf_counter() - t0
        st = v.stats()
        rows.append((f, 1e3 * dt, int(st[14]), int(st[15]), int(st[9])))
    n_pts = len(v.GetPoints())
    v.close()
    return rows, n_pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=61)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--parallax", type=float, default=0.25)
    ap.add_argument("--ba", type=int, default=0)
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(1242, 375, seed=0, z_amp=20.0, z_period=1000.0)
    run.baseline = seq.p.baseline
    images = [seq.image(f) for f in range(a.frames)]
    right0 = seq.image(0, 1)
    run(images[:12], right0, seq.K, a.interval, 1000, a.cell, a.parallax, a.ba)  # warm-up (code objects, pools)
    closed, _ = run(images, right0, seq.K, a.interval, 0, a.cell, a.parallax, a.ba)
    opened, n_pts = run(images, right0, seq.K, a.interval, 1000, a.cell, a.parallax, a.ba)
    med = statistics.median
    plain = [r[1] for r in closed if r[0] % a.interval]
    check = [r[1] for r in closed if r[0] % a.interval == 0]
    insert = [r[1] for r in opened if r[2] > 0]
    out = {
        "bench": "mono_kf", "size": [1242, 375], "frames": a.frames, "interval": a.interval, "cell": a.cell,
        "min_parallax_deg": a.parallax, "ba_iterations": a.ba,
        "plain_frame_ms": round(med(plain), 4), "check_frame_ms": round(med(check), 4),
        "insert_frame_ms": round(med(insert), 4) if insert else None,
        "insert_frame_ms_all": [round(x, 4) for x in insert],
        "points_added": [r[2] for r in opened if r[2] > 0], "keyframes": opened[-1][3], "map_points": n_pts,
        "ngood_last": {"inserting": opened[-1][4], "frozen": closed[-1][4]},
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash(),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
