"""Cost of robust tracking (viso_set_robust) at 1242 x 375 on
the synthetic sequence: frame k mapped to tools/bench_brightness.py's g_k I +
o_k (clipped to bytes), with a block of every frame replaced by the frame's own texture
from elsewhere, the occluder the weights are for.

* brightness_alone: host wall time per tracking frame and the chain's event
  time (viso:bright) with viso_set_brightness(10) alone.
* robust_on: the same frames with viso_set_robust(k) as well; the mean weight
  and the down-weighted pixels of the first frames from the robust log.

The two are run interleaved, --rounds times each.  With --plain-only only
brightness_alone is run: the form for a library of an earlier revision (named
by VISO_LIB), whose lines are the comparison on the same box.

Prints one JSON line (and appends it to --out).

    python tools/bench_robust.py [--frames 41] [--rounds 3] [--k 9] [--label NAME] [--plain-only] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_brightness import GO, H, ITER, W, stat  # noqa: E402

BLOCK = (slice(100, 300), slice(450, 800))  # 15 % of the image


def gained(img, k):
    """Frame k mapped to g_k I + o_k, clipped to bytes."""
    g, o = GO[k % len(GO)]
    return np.clip(np.rint(img.astype(np.float64) * g + o), 0, 255).astype(np.uint8)


def occluded(img):
    img = img.copy()
    img[BLOCK] = np.roll(np.roll(img, -23, axis=1), 17, axis=0)[BLOCK]
    return img


def tracking_times(seq, images, k):
    import viso_amd
    v = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    v.set_brightness(ITER)
    if k:
        v.set_robust(k)
    v.process(seq.image(0), seq.image(0, 1))
    assert v.state == 1
    v.ctx.timing_enable(True)
    v.ctx.timing_select(["bright"])
    v.synchronize()
    wall = []
    for img in images:
        t0 = time.perf_counter()
        v.OnNewFrame(img)
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    v.synchronize()
    tail = (time.perf_counter() - t0) * 1e3
    regions, ms = v.ctx.timing("bright")
    info = [int(x) for x in v.brightness()]
    out = {"host_wall_ms_per_frame": stat(wall[2:]),
           "host_wall_ms_mean_with_final_sync": round((sum(wall) + tail) / len(wall), 4),
           "bright_event_ms_per_frame": round(ms / max(regions, 1), 4), "map_points": len(v.GetPoints()),
           "steps_applied_per_frame": round(info[2] / max(info[1], 1), 3)}
    if k:
        out.update(info=[int(x) for x in v.robust()],
                   mean_weight_and_down_weighted_first_frames=[[round(float(x), 4) for x in r]
                                                                for r in v.robust_log()[:8]])
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--k", type=float, default=9.0)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_bench_ab.jsonl"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(W, H, seed=0)
    images = [occluded(gained(seq.image(f), f)) for f in range(1, a.frames)]
    tracking_times(seq, images[:8], 0)  # warm-up
    runs = {"brightness_alone": []}
    if not a.plain_only:
        tracking_times(seq, images[:8], a.k)
        runs["robust_on"] = []
    for _ in range(a.rounds):
        runs["brightness_alone"].append(tracking_times(seq, images, 0))
        if not a.plain_only:
            runs["robust_on"].append(tracking_times(seq, images, a.k))
    out = {"bench": "robust", "label": a.label, "size": [W, H], "iterations": ITER, "huber_k": a.k,
           "tracking_frames": len(images), **runs, "device": torch.cuda.get_device_name(0),
           "source_hash": _lib.built_hash()}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
