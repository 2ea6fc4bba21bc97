#!/usr/bin/env python3
"""Rectification microbenchmark (dev tool, GPU box): the batched rectify launch
against the pyramid launches of the same chunk, in one process.

Times, by the library's device events around the launch (viso_timing_get), the
rectify launch of a 20-frame and a 64-frame chunk of 1242x375 and of one
1920x1080 frame, both models (RADTAN computes the coordinates, TABLE reads
8 B/pixel), through the stage entry (viso_rectify: the frame path's launch),
and the pyramid launches (viso_pyramid: level 1 and the tail) of the same
images, and of those the level-1 launch alone (VISO_KERNEL_PYRAMID_L1: the
yardstick; both times and their ratio are reported).  Warmed; per shape the median of REPS (default 11) calls and min-max.
One JSON line per shape and kernel.  Algorithmic bytes: rectify = raw read +
output written (2 B/pixel; TABLE + 8); pyramid = level 0 read + levels 1..3
written; its level-1 launch alone reads 1 and writes 1/4 B/pixel, so
rectification's bytes are 1.6 times the level-1 launch's.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIST = (-0.28, 0.09, 0.0006, -0.0004, -0.01)


def _median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def _timed(ctx, kernel, fn, reps):
    fn()  # warm-up: code objects, scratch growth
    fn()
    out = []
    for _ in range(reps):
        n0, ms0 = ctx.timing(kernel)
        fn()
        n1, ms1 = ctx.timing(kernel)
        out.append((ms1 - ms0) * 1e3)
    return out, n1 - n0


def main():
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "bench_rectify needs a GPU"
    import viso_amd
    from viso_amd import rectify as vr

    reps = int(os.environ.get("REPS", "11"))
    rng = np.random.default_rng(0)
    for (w, h, n) in ((1242, 375, 20), (1242, 375, 64), (1920, 1080, 1)):
        K = (0.58 * w, 0.58 * w, w / 2 - 0.5, h / 2 - 0.5)
        Kr = (0.6 * w, 0.6 * w, w / 2 + 3.2, h / 2 - 2.1)
        raw = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        ctx = viso_amd.Context(viso_amd.default_params(*K, width=w, height=h))
        ctx.timing_enable(True)
        px = w * h * n
        tab = vr.radtan_map(K, (w, h), Kr, DIST)
        runs = {
            "rectify_radtan": ("rectify", 2 * px,
                               lambda: ctx.rectify(raw, K, (w, h), counts=False, K_raw=Kr, dist=DIST)),
            "rectify_table": ("rectify", 2 * px + 8 * w * h,
                              lambda: ctx.rectify(raw, K, (w, h), counts=False, model=vr.TABLE, map=tab)),
            "pyramid": ("pyramid", sum(a * b for a, b in viso_amd.pyramid_dims(w, h)[0]) * n,
                        lambda: ctx.pyramid(raw)),
            # the yardstick: the pyramid's level-1 launch alone (reads 1, writes 1/4 B/pixel)
            "pyramid_level1": ("pyramid_l1", px + viso_amd.pyramid_dims(w, h)[0][1][0] *
                               viso_amd.pyramid_dims(w, h)[0][1][1] * n, lambda: ctx.pyramid(raw)),
        }
        res = {}
        for name, (kernel, nbytes, fn) in runs.items():
            ctx.timing_select([kernel])  # one pair of events per call: nothing else is bracketed
            us, launches = _timed(ctx, kernel, fn, reps)
            res[name] = _median(us)
            print(json.dumps({"bench": "rectify", "kernel": name, "width": w, "height": h, "images": n,
                              "reps": reps, "timed_regions_per_call": launches, "median_us": round(res[name], 2),
                              "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                              "algorithmic_bytes": nbytes,
                              "algorithmic_GBps": round(nbytes / (res[name] * 1e-6) / 1e9, 1)}), flush=True)
        print(json.dumps({"bench": "rectify", "width": w, "height": h, "images": n,
                          "radtan_over_level1": round(res["rectify_radtan"] / res["pyramid_level1"], 3),
                          "table_over_level1": round(res["rectify_table"] / res["pyramid_level1"], 3),
                          "bytes_over_level1": 1.6,
                          "radtan_over_pyramid": round(res["rectify_radtan"] / res["pyramid"], 3),
                          "table_over_radtan": round(res["rectify_table"] / res["rectify_radtan"], 3)}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
