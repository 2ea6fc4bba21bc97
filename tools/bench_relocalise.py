"""Cost and effect of the relocalisation (viso_set_relocalise, viso_kf_align;
DESIGN.md §19) at 1242 x 375 on the synthetic sequence: a stereo
initialisation at frame 0, then left images only.

* attempt: HIP events around one attempt's launches (viso:reloc: the
  candidates' launch and the choice) through the stage entry, at 2 candidates
  (keyframe 0, its own pose and an extra seed) and at 16 (frames 0..7 as
  keyframes at the renderer's poses), with max_points 256, 512 and 1,024;
  the current frame is frame 8, the extra seed frame 4's pose.  Median, min
  and max over --repeat attempts.
* tracking: host wall time per tracking frame and the direct chain's event
  time (viso:direct) over --frames frames, with the mode off, with the mode off
  but every frame finished inside its call (a point cull whose interval never
  comes), and with the mode on: the last two differ by the verdict's host
  synchronisation.
* occlusion: frames 5-7 replaced by another scene (tests/test_relocalise.py):
  per frame the status and the translation error against the renderer's
  truth, with the mode off and on.

Prints one JSON line (and writes it to --out).

    python tools/bench_relocalise.py [--frames 41] [--repeat 9] [--out FILE]
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
RELOC = (1, 57600.0, 500, 0, 10, 512)
NEVER_CULL = (100000, 3, 2.0, 50)


def truth(seq, f):
    a, b = seq.pose(f), seq.pose(0)
    R = a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T
    return np.concatenate([R.ravel(), a[9:] - R @ b[9:]])


def viso(seq, reloc=None, cull=None):
    import viso_amd
    v = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    if cull:
        v.set_point_cull(*cull)
    if reloc:
        v.set_relocalise(*reloc)
    v.process(seq.image(0), seq.image(0, 1))
    assert v.state == 1
    return v


def stat(ms):
    r4 = lambda x: round(float(x), 4)  # noqa: E731
    return {"median": r4(statistics.median(ms)), "min": r4(min(ms)), "max": r4(max(ms))}


def attempt_times(seq, points, repeat):
    from viso_amd import api
    ctx = api.Context(api.default_params(*seq.K, width=W, height=H))
    pyr = [ctx.pyramid(seq.image(f))[0] for f in range(9)]
    poses = [truth(seq, f) for f in range(8)]
    ctx.timing_enable(True)
    ctx.timing_select(["reloc"])
    out = {}
    for n_kf in (1, 8):
        for mp in (256, 512, 1024):
            ms, prev = [], ctx.timing("reloc")
            for _ in range(repeat + 1):
                r = ctx.kf_align(pyr[:n_kf], poses[:n_kf], pyr[8], W, H, points, truth(seq, 4), 10, mp, RELOC[1], 500)
                t = ctx.timing("reloc")
                assert t[0] == prev[0] + 1
                ms.append(t[1] - prev[1])
                prev = t
            row = stat(ms[1:])  # the first is the warm-up
            row.update(winner=r["winner"], statuses=[int(s) for s in r["report"][:, 0]],
                       steps_applied=int(np.nansum(r["report"][:, 5::4])))
            out[f"{2 * n_kf}_candidates_{mp}_points"] = row
    ctx.close()
    return out


def tracking_times(seq, images, reloc, cull):
    v = viso(seq, reloc, cull)
    v.ctx.timing_enable(True)
    v.ctx.timing_select(["direct"])
    v.synchronize()
    wall = []
    for img in images:
        t0 = time.perf_counter()
        v.OnNewFrame(img)
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    v.synchronize()
    tail = (time.perf_counter() - t0) * 1e3
    launches, ms = v.ctx.timing("direct")
    poses = v.poses
    v.close()
    return {"host_wall_ms_per_frame": stat(wall[2:]), "host_wall_ms_mean_with_final_sync":
            round((sum(wall) + tail) / len(wall), 4), "direct_event_ms_per_frame": round(ms / max(launches, 1), 4)}, poses


def occlusion(seq, reloc):
    from viso_amd.synth import Sequence
    other = Sequence(W, H, seed=7)
    v = viso(seq, reloc)
    for f in range(1, 14):
        v.OnNewFrame(other.image(40 + f) if f in (5, 6, 7) else seq.image(f))
    poses, status, info = v.poses, [int(s) for s in v.frame_status()], [int(x) for x in v.relocalise()]
    v.close()
    err = [round(float(np.linalg.norm(p[9:12] - truth(seq, f + 1)[9:12])), 5) for f, p in enumerate(poses)]
    return {"status": status, "translation_error": err, "info": info}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relocalise_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(W, H, seed=0)
    v = viso(seq)
    points = v.GetPoints()
    v.close()
    images = [seq.image(f) for f in range(1, a.frames)]
    tracking_times(seq, images[:8], RELOC, None)  # warm-up
    t_off, p_off = tracking_times(seq, images, None, None)
    t_one, p_one = tracking_times(seq, images, None, NEVER_CULL)
    t_on, p_on = tracking_times(seq, images, RELOC, None)
    out = {
        "bench": "relocalise", "size": [W, H], "map_points": len(points), "relocalise": list(RELOC),
        "attempt_event_ms": attempt_times(seq, points, a.repeat),
        "tracking_frames": len(images),
        "tracking_off": t_off, "tracking_off_frames_finished_one_by_one": t_one, "tracking_on": t_on,
        "poses_equal_off_on": bool(np.array_equal(p_off, p_on) and np.array_equal(p_off, p_one)),
        "occlusion_off": occlusion(seq, None), "occlusion_on": occlusion(seq, RELOC),
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash(),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
