"""Cost of one relocalisation attempt in its two forms (viso_kf_align and
viso_kf_align_illum) at 1242 x 375 on the synthetic
sequence, on the same inputs: the current frame is frame 8 mapped to
0.6 I + 30 (rounded, clipped), the extra seed frame 4's pose; 2 candidates
(keyframe 0) and 16 (frames 0..7 as keyframes at the renderer's poses) at
max_points 256, 512 and 1,024.

HIP events around both launches of an attempt (viso:reloc: the candidates'
launch and the choice) through the stage entries; median, min and max over
--repeat attempts behind one warm-up.  Per row and form also the winner, the
statuses and the steps applied over all candidates and levels: the two forms do
not iterate alike on a frame whose exposure changed.

Prints one JSON line (and writes it to --out).

    python tools/bench_reloc_illum.py [--repeat 9] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_relocalise import H, RELOC, W, stat, truth, viso  # noqa: E402

GAIN, OFFSET, MAX_GAIN = 0.6, 30.0, 4.0


def mapped(img):
    return np.clip(np.rint(GAIN * img.astype(np.float64) + OFFSET), 0, 255).astype(np.uint8)


def attempt_times(seq, points, repeat):
    from viso_amd import api
    ctx = api.Context(api.default_params(*seq.K, width=W, height=H))
    pyr = [ctx.pyramid(seq.image(f))[0] for f in range(8)]
    cur = ctx.pyramid(mapped(seq.image(8)))[0]
    poses = [truth(seq, f) for f in range(8)]
    ctx.timing_enable(True)
    ctx.timing_select(["reloc"])
    forms = {"plain": lambda *a: ctx.kf_align(*a), "illum": lambda *a: ctx.kf_align_illum(*a, MAX_GAIN)}
    out = {}
    for n_kf in (1, 8):
        for mp in (256, 512, 1024):
            row = {}
            for name, fn in forms.items():
                ms, prev = [], ctx.timing("reloc")
                for _ in range(repeat + 1):
                    r = fn(pyr[:n_kf], poses[:n_kf], cur, W, H, points, truth(seq, 4), 10, mp, RELOC[1], 500)
                    t = ctx.timing("reloc")
                    assert t[0] == prev[0] + 1
                    ms.append(t[1] - prev[1])
                    prev = t
                row[name] = stat(ms[1:])  # the first is the warm-up
                row[name].update(winner=r["winner"], statuses=[int(s) for s in r["report"][:, 0]],
                                 steps_applied=int(np.nansum(r["report"][:, 5::4])))
                if name == "illum" and r["winner"] >= 0:
                    row[name]["winner_gain_offset"] = [round(float(x), 4) for x in r["gain_offset"][r["winner"]]]
            row["ratio_of_medians"] = round(row["illum"]["median"] / row["plain"]["median"], 3)
            out[f"{2 * n_kf}_candidates_{mp}_points"] = row
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_illum_cost.json"))
    a = ap.parse_args()
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(W, H, seed=0)
    v = viso(seq)
    points = v.GetPoints()
    v.close()
    out = {"bench": "reloc_illum", "size": [W, H], "map_points": len(points), "current": "frame 8 as 0.6 I + 30",
           "max_gain": MAX_GAIN, "attempt_event_ms": attempt_times(seq, points, a.repeat),
           "device": torch.cuda.get_device_name(0), "source_hash": _lib.built_hash()}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
