"""Cost and effect of the relocalisation seed (viso_set_reloc_seed,
viso_reloc_seed) at 1242 x 375 on the synthetic sequence: a
stereo initialisation at frame 0, then left images only.

* stage: HIP events around the stage's launches through the stage entry
  (viso:reloc_seed: everything behind FAST; viso:fast beside it) at the
  renderer's map with the default parameters, and around one keyframe-alignment
  attempt (viso:reloc, 2 candidates, 512 points) on the same frame.  The
  current frame is frame 12, the start pose frame 4's.  Median, min and max
  over --repeat runs.
* occlusion: frames 5-11 replaced by another scene (tests/test_reloc_seed.py):
  per frame the status and the translation error against the renderer's truth,
  with the seed off and on, and the two info vectors.
* bench: with --parent-lib, `bench.py --gpus 1 --steps 20 --warmup 5` by that
  library (VISO_LIB) and by this one, --pairs times interleaved, every
  frames/s; and one --dump-outputs of each, compared byte for byte (the mode
  is off there).

Prints one JSON line (and appends it to --out).

    python tools/bench_reloc_seed.py [--repeat 9] [--parent-lib SO --pairs 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1242, 375
RELOC = (1, 57600.0, 500, 0, 10, 512)
GAP = 12  # the first real frame after the occlusion


def truth(seq, f):
    a, b = seq.pose(f), seq.pose(0)
    R = a[:9].reshape(3, 3) @ b[:9].reshape(3, 3).T
    return np.concatenate([R.ravel(), a[9:] - R @ b[9:]])


def viso(seq, seed_on):
    import viso_amd
    v = viso_amd.Viso(*seq.K, width=W, height=H, enable_tracking=1, batch_frames=32)
    v.set_stereo(seq.p.baseline, 128, 1)
    v.set_relocalise(*RELOC)
    if seed_on:
        v.set_reloc_seed()
    v.process(seq.image(0), seq.image(0, 1))
    assert v.state == 1
    return v


def stat(ms):
    r4 = lambda x: round(float(x), 4)  # noqa: E731
    return {"median": r4(statistics.median(ms)), "min": r4(min(ms)), "max": r4(max(ms))}


def stage_times(seq, points, repeat):
    from viso_amd import api
    ctx = api.Context(api.default_params(*seq.K, width=W, height=H))
    kf, cur = ctx.pyramid(seq.image(0))[0], ctx.pyramid(seq.image(GAP))[0]
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float64)
    hosts = np.zeros(len(points), np.int32)
    ctx.timing_enable(True)
    ctx.timing_select(["reloc_seed", "fast", "reloc"])
    rows = {"reloc_seed": [], "fast": [], "reloc": []}
    prev = {k: ctx.timing(k) for k in rows}
    for _ in range(repeat + 1):
        r = ctx.reloc_seed([kf], [ident], cur, W, H, points, hosts, truth(seq, 4))
        a = ctx.kf_align([kf], [ident], cur, W, H, points, r["pose"], *RELOC[4:], RELOC[1], RELOC[2])
        for k in rows:
            t = ctx.timing(k)
            assert t[0] == prev[k][0] + 1, k
            rows[k].append(t[1] - prev[k][1])
            prev[k] = t
    ctx.close()
    out = {k + "_event_ms": stat(v[1:]) for k, v in rows.items()}  # the first is the warm-up
    out.update(report=[float(x) for x in np.nan_to_num(r["report"], nan=-1.0)],
               seed_translation_error=round(float(np.linalg.norm(r["pose"][9:] - truth(seq, GAP)[9:])), 5),
               attempt_winner=int(a["winner"]), attempt_statuses=[int(s) for s in a["report"][:, 0]])
    return out


def occlusion(seq, seed_on):
    from viso_amd.synth import Sequence
    other = Sequence(W, H, seed=7)
    v = viso(seq, seed_on)
    for f in range(1, GAP + 4):
        v.OnNewFrame(other.image(40 + f) if 5 <= f < GAP else seq.image(f))
    poses, status = v.poses, [int(s) for s in v.frame_status()]
    info, sinfo = [int(x) for x in v.relocalise()], [int(x) for x in v.reloc_seed()]
    v.close()
    err = [round(float(np.linalg.norm(p[9:12] - truth(seq, f + 1)[9:12])), 5) for f, p in enumerate(poses)]
    return {"status": status, "translation_error": err, "info": info, "seed_info": sinfo}


def bench_ab(parent_lib, pairs):
    """bench.py's lines by the parent's library and this one, interleaved."""
    args = [sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]

    def run(lib, extra=()):
        env = dict(os.environ)
        if lib:
            env["VISO_LIB"] = lib
        else:
            env.pop("VISO_LIB", None)
        r = subprocess.run([*args, *extra], env=env, capture_output=True, text=True, timeout=300, check=True)
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    fps = {"parent": [], "this": []}
    for _ in range(pairs):
        for name, lib in (("parent", parent_lib), ("this", "")):
            line = run(lib)
            fps[name].append(round(float(line.get("value", line.get("frames_per_s", 0.0))), 1))
    with tempfile.TemporaryDirectory() as d:
        dirs = {}
        for name, lib in (("parent", parent_lib), ("this", "")):
            dirs[name] = os.path.join(d, name)
            run(lib, ("--dump-outputs", dirs[name]))
        names = sorted(os.listdir(dirs["parent"]))
        equal = names == sorted(os.listdir(dirs["this"])) and all(
            open(os.path.join(dirs["parent"], n), "rb").read() == open(os.path.join(dirs["this"], n), "rb").read()
            for n in names)
    return {"frames_per_s": fps, "dump_outputs_byte_equal": bool(equal), "dumped": names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_seed_bench_ab.jsonl"))
    a = ap.parse_args()
    out = {"bench": "reloc_seed", "size": [W, H], "relocalise": list(RELOC)}
    if a.parent_lib:  # first: no context of this process is alive beside the child's
        out["bench_py"] = bench_ab(os.path.abspath(a.parent_lib), a.pairs)
    import torch

    from viso_amd import _lib
    from viso_amd.synth import Sequence
    seq = Sequence(W, H, seed=0)
    v = viso(seq, False)
    points = v.GetPoints()
    v.close()
    out.update(map_points=len(points), stage=stage_times(seq, points, a.repeat),
               occlusion_off=occlusion(seq, False), occlusion_on=occlusion(seq, True),
               device=torch.cuda.get_device_name(0), source_hash=_lib.built_hash())
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
