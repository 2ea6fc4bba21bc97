#!/usr/bin/env python3
"""Recorder of tests/golden/direct_partial_tree_parent.npz (GPU; run once).

Runs the inputs of tests/test_direct_partial_tree.py with the library named by
VISO_LIB -- the library built from the commit BEFORE four levels of the tile
tree moved into the loads -- and stores every result as uint64 bit patterns:
the 12 pose doubles of Context.direct_pose per key, and the poses of the
3-frame + 2-frame process_device run.  The test then holds the current library
to these bits.

    VISO_LIB=/path/to/parent/libviso_amd.so python tests/golden/make_direct_partial_tree.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("VISO_LIB"):
        sys.exit("set VISO_LIB to the parent commit's library")
    from tests import test_direct_partial_tree as tt
    from tests import test_direct_partials_layout as tl
    from viso_amd import _lib

    out = sys.argv[1] if len(sys.argv) > 1 else tt.GOLDEN
    cases = tt.make_cases()
    arrays = {}
    for key in tt.KEYS:
        pose = np.ascontiguousarray(tl.direct_pose(cases[key]), np.float64).reshape(12)
        assert np.isfinite(pose).all(), key
        arrays[key] = pose.view(np.uint64).copy()
    poses, _, _ = tl.two_frame_poses()
    assert np.isfinite(poses).all()
    arrays["two_frame"] = poses.view(np.uint64).copy()
    np.savez(out, **arrays)
    print(f"{len(arrays)} results of {_lib.load().viso_version().decode()} -> {out}")


if __name__ == "__main__":
    main()
