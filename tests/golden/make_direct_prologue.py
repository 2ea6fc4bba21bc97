#!/usr/bin/env python3
"""Recorder of tests/golden/direct_prologue_parent.npz (GPU; run once).

Runs Context.direct_pose on the keys of tests/test_direct_prologue.py with the
library named by VISO_LIB -- the library built from the commit BEFORE the
lane-placed solver quotients -- and stores the 12 pose doubles of every key
and precision as uint64 bit patterns.  The test then holds the current library
to these bits.

    VISO_LIB=/path/to/parent/libviso_amd.so python tests/golden/make_direct_prologue.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("VISO_LIB"):
        sys.exit("set VISO_LIB to the parent commit's library")
    from tests import test_direct_prologue as tp
    from viso_amd import _lib

    out = sys.argv[1] if len(sys.argv) > 1 else tp.GOLDEN
    arrays = {}
    for key, fast in tp._parent_params():
        pose = np.ascontiguousarray(tp._direct_pose(key, fast), np.float64).reshape(12)
        assert np.isfinite(pose).all(), (key, fast)
        arrays[tp.golden_name(key, fast)] = pose.view(np.uint64).copy()
    np.savez(out, **arrays)
    print(f"{len(arrays)} poses of {_lib.load().viso_version().decode()} -> {out}")


if __name__ == "__main__":
    main()
