#!/usr/bin/env python3
"""Recorder of tests/golden/map_compaction_parent.txt (GPU; run once).

Runs the cases of tests/test_map_compaction.py with the library named by
VISO_LIB -- the library built from the commit BEFORE the compaction kernels
moved to block_rank.hpp -- and stores one SHA-256 per case over every output
array.  The test then holds the current library to these digests.

    VISO_LIB=/path/to/parent/libviso_amd.so python tests/golden/make_map_compaction.py [out.txt]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    if not os.environ.get("VISO_LIB"):
        sys.exit("set VISO_LIB to the parent commit's library")
    from tests import test_map_compaction as tc
    from viso_amd import _lib

    out = sys.argv[1] if len(sys.argv) > 1 else tc.GOLDEN
    lines = []
    for case in sorted(tc.CASES):
        lines.append(f"{case} {tc.digest(tc.CASES[case]())}\n")
        print(lines[-1], end="", flush=True)
    with open(out, "w") as f:
        f.writelines(lines)
    print(f"{len(lines)} cases of {_lib.load().viso_version().decode()} -> {out}")


if __name__ == "__main__":
    main()
