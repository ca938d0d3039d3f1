"""Runs csrc/raytri.h and csrc/raybox.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over
the adversarial (ray, triangle, box) groups of tests/meshray_cases.bound_groups: writes the groups to a temporary file, compiles
tools/meshray_hostcheck.cpp with -fsanitize=address,undefined -ffp-contract=off, runs it, and prints (``--out``: also appends)
the outcome.  CPU only: nothing is loaded into python and no device is touched.
    python tools/meshray_hostcheck.py [--cxx g++] [--out profiles/meshray_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshray_cases as MC  # noqa: E402


def main():
    groups = MC.bound_groups()
    rows = np.concatenate([np.concatenate([o, d, lo_t[:, None], hi_t[:, None], tri.reshape(len(o), 9), lo, hi], 1)
                           for o, d, lo_t, hi_t, tri, lo, hi in groups.values()]).astype(np.float32)
    return hostcheck.run(__file__, "raytri.h + raybox.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(groups)} groups of tests/meshray_cases.bound_groups",
                         np.int64(len(rows)).tobytes() + np.ascontiguousarray(rows).tobytes())


if __name__ == "__main__":
    sys.exit(main())
