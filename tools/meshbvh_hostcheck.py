"""Runs csrc/boxbound.h and csrc/tridist.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over
the adversarial (query, triangle, box) pairs of tests/meshbvh_cases.bound_pairs: writes the pairs to a temporary file, compiles
tools/meshbvh_hostcheck.cpp with -fsanitize=address,undefined -ffp-contract=off, runs it, and prints (``--out``: also appends)
the outcome.  CPU only: nothing is loaded into python and no device is touched.
    python tools/meshbvh_hostcheck.py [--cxx g++] [--out profiles/meshbvh_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshbvh_cases as BC  # noqa: E402


def main():
    pairs = BC.bound_pairs()
    rows = np.concatenate([np.concatenate([q, tri.reshape(len(q), 9), lo, hi], 1) for q, tri, lo, hi in pairs.values()]).astype(np.float32)
    return hostcheck.run(__file__, "boxbound.h + tridist.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(pairs)} groups of tests/meshbvh_cases.bound_pairs",
                         np.int64(len(rows)).tobytes() + np.ascontiguousarray(rows).tobytes())


if __name__ == "__main__":
    sys.exit(main())
