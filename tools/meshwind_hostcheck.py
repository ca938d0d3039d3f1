"""Runs csrc/solidangle.h and the two host entries' loops (csrc/meshwind_host.h) as a stand-alone host program under AddressSanitizer
and UndefinedBehaviorSanitizer: over the (point, triangle) groups tests/test_meshwind.py holds the term to, and the brute-force
cases of tests/meshwind_cases.py (the 4 096 copies and the permuted twins left out: they add time, not paths).  Writes the records
with the float64 restatement's answers to a temporary file, compiles tools/meshwind_hostcheck.cpp with -fsanitize=address,undefined
-ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into python and no device
is touched.
    python tools/meshwind_hostcheck.py [--cxx g++] [--out profiles/meshwind_parity.txt]"""
import io
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshwind_cases as WC  # noqa: E402
from tests import meshwind_restate as W  # noqa: E402

CASES = ("icosphere", "uv_sphere", "holed_icosphere", "sphere_square", "cube", "degenerate", "soup_257", "soup_1", "empty")


def main():
    groups = WC.term_pairs()
    q = np.concatenate([np.asarray(g[0], np.float32) for g in groups.values()])
    tri = np.concatenate([np.asarray(g[1], np.float32).reshape(-1, 9) for g in groups.values()])
    want = W.solid(q, tri[:, 0:3], tri[:, 3:6], tri[:, 6:9])
    f = io.BytesIO()
    f.write(np.int64(len(q)).tobytes())
    f.write(np.ascontiguousarray(np.concatenate([q, tri], 1), np.float32).tobytes())
    f.write(np.ascontiguousarray(want, np.float64).tobytes())
    f.write(np.int64(len(CASES)).tobytes())
    for key in CASES:
        c = WC.case(key)
        t9 = np.ascontiguousarray(np.stack(W.triangles(c["V"], c["F"]), 1).reshape(-1, 9), np.float32)
        f.write(np.int64(len(c["P"])).tobytes() + np.int64(len(t9)).tobytes())
        f.write(np.ascontiguousarray(c["P"], np.float32).tobytes() + t9.tobytes())
        f.write(np.ascontiguousarray(c["w"], np.float64).tobytes())
        f.write(np.ascontiguousarray(W.bar(c["n_valid"], c["mag"]), np.float64).tobytes())
    return hostcheck.run(__file__, "solidangle.h and the host entries' loops, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(groups)} groups of (point, triangle) pairs and {len(CASES)} brute-force cases", f.getvalue())


if __name__ == "__main__":
    sys.exit(main())
