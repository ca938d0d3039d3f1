"""Runs csrc/meshtopo_ops.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over every mesh of
tests/meshtopo_cases.py (the permuted ones included): writes each case's arrays and the float64 restatement's answers -- the normals
for both weightings with their zero counts, one smoothing pass with lam and with mu, with and without the boundary held -- to a
temporary file, compiles tools/meshtopo_hostcheck.cpp with -fsanitize=address,undefined -ffp-contract=off, runs it, and prints
(``--out``: also appends) the outcome.  CPU only: nothing is loaded into python and no device is touched.
    python tools/meshtopo_hostcheck.py [--cxx g++] [--out profiles/meshtopo_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshtopo_cases as C  # noqa: E402
from tests import meshtopo_restate as S  # noqa: E402

LAM, MU = 0.5, -0.53


def _record(key):
    c = C.case(key)
    V, F, topo = c["V"], c["F"], c["topo"]
    (no, nb), (fo, fc) = c["vv"], c["vf"]
    fixed = topo.boundary_vertices()
    parts = [np.array([len(V), len(F), len(nb), len(fc)], np.int64), V.astype(np.float32), F.astype(np.int32), no.astype(np.int64),
             nb.astype(np.int32), fo.astype(np.int64), fc.astype(np.int32), fixed.astype(np.int32),
             c["normals"][S.AREA][0], c["normals"][S.UNIFORM][0],
             np.array([c["normals"][S.AREA][1], c["normals"][S.UNIFORM][1]], np.int64), np.array([LAM, MU], np.float64)]
    for hold in (None, fixed):
        for s in (LAM, MU):
            parts.append(S.smooth_pass(V, no, nb, s, hold))
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def main():
    return hostcheck.run(__file__, "meshtopo_ops.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"the {len(C.CASES)} cases of tests/meshtopo_cases.py",
                         np.int64(len(C.CASES)).tobytes() + b"".join(_record(key) for key in C.CASES))


if __name__ == "__main__":
    sys.exit(main())
