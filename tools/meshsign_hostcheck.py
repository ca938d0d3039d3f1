"""Runs csrc/raycross.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over the (ray, triangle)
groups of tests/meshray_cases.bound_groups and the crafted rays that meet a corner or an edge of the dyadic cube
(tests/meshsign_cases.touching_points, every such ray against every triangle of the cube): writes the records with the float64
restatement's answers to a temporary file, compiles tools/meshsign_hostcheck.cpp with -fsanitize=address,undefined
-ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into python and no device
is touched.
    python tools/meshsign_hostcheck.py [--cxx g++] [--out profiles/meshsign_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshray_cases as MC  # noqa: E402
from tests import meshray_restate as RR  # noqa: E402
from tests import meshsign_cases as SC  # noqa: E402
from tests import meshsign_restate as S  # noqa: E402


def _records(o, d, tri):
    hit, orient, touch = S.cross(RR.setup(o, d), tri[:, 0], tri[:, 1], tri[:, 2])
    return np.concatenate([o, d, tri.reshape(len(o), 9), hit[:, None], orient[:, None], touch[:, None]], 1).astype(np.float32)


def main():
    groups = MC.bound_groups()
    rows = [_records(o, d, tri) for o, d, _, _, tri, _, _ in groups.values()]
    V, F = SC.cube()
    tri = V[F]
    crafted = 0
    for k, P in SC.touching_points():
        o = np.repeat(P, len(tri), 0)
        rows.append(_records(o, np.broadcast_to(S.DIRECTIONS[k], o.shape).astype(np.float32), np.tile(tri, (len(P), 1, 1))))
        crafted += len(P)
    rows = np.concatenate(rows)
    return hostcheck.run(__file__, "raycross.h on raytri.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(groups)} groups of tests/meshray_cases.bound_groups and {crafted} crafted rays x {len(tri)} triangles of the cube",
                         np.int64(len(rows)).tobytes() + np.ascontiguousarray(rows).tobytes())


if __name__ == "__main__":
    sys.exit(main())
