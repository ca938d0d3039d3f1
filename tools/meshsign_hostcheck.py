"""Runs csrc/raycross.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over the (ray, triangle)
groups of tests/meshray_cases.bound_groups and the crafted rays that meet a corner or an edge of the dyadic cube
(tests/meshsign_cases.touching_points, every such ray against every triangle of the cube): writes the records with the float64
restatement's answers to a temporary file, compiles tools/meshsign_hostcheck.cpp with -fsanitize=address,undefined
-ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into python and no device
is touched.
    python tools/meshsign_hostcheck.py [--cxx g++] [--out profiles/meshsign_parity.txt]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=shutil.which("g++") or shutil.which("clang++") or "c++")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "records.bin"), os.path.join(tmp, "meshsign_hostcheck")
        with open(data, "wb") as f:
            f.write(np.int64(len(rows)).tobytes())
            f.write(np.ascontiguousarray(rows).tobytes())
        flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call([a.cxx] + flags + [os.path.join(ROOT, "tools", "meshsign_hostcheck.cpp"), "-o", exe])
        run = subprocess.run([exe, data], capture_output=True, text=True)
    lines = [f"tools/meshsign_hostcheck.py: raycross.h on raytri.h, stand-alone host program, {os.path.basename(a.cxx)} "
             f"-fsanitize=address,undefined, {len(groups)} groups of tests/meshray_cases.bound_groups and {crafted} crafted rays x "
             f"{len(tri)} triangles of the cube",
             run.stdout.strip(), f"exit code {run.returncode}; sanitizer reports: {'none' if not run.stderr.strip() else run.stderr.strip()}"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
