"""Runs csrc/solidangle.h and the two host entries' loops (csrc/meshwind_host.h) as a stand-alone host program under AddressSanitizer
and UndefinedBehaviorSanitizer: over the (point, triangle) groups tests/test_meshwind.py holds the term to, and the brute-force
cases of tests/meshwind_cases.py (the 4 096 copies and the permuted twins left out: they add time, not paths).  Writes the records
with the float64 restatement's answers to a temporary file, compiles tools/meshwind_hostcheck.cpp with -fsanitize=address,undefined
-ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into python and no device
is touched.
    python tools/meshwind_hostcheck.py [--cxx g++] [--out profiles/meshwind_parity.txt]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshwind_cases as WC  # noqa: E402
from tests import meshwind_restate as W  # noqa: E402

CASES = ("icosphere", "uv_sphere", "holed_icosphere", "sphere_square", "cube", "degenerate", "soup_257", "soup_1", "empty")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=shutil.which("g++") or shutil.which("clang++") or "c++")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    groups = WC.term_pairs()
    q = np.concatenate([np.asarray(g[0], np.float32) for g in groups.values()])
    tri = np.concatenate([np.asarray(g[1], np.float32).reshape(-1, 9) for g in groups.values()])
    want = W.solid(q, tri[:, 0:3], tri[:, 3:6], tri[:, 6:9])
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "records.bin"), os.path.join(tmp, "meshwind_hostcheck")
        with open(data, "wb") as f:
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
        flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call([a.cxx] + flags + [os.path.join(ROOT, "tools", "meshwind_hostcheck.cpp"), "-o", exe])
        run = subprocess.run([exe, data], capture_output=True, text=True)
    lines = [f"tools/meshwind_hostcheck.py: solidangle.h and the host entries' loops, stand-alone host program, {os.path.basename(a.cxx)} "
             f"-fsanitize=address,undefined, {len(groups)} groups of (point, triangle) pairs and {len(CASES)} brute-force cases",
             run.stdout.strip(), f"exit code {run.returncode}; sanitizer reports: {'none' if not run.stderr.strip() else run.stderr.strip()}"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
