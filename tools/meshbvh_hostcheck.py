"""Runs csrc/boxbound.h and csrc/tridist.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over
the adversarial (query, triangle, box) pairs of tests/meshbvh_cases.bound_pairs: writes the pairs to a temporary file, compiles
tools/meshbvh_hostcheck.cpp with -fsanitize=address,undefined -ffp-contract=off, runs it, and prints (``--out``: also appends)
the outcome.  CPU only: nothing is loaded into python and no device is touched.
    python tools/meshbvh_hostcheck.py [--cxx g++] [--out profiles/meshbvh_parity.txt]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshbvh_cases as BC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=shutil.which("g++") or shutil.which("clang++") or "c++")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pairs = BC.bound_pairs()
    rows = np.concatenate([np.concatenate([q, tri.reshape(len(q), 9), lo, hi], 1) for q, tri, lo, hi in pairs.values()]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "pairs.bin"), os.path.join(tmp, "meshbvh_hostcheck")
        with open(data, "wb") as f:
            f.write(np.int64(len(rows)).tobytes())
            f.write(np.ascontiguousarray(rows).tobytes())
        flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call([a.cxx] + flags + [os.path.join(ROOT, "tools", "meshbvh_hostcheck.cpp"), "-o", exe])
        run = subprocess.run([exe, data], capture_output=True, text=True)
    lines = [f"tools/meshbvh_hostcheck.py: boxbound.h + tridist.h, stand-alone host program, {os.path.basename(a.cxx)} "
             f"-fsanitize=address,undefined, {len(pairs)} groups of tests/meshbvh_cases.bound_pairs",
             run.stdout.strip(), f"exit code {run.returncode}; sanitizer reports: {'none' if not run.stderr.strip() else run.stderr.strip()}"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
