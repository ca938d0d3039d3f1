"""Runs csrc/raytri.h and csrc/raybox.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over
the adversarial (ray, triangle, box) groups of tests/meshray_cases.bound_groups: writes the groups to a temporary file, compiles
tools/meshray_hostcheck.cpp with -fsanitize=address,undefined -ffp-contract=off, runs it, and prints (``--out``: also appends)
the outcome.  CPU only: nothing is loaded into python and no device is touched.
    python tools/meshray_hostcheck.py [--cxx g++] [--out profiles/meshray_parity.txt]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=shutil.which("g++") or shutil.which("clang++") or "c++")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    groups = MC.bound_groups()
    rows = np.concatenate([np.concatenate([o, d, lo_t[:, None], hi_t[:, None], tri.reshape(len(o), 9), lo, hi], 1)
                           for o, d, lo_t, hi_t, tri, lo, hi in groups.values()]).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "groups.bin"), os.path.join(tmp, "meshray_hostcheck")
        with open(data, "wb") as f:
            f.write(np.int64(len(rows)).tobytes())
            f.write(np.ascontiguousarray(rows).tobytes())
        flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        subprocess.check_call([a.cxx] + flags + [os.path.join(ROOT, "tools", "meshray_hostcheck.cpp"), "-o", exe])
        run = subprocess.run([exe, data], capture_output=True, text=True)
    lines = [f"tools/meshray_hostcheck.py: raytri.h + raybox.h, stand-alone host program, {os.path.basename(a.cxx)} "
             f"-fsanitize=address,undefined, {len(groups)} groups of tests/meshray_cases.bound_groups",
             run.stdout.strip(), f"exit code {run.returncode}; sanitizer reports: {'none' if not run.stderr.strip() else run.stderr.strip()}"]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
