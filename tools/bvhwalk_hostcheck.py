"""Runs the walk of csrc/bvhwalk.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over the
layouts mb_layout(T) gives at T = 1, around every T at which the number of levels changes, and at a T whose last sibling group is
partly padding on two levels at once, under each of the eight sibling masks (tools/bvhwalk_hostcheck.cpp says what is held).  The
header that holds the layout is HIP source, so the compiler is hipcc, for the host alone (--cuda-host-only): compiles the program
with -fsanitize=address,undefined, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into
python and no device is touched.
    python tools/bvhwalk_hostcheck.py [--hipcc /opt/rocm/bin/hipcc] [--out profiles/bvhwalk_parity.txt]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hipcc", default=shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bvhwalk_hostcheck")
        flags = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all", "-Wno-unused-function"]
        subprocess.check_call([a.hipcc] + flags + [os.path.join(ROOT, "tools", "bvhwalk_hostcheck.cpp"), "-o", exe])
        run = subprocess.run([exe], capture_output=True, text=True)
    rows = run.stdout.strip().splitlines()
    lines = [f"tools/bvhwalk_hostcheck.py: lara_bvhwalk of bvhwalk.h over mb_layout(T), stand-alone host program, "
             f"{os.path.basename(a.hipcc)} --cuda-host-only -fsanitize=address,undefined"] + rows[-1:] + \
            [f"exit code {run.returncode}; sanitizer reports: {'none' if not run.stderr.strip() else run.stderr.strip()}"]
    print("\n".join(rows[:-1] + lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return run.returncode


if __name__ == "__main__":
    sys.exit(main())
