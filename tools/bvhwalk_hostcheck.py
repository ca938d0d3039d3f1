"""Runs the walk of csrc/bvhwalk.h as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over the
layouts mb_layout(T) gives at T = 1, around every T at which the number of levels changes, and at a T whose last sibling group is
partly padding on two levels at once, under each of the eight sibling masks (tools/bvhwalk_hostcheck.cpp says what is held).  The
header that holds the layout is HIP source, so the compiler is hipcc, for the host alone (--cuda-host-only): compiles the program
with -fsanitize=address,undefined, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into
python and no device is touched.
    python tools/bvhwalk_hostcheck.py [--hipcc /opt/rocm/bin/hipcc] [--out profiles/bvhwalk_parity.txt]"""
import sys

import hostcheck


def main():
    return hostcheck.run(__file__, "lara_bvhwalk of bvhwalk.h over mb_layout(T), stand-alone host program, "
                         "{cxx} --cuda-host-only -fsanitize=address,undefined", compiler="hipcc",
                         flags=["-x", "hip", "--cuda-host-only", "-Wno-unused-function"], rows_first=True)


if __name__ == "__main__":
    sys.exit(main())
