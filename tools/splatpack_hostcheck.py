"""Runs csrc/splatpack_ops.h -- the per-row functions and the host entries' loops -- as a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer, over the cases of tests/splatpack_cases.py (every size, SH degree and kind of cloud):
writes each case's arrays, the plan and the numpy restatement's answers to a temporary file, compiles tools/splatpack_hostcheck.cpp
with -fsanitize=address,undefined -ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is
loaded into python's process but numpy, and no device is touched.
    python tools/splatpack_hostcheck.py [--cxx g++] [--out profiles/splatpack_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import splatpack_cases as C  # noqa: E402
from tests import splatpack_restate as S  # noqa: E402


def _blob(parts):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def _records():
    for P, degree, kind in C.cases():
        k = C.case(P, degree, kind)
        near = C.near_boundary(k["alpha_pre"]).astype(np.uint8) | (C.near_fp32_boundary(k["importance_pre"]).astype(np.uint8) << 1)
        parts = [np.array([degree, P, k["order"].shape[0], 0, 0, 0], np.int64), k["plan"]] + [k["cloud"][f] for f in C.FIELDS]
        parts += [near, k["valid"], k["box"], np.array([k["dropped"]], np.int64), k["morton_keys"], k["importance_keys"], k["order"],
                  k["chunks"], k["words"], k["sh"], k["splat_order"], k["splat"]]
        parts += [S.f32(k["decoded"][f]) for f in C.FIELDS] + [S.f32(k["splat_decoded"][f]) for f in C.FIELDS]
        yield _blob(parts)


def main():
    records = list(_records())
    return hostcheck.run(__file__, "splatpack_ops.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(records)} cases of tests/splatpack_cases.py", np.int64(len(records)).tobytes() + b"".join(records))


if __name__ == "__main__":
    sys.exit(main())
