"""Runs csrc/splatxform_ops.h -- the per-surfel function and the host entry's loop -- as a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer, over the clouds of tests/splatxform_cases.py (every SH degree, every size, the row
offsets, the special rows) under the three transforms of the cases: writes each case's arrays, the plan and the float64
restatement's answers to a temporary file, compiles tools/splatxform_hostcheck.cpp with -fsanitize=address,undefined
-ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into python's process
but numpy, and no device is touched.
    python tools/splatxform_hostcheck.py [--cxx g++] [--out profiles/splatxform_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import splatxform_cases as C  # noqa: E402
from tests import splatxform_restate as S  # noqa: E402


def _plan(T):
    """The plan from the restatement's own parts (the module is not imported): the fitted blocks, the quaternion by the trace."""
    R, s, t, A = S.split(T)
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    assert w > 0.25, "the cases' rotations are well below half a turn"
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    D = S.fit_blocks(R)
    return np.concatenate([A.ravel(), t, q / np.linalg.norm(q), [np.log(s)], D[0].ravel(), D[1].ravel(), D[2].ravel()]).astype(np.float64)


def _records():
    n = 0
    for name in sorted(C.TRANSFORMS):
        plan = _plan(C.TRANSFORMS[name])
        for degree in C.DEGREES:
            for P in C.SIZES:
                c = C.cloud(P, degree, seed=P + degree)
                want = S.apply(plan, c)
                for row0 in C.ROW_OFFSETS if name == "similarity" else (0,):
                    parts = [np.array([degree, P, row0, row0 + P + 7], np.int64), plan] + [c[k] for k in C.FIELDS] + [want[k] for k in C.FIELDS]
                    n += 1
                    yield b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def main():
    records = list(_records())
    return hostcheck.run(__file__, "splatxform_ops.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(records)} cases of tests/splatxform_cases.py", np.int64(len(records)).tobytes() + b"".join(records))


if __name__ == "__main__":
    sys.exit(main())
