"""Runs csrc/splatadam_ops.h -- the per-word function and the host entry's loop -- as a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer, over the cases of tests/splatrefine_cases.py (every size, SH degree, step, zero and
non-zero moments, dense and masked; the masked ones also zero the gradients): writes each case's arrays, the plan and the float64
restatement's answers to a temporary file, compiles tools/splatadam_hostcheck.cpp with -fsanitize=address,undefined
-ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into python's process but
numpy, and no device is touched.
    python tools/splatadam_hostcheck.py [--cxx g++] [--out profiles/splatrefine_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import splatrefine_cases as C  # noqa: E402
from tests import splatrefine_restate as S  # noqa: E402


def _records():
    for P, degree, t, moments, sparse in C.all_cases():
        parts = C.case(P, degree, moments, seed=P + degree)
        row = S.plan(t, C.LRS)
        visible = C.mask(P, seed=degree) if sparse else None
        *want, skipped = S.step(row, *parts, visible=visible, zero_grads=sparse)
        blobs = [np.array([degree, P, int(sparse), int(sparse), skipped], np.int64), row]
        blobs += [d[k] for d in parts for k in C.FIELDS]
        if sparse:
            blobs.append(visible)
        blobs += [d[k] for d in want for k in C.FIELDS]
        yield b"".join(np.ascontiguousarray(b).tobytes() for b in blobs)


def main():
    records = list(_records())
    return hostcheck.run(__file__, "splatadam_ops.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(records)} cases of tests/splatrefine_cases.py", np.int64(len(records)).tobytes() + b"".join(records))


if __name__ == "__main__":
    sys.exit(main())
