"""Runs csrc/splatdensify_ops.h -- the per-row functions and the host entries' loops -- as a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer, over the cases of tests/splatdensify_cases.py (every size, SH degree, children per
split and kind of round, the rows on a limit, every accumulation): writes each case's arrays, the plan and the numpy restatement's
answers to a temporary file, compiles tools/splatdensify_hostcheck.cpp with -fsanitize=address,undefined -ffp-contract=off, runs it,
and prints (``--out``: also appends) the outcome.  CPU only: nothing is loaded into python's process but numpy, and no device is
touched.
    python tools/splatdensify_hostcheck.py [--cxx g++] [--out profiles/splatdensify_parity.txt]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import splatdensify_cases as C  # noqa: E402
from tests import splatdensify_restate as S  # noqa: E402


def _blob(parts):
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def _records():
    for P, V in C.accumulate_cases():
        arrays = C.accumulate_case(P, V, seed=P + V)
        yield _blob([np.array([0, V, P, 0, 0, 0], np.int64), *arrays, *S.accumulate(*arrays)])
    for P, degree, n, kind in C.round_cases():
        case = C.round_case(P, degree, n, kind, seed=P + degree + n)
        stats = [case[k] for k in ("grad_sum", "seen", "max_radius")]
        action, offset, counts = S.decide(case["plan"], case["params"]["opacity"], case["params"]["scales"], *stats)
        p, m, v, source, child, _ = S.apply(case["plan"], case["params"], case["exp_avg"], case["exp_avg_sq"], action, offset, counts, case["noise"])
        blobs = [np.array([1, degree, P, counts[4], counts[0] + counts[1], 0], np.int64), case["plan"]]
        blobs += [case[g][k] for g in ("params", "exp_avg", "exp_avg_sq") for k in C.FIELDS]
        blobs += stats + [case["noise"], action, offset, counts, source, child]
        blobs += [d[k] for d in (p, m, v) for k in C.FIELDS]
        yield _blob(blobs)


def main():
    records = list(_records())
    return hostcheck.run(__file__, "splatdensify_ops.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(records)} cases of tests/splatdensify_cases.py", np.int64(len(records)).tobytes() + b"".join(records))


if __name__ == "__main__":
    sys.exit(main())
