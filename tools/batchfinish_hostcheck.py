"""Runs csrc/batchfinish_ops.h -- the per-pixel function and the host entry's loop -- as a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer, over the raw batches of tests/batchfinish_cases.py (every shape, with normals and in
the rgb-only form) and the exhaustive (colour, alpha) plane: writes each case's arrays and the numpy float32 restatement's answers to
a temporary file, compiles tools/batchfinish_hostcheck.cpp with -fsanitize=address,undefined -ffp-contract=off, runs it, and prints
(``--out``: also appends) the outcome.  CPU only: nothing is loaded into python's process but numpy, and no device is touched.
    python tools/batchfinish_hostcheck.py [--cxx g++] [--out FILE]"""
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import batchfinish_cases as C  # noqa: E402
from tests import batchfinish_restate as S  # noqa: E402


def _record(rgba, bg, n_u8, rot):
    B, V, H, W = rgba.shape[:4]
    rgb, msk = S.colour(rgba, bg)
    parts = [np.array([B, V, H, W, n_u8 is not None], np.int64), rgba, bg]
    parts += [n_u8, rot] if n_u8 is not None else []
    parts += [rgb, msk] + ([S.normals(n_u8, rot)] if n_u8 is not None else [])
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def _records():
    for i, shape in enumerate(C.SHAPES):
        b = C.batch(shape, seed=i)
        yield _record(b["rgba"], b["bg"], b["n_u8"], b["rot"])
        yield _record(b["rgba"], b["bg"], None, None)
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    plane = np.stack([c, c[::-1], c.T, a], axis=-1)[None, None]
    for bg in (0.0, 0.5, 1.0, 0.2, 250.0, -0.0):
        yield _record(plane, np.full((1, 1, 3), bg, np.float32), np.ascontiguousarray(plane[..., :3]), np.eye(3, dtype=np.float32)[None] * np.float32(bg + 1))


def main():
    records = list(_records())
    return hostcheck.run(__file__, "batchfinish_ops.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(records)} cases of tests/batchfinish_cases.py and the (colour, alpha) plane",
                         np.int64(len(records)).tobytes() + b"".join(records))


if __name__ == "__main__":
    sys.exit(main())
