"""Runs csrc/texatlas.h -- the layout and the three per-element functions the kernels of csrc/meshtexture.hip and the library's host
entries run -- as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer, over every case and every bake
variant of tests/meshtexture_cases.py and a dense barycentric sample per case.  Writes the records with the float64 restatement's
answers (tests/meshtexture_restate.py) to a temporary file, compiles tools/meshtexture_hostcheck.cpp with -fsanitize=address,undefined
-ffp-contract=off, runs it, and prints (``--out``: also appends) the outcome: every output must equal the restatement's bytes.  CPU
only: nothing is loaded into python and no device is touched.
    python tools/meshtexture_hostcheck.py [--cxx g++] [--out profiles/meshtexture_parity.txt]"""
import io
import os
import sys

import numpy as np

import hostcheck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import meshtexture_cases as TC  # noqa: E402
from tests import meshtexture_restate as X  # noqa: E402


def block(f, a, dtype):
    a = np.ascontiguousarray(a, dtype).ravel()
    f.write(np.int64(a.size).tobytes() + a.tobytes())


def main():
    f = io.BytesIO()
    f.write(np.int64(len(TC.KEYS)).tobytes())
    for key in TC.KEYS:
        c = TC.case(key)
        L, T = c["layout"], len(c["F"])
        nv, H, W = c["images"].shape[:3]
        block(f, [L[0], L[1], T, len(c["V"]), nv, H, W], np.int32)
        for name, dtype in (("V", np.float32), ("F", np.int32), ("images", np.float32), ("k", np.float32), ("w2c", np.float32),
                            ("eyes", np.float32), ("colours", np.float32), ("mask", np.int64)):
            block(f, c[name], dtype)
        face, point, anchor = X.texels(L, c["V"], c["F"])
        block(f, face, np.int32), block(f, point, np.float32), block(f, anchor, np.float32)
        block(f, [len(TC.VARIANTS)], np.int32)
        for name, kw in TC.VARIANTS:
            fill = kw.get("fill", (0, 0, 0))
            block(f, [kw.get("near", 0.0), kw.get("min_cos", 0.1), kw.get("power", 2), kw.get("two_sided", False), kw["blend"] == "best",
                      kw.get("mask", False), kw.get("colours", False), fill[0], fill[1], fill[2]], np.float32)
            texture, weight, view = TC.restated(key, name)
            block(f, texture, np.uint8), block(f, weight, np.float32), block(f, view, np.int32)
        g = np.random.default_rng(11)
        bary = np.concatenate([TC.dense_bary(12), (g.random((200, 3)) * 1.4 - 0.2).astype(np.float32), np.array([[np.nan, np.nan, 0.5]], np.float32)])
        sf = g.integers(-1, T + 2, len(bary)).astype(np.int32)
        block(f, sf, np.int32), block(f, bary, np.float32)
        block(f, X.sample(L, T, texture, sf, bary, True, (0.1, 0.2, 0.3)), np.float32)
    return hostcheck.run(__file__, "texatlas.h, stand-alone host program, {cxx} -fsanitize=address,undefined, "
                         f"{len(TC.KEYS)} cases x {len(TC.VARIANTS)} bake variants", f.getvalue())


if __name__ == "__main__":
    sys.exit(main())
