#!/usr/bin/env python
"""Compare two `bench.py --dump-outputs` directories (the same command from two trees or under two settings) with the bars the
project uses where only list positions and summation order may differ
(tests/test_raster_parity_gpu.py::test_opt_in_culling_of_transparent_surfels_changes_no_pixel and
tests/test_pipeline.py::test_pipeline_equals_the_operators_called_one_by_one):

  image maps                  max |a - b| <= 2.5e-7, at most 1 % of the dumped elements differ at all
  every other map             max |a - b| <= 1e-6,   at most 1 % of the dumped elements differ at all
  loss and its terms          |a - b| <= 1e-6 |b|
  grad_params, grad_feat_vol  max |a - b| <= 1e-2 max |b|, cosine >= 1 - 1e-5   (the bf16-path bar of `close()`; the dump holds
                              the parameters' gradients as ONE flat array, so the 2e-4 bar of the fp32-path parameters cannot
                              be applied to them alone: the figure is printed against 2e-4 too)

usage: tools/compare_dumps.py <dir a> <dir b>      prints one line per array, `PASS` / `FAIL` last; exit status 1 on any FAIL."""
import os
import sys

import numpy as np

MAP_KEYS = ("image", "depth", "acc_map", "rend_normal", "depth_normal", "rend_dist")


def main(a_dir, b_dir):
    names_a = {f[:-4] for f in os.listdir(a_dir) if f.endswith(".npy")}
    names_b = {f[:-4] for f in os.listdir(b_dir) if f.endswith(".npy")}
    ok = names_a == names_b
    if not ok:
        print(f"the two dumps hold different arrays: only in a {sorted(names_a - names_b)}, only in b {sorted(names_b - names_a)}  FAIL")
    for name in sorted(names_a & names_b):
        a, b = (np.load(os.path.join(d, name + ".npy")).astype(np.float64) for d in (a_dir, b_dir))
        if a.shape != b.shape:
            print(f"{name:24s} shapes {a.shape} / {b.shape}  FAIL")
            ok = False
            continue
        d = float(np.abs(a - b).max()) if a.size else 0.0
        mx = float(np.abs(b).max()) if b.size else 0.0
        if name.startswith("grad_"):
            cos = float((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))
            good = d <= 1e-2 * mx + 1e-12 and cos >= 1 - 1e-5
            line = f"max diff {d:.3e} = {d / (mx + 1e-300):.3e} of max (bar 1e-2; 2e-4 {'holds too' if d <= 2e-4 * mx else 'does not hold'}), 1 - cosine {1 - cos:.3e} (bar 1e-5)"
        elif name.startswith("loss"):
            good = d <= 1e-6 * mx
            line = f"a {float(a.ravel()[0])!r} b {float(b.ravel()[0])!r} relative diff {d / (mx + 1e-300):.3e} (bar 1e-6)"
        elif name.startswith(MAP_KEYS):
            bar = 2.5e-7 if name.startswith("image") else 1e-6
            moved = float((a != b).mean())
            good = d <= bar and moved <= 1e-2
            line = f"max diff {d:.3e} (bar {bar:.1e}), elements that differ {moved:.3e} (bar 1e-2), max |b| {mx:.3g}"
        else:
            good = d == 0.0
            line = f"max diff {d:.3e} (expected equal)"
        ok = ok and good
        print(f"{name:24s} n {a.size:8d}  {line}  {'PASS' if good else 'FAIL'}")
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
