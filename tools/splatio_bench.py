"""Wall times of `lara_amd.splatio.write_ply` / `read_ply` for the headline scene's surfel count (64^3 x 2 = 524 288, SH degree 1)
beside the floor they are measured against: ``numpy.tofile`` / ``numpy.fromfile`` of one buffer of the body's size.  ONE run of
each, in this order, into a fresh temporary directory: no spread is measured, and the figures include whatever the page cache of
the machine does (the files are not synced).  The tensors lie on the GPU when there is one (the write then includes the one
device-to-host copy, the read the one host-to-device copy), else on the host.
    python tools/splatio_bench.py [--grid 64] [--out profiles/splatio_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lara_amd import splatio, synthetic
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    sc = synthetic.make_scene(grid=args.grid, K=2, regime="trained", sh_coeffs=4, device=dev)
    cloud = splatio.SurfelCloud(*(sc[k] for k in ("centers", "shs", "opacity", "scales", "rotations")))

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def wall(f):
        sync()
        t0 = time.perf_counter()
        r = f()
        sync()
        return r, time.perf_counter() - t0

    with tempfile.TemporaryDirectory() as d:
        ply, raw = os.path.join(d, "point_cloud.ply"), os.path.join(d, "floor.bin")
        nbytes, t_write = wall(lambda: splatio.write_ply(ply, cloud))
        (back, _), t_read = wall(lambda: splatio.read_ply(ply, device=dev))
        body = np.zeros(nbytes - len(splatio.ply_header(cloud.n_surfels, cloud.sh_degree)), np.uint8)
        _, t_tofile = wall(lambda: body.tofile(raw))
        _, t_fromfile = wall(lambda: np.fromfile(raw, np.uint8))
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(back.render_args(), cloud.render_args()))
    res = {"device": str(dev), "n_surfels": cloud.n_surfels, "sh_degree": cloud.sh_degree, "file_bytes": nbytes,
           "bytes_per_surfel": (nbytes - len(splatio.ply_header(cloud.n_surfels, cloud.sh_degree))) // max(cloud.n_surfels, 1),
           "write_ply_s": t_write, "read_ply_s": t_read, "floor_numpy_tofile_s": t_tofile, "floor_numpy_fromfile_s": t_fromfile,
           "round_trip_same_bits": same, "runs": 1}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
