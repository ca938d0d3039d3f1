"""`lara_amd/csrc/tilebox.h` -- the one statement of "does this cull box meet this cell of pixels", shared by the composite's
staging and the preprocess's tight binning -- on the host: the header itself, compiled into a stand-alone program, and its
numpy restatement `tile_keep` (which tests/test_tight_tiles_gpu.py holds the device lists to), both against a brute-force loop
over a tile's 16 pixel coordinates for boxes on a grid of bounds, +-INF, the empty box and NaN included."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tile_keep(cullbox, tx, ty):
    """Does tight binning keep the pair (surfel with `cullbox` = (minx, maxx, miny, maxy) [..., 4], tile (tx, ty))?  Pixels sit at
    integer coordinates, tile tx covers 16 tx ... 16 tx + 15: the box meets it in x iff minx <= 16 tx + 15 and maxx >= 16 tx.
    The empty box (INF, -INF, INF, -INF) meets nothing, the unbounded box everything; a NaN bound keeps the pair."""
    cb = np.asarray(cullbox, np.float64)
    tx, ty = np.asarray(tx, np.float64), np.asarray(ty, np.float64)
    minx, maxx, miny, maxy = cb[..., 0], cb[..., 1], cb[..., 2], cb[..., 3]
    with np.errstate(invalid="ignore"):
        meets = (minx <= 16 * tx + 15) & (maxx >= 16 * tx) & (miny <= 16 * ty + 15) & (maxy >= 16 * ty)
    return meets | np.isnan(cb).any(-1)


def test_tile_keep_is_the_brute_force_over_a_tiles_pixels():
    inf = np.inf
    b = np.array([-inf, -100, -17, -16, -15.5, -1, -0.5, 0, 0.5, 14.5, 15, np.float32(15.000001), 15.5, 16, 17, 31, 31.5, 32, 47, 47.5, 48,
                  63, 64, 1000, inf, np.nan])
    boxes = np.stack(np.meshgrid(b, b, [-inf, 3.0, 20.0, inf, np.nan], [-inf, 15.0, 33.0, inf], indexing="ij"), -1).reshape(-1, 4)
    for ty in range(3):
        for tx in range(4):
            px, py = 16 * tx + np.arange(16), 16 * ty + np.arange(16)
            with np.errstate(invalid="ignore"):
                want = ((boxes[:, None, 0] <= px).any(1) & (boxes[:, None, 1] >= px).any(1) &
                        (boxes[:, None, 2] <= py).any(1) & (boxes[:, None, 3] >= py).any(1))
            want |= np.isnan(boxes).any(1)
            assert np.array_equal(tile_keep(boxes, tx, ty), want), (tx, ty)
    # the two special boxes and NaN, spelled out
    assert not tile_keep([inf, -inf, inf, -inf], 0, 0) and tile_keep([-inf, inf, -inf, inf], 5, 7)
    assert tile_keep([np.nan, 3.0, 0.0, 3.0], 9, 9) and not tile_keep([0.0, 3.0, 0.0, 3.0], 1, 0)
    # a box thinner than a pixel, between two pixels of tile 0, still meets tile 0 (the test is on the tile's span, conservative)
    assert tile_keep([3.2, 3.8, 3.2, 3.8], 0, 0) and not tile_keep([15.2, 15.8, 3.0, 4.0], 0, 0) and not tile_keep([15.2, 15.8, 3.0, 4.0], 1, 0)


def test_the_shared_header_on_the_host_matches_the_brute_force(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler (the oracle's build needs one too)"
    exe = str(tmp_path / "tilebox_host")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "lara_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tilebox_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 100000 and int(last[3]) == 0, r.stdout
