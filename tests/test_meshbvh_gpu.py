"""csrc/meshbvh.hip held to the restatement of its header (tests/meshbvh_restate.py) and to `meshdist.TriangleGrid`: the build --
keys, sorted order, records, every level's boxes, the header's counts -- equal to the numpy restatement exactly on every case of
tests/meshdist_cases.py; the query equal to ``TriangleGrid.query`` BIT FOR BIT on every case (dist, face and closest point compared
as integers, no pair exempt: both are argmins of the same computed numbers under the same tie rule), and independently within the
two bars of tests/meshdist_cases.check_against_brute_force; exact ties across subtrees; 4 096 copies of one triangle; inputs
without a candidate; reproducibility; `icp`, `aligned_scores` and `mesh_scores` with ``search="bvh"`` equal to the grid's results;
the bench tool at its --quick size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import meshbvh_cases as BC
from tests import meshbvh_restate as RB
from tests import meshdist_cases as C
from tests import meshdist_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


_runs = {}


def _case(key):
    """One device build and query of the case with both structures, shared by the tests."""
    if key not in _runs:
        from lara_amd import meshbvh, meshdist
        Q, V, F = C.CASES[key]()
        bvh = meshbvh.TriangleBVH(_t(V), _t(F))
        grid = meshdist.TriangleGrid(_t(V), _t(F))
        _runs[key] = {"Q": Q, "V": V, "F": F, "bvh": bvh, "got": bvh.query(_t(Q), return_closest=True, return_fallbacks=True),
                      "grid": grid.query(_t(Q), return_closest=True)}
    return _runs[key]


@pytest.mark.parametrize("key", sorted(C.CASES))
def test_build_equals_the_restatement(hip_lib, key):
    r = _case(key)
    bvh, ref = r["bvh"], RB.BVH(r["V"], r["F"])
    assert bvh.counts.cpu().tolist() == ref.counts
    assert np.array_equal(bvh.keys.cpu().numpy(), ref.sorted_keys)                                  # keys and their sorted order
    assert sorted(ref.keys.tolist()) == ref.sorted_keys.tolist() and len(set(ref.keys.tolist())) == len(r["F"])
    assert np.array_equal(bvh.records.cpu().numpy().view(np.int32), ref.records.view(np.int32))
    assert len(bvh.layout["levels"]) == len(ref.levels)
    for k, boxes in enumerate(ref.levels):
        assert np.array_equal(bvh.level_boxes(k).cpu().numpy().view(np.int32), boxes.view(np.int32)), (key, k)
    assert bvh.nbytes == RB.nbytes(len(r["F"]))


@pytest.mark.parametrize("key", sorted(C.CASES))
def test_query_equals_the_grid_bit_for_bit(hip_lib, key):
    r = _case(key)
    Q, V, F = r["Q"], r["V"], r["F"]
    d, face, closest, fb = r["got"]
    gd, gface, gclosest = r["grid"]
    assert torch.equal(face, gface), (key, int((face != gface).sum()))
    assert torch.equal(_bits(d), _bits(gd)) and torch.equal(_bits(closest), _bits(gclosest))
    assert fb.dtype == torch.int32 and fb.shape == (1,) and int(fb.item()) == 0
    d64_min, face64, d2_all = R.brute(Q, V, F)
    r_dist, r_choice = C.check_against_brute_force(key, Q, V, F, d.cpu().numpy().astype(np.float64), face.cpu().numpy().astype(np.int64),
                                                   d64_min, d2_all)
    print(f"meshbvh {key}: distance {r_dist:.4f}, choice {r_choice:.4f} of the bars")
    assert r_dist <= 1.0 and r_choice <= 1.0, (key, r_dist, r_choice)
    if key == "identical":
        assert bool((face == 0).all())
    if key == "bad_triangles":
        assert not set(face.cpu().tolist()) & set(C.BAD)


def test_ties_across_subtrees_go_to_the_smaller_face(hip_lib):
    """Mirror-image triangles at x = -1 and x = +1 in different level-1 nodes, queries on the plane x = 0 (dyadic coordinates: the
    two d2 have equal bits): face 0 whichever of the two it names."""
    from lara_amd import meshbvh, meshdist
    for swap in (False, True):
        Q, V, F, minus, plus = BC.mirror_pair(swap)
        bvh = meshbvh.TriangleBVH(_t(V), _t(F))
        ids = bvh.records[:, 9].contiguous().view(torch.int32).cpu().numpy()
        pos = {int(i): k for k, i in enumerate(ids)}
        assert pos[minus] >> 6 != pos[plus] >> 6
        d2 = R.all_d2(Q, V, F)
        assert np.all(d2[:, minus].view(np.int64) == d2[:, plus].view(np.int64)) and np.all(d2.argmin(1) == 0)
        got = bvh.query(_t(Q), return_closest=True)
        assert got[1].cpu().tolist() == [0] * len(Q)
        assert _same(got, meshdist.TriangleGrid(_t(V), _t(F)).query(_t(Q), return_closest=True))
        assert np.array_equal(got[0].cpu().numpy(), np.sqrt(d2[:, 0]).astype(np.float32))


def test_copies_of_one_triangle(hip_lib):
    """4 096 copies: every Morton code is equal and the order is by id alone; face 0 everywhere, on the triangle (d2 = 0 = every
    node's bound: only the strict skip rule reaches face 0) and off it, and the bits of the one-triangle mesh."""
    from lara_amd import meshbvh
    Q, V, F, tri = BC.copies(4096)
    bvh = meshbvh.TriangleBVH(_t(V), _t(F))
    assert torch.equal(bvh.keys & ((1 << 26) - 1), torch.arange(4096, device=_dev()))
    assert len(set((bvh.keys >> 26).cpu().tolist())) == 1 and bvh.counts.cpu().tolist() == [0, 4096, 4096, 4]
    d, face, c = bvh.query(_t(Q), return_closest=True)
    assert face.cpu().tolist() == [0] * len(Q) and d[:6].cpu().tolist() == [0.0] * 6
    one = meshbvh.point_to_mesh(_t(Q), _t(tri), _t(np.array([[0, 1, 2]])), return_closest=True)
    assert _same((d, face, c), one)


def test_queries_and_meshes_without_a_candidate(hip_lib):
    """A query with a coordinate that is not finite, a mesh with no valid triangle, a mesh of bad triangles only: face -1,
    dist +inf, closest NaN, as the grid gives them; N = 0 is a no-op."""
    from lara_amd import meshbvh
    V, F = R.icosphere(1)
    bvh = meshbvh.TriangleBVH(_t(V), _t(F))
    Q = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.5, 0.5, 0.5], [np.nan, np.nan, np.nan]], np.float32)
    d, face, c, fb = bvh.query(_t(Q), return_closest=True, return_fallbacks=True)
    d, face, c = d.cpu().numpy(), face.cpu().numpy(), c.cpu().numpy()
    assert face.tolist()[:3] == [-1, -1, -1] and face[4] == -1 and face[3] >= 0 and np.isfinite(d[3]) and np.isfinite(c[3]).all()
    assert np.all(np.isposinf(d[[0, 1, 2, 4]])) and np.isnan(c[[0, 1, 2, 4]]).all() and int(fb.item()) == 0
    none = meshbvh.TriangleBVH(_t(V), _t(np.full((5, 3), len(V) + 1, np.int64)))
    d, face, c = none.query(_t(Q[3:4]), return_closest=True)
    assert face.item() == -1 and np.isposinf(d.item()) and bool(torch.isnan(c).all()) and none.counts.cpu().tolist() == [5, 0, 5, 1]
    Vn = V.copy()
    Vn[:, 1] = np.nan                                    # every triangle has a coordinate that is not finite
    bad = meshbvh.TriangleBVH(_t(Vn), _t(F))
    d, face, c = bad.query(_t(Q), return_closest=True)
    assert bad.counts.cpu().tolist()[:2] == [len(F), 0] and bool((face == -1).all()) and bool(torch.isposinf(d).all()) and bool(torch.isnan(c).all())
    d, face = bvh.query(_t(Q[:0]))
    assert d.shape == (0,) and face.shape == (0,)
    with pytest.raises(ValueError):
        meshbvh.TriangleBVH(_t(V), _t(F[:0]))


def test_query_is_reproducible_and_follows_a_permutation(hip_lib):
    from lara_amd import meshbvh
    V, F = R.icosphere(3)
    F = np.concatenate([F[:1279], F[100:101]])                 # two identical triangles: exact ties
    Q = R.rippled_sphere_points(4096, 41)
    q, v = _t(Q), _t(V)
    bvh = meshbvh.TriangleBVH(v, _t(F))
    first = bvh.query(q, return_closest=True)
    assert _same(first, bvh.query(q, return_closest=True))
    again = meshbvh.TriangleBVH(v, _t(F))
    assert torch.equal(again.keys, bvh.keys) and torch.equal(_bits(again.records), _bits(bvh.records))
    assert all(torch.equal(_bits(again.level_boxes(k)), _bits(bvh.level_boxes(k))) for k in range(len(bvh.layout["levels"])))
    assert _same(first, again.query(q, return_closest=True))
    perm = np.random.default_rng(42).permutation(len(F))
    d4, f4 = meshbvh.point_to_mesh(q, v, _t(F[perm]))
    assert torch.equal(_bits(first[0]), _bits(d4))
    back, f1h = perm[f4.cpu().numpy()], first[1].cpu().numpy()
    moved = back != f1h
    d2_all = R.all_d2(Q[moved], V, F)
    k = np.arange(moved.sum())
    assert np.all(d2_all[k, back[moved]] == d2_all[k, f1h[moved]])          # only where the minimum is not unique
    assert np.all(f1h != 1279)                                               # of the identical pair, the smaller id


def _strip(history):
    return [{k: v for k, v in h.items() if k != "fallbacks"} for h in history]


def test_icp_with_the_bvh_equals_icp_with_the_grid(hip_lib):
    """`registration_case(3, 10)`, plane mode: the same correspondences bit for bit, hence the same transformation bits, iterations
    and history; no fallbacks with the BVH.  ``search="grid"`` is the call without the keyword."""
    from lara_amd import meshalign
    from tests import meshalign_cases as AC
    S, V, F, _ = AC.registration_case(3, 10)
    s, mesh = _t(S), (_t(V), _t(F))
    plain = meshalign.icp(s, mesh, max_dist=AC.MAX_DIST)
    grid = meshalign.icp(s, mesh, max_dist=AC.MAX_DIST, search="grid")
    bvh = meshalign.icp(s, mesh, max_dist=AC.MAX_DIST, search="bvh")
    assert np.array_equal(plain["transformation"].view(np.int64), grid["transformation"].view(np.int64)) and \
        {k: v for k, v in plain.items() if k != "transformation"} == {k: v for k, v in grid.items() if k != "transformation"}
    assert np.array_equal(bvh["transformation"].view(np.int64), grid["transformation"].view(np.int64))
    assert bvh["iterations"] == grid["iterations"] > 0 and bvh["converged"] == grid["converged"]
    assert _strip(bvh["history"]) == _strip(grid["history"])
    assert bvh["fallbacks"] == 0 and all(h["fallbacks"] == 0 for h in bvh["history"])
    for k in ("scale", "fitness", "inlier_rmse"):
        assert bvh[k] == grid[k]
    a = meshalign.aligned_scores(mesh, mesh, n=4096, distance="triangle", max_dist=AC.MAX_DIST, init=AC_init(), search="bvh")
    b = meshalign.aligned_scores(mesh, mesh, n=4096, distance="triangle", max_dist=AC.MAX_DIST, init=AC_init())
    assert a["fallbacks"] == 0 and a["alignment"]["fallbacks"] == 0 and a["distance"] == "triangle"
    ra, rb = a.pop("alignment"), b.pop("alignment")
    assert {k: v for k, v in a.items() if k != "fallbacks"} == {k: v for k, v in b.items() if k != "fallbacks"}
    assert np.array_equal(ra["transformation"].view(np.int64), rb["transformation"].view(np.int64)) and \
        _strip(ra["history"]) == _strip(rb["history"])


def AC_init():
    """A start 10 degrees off, so that the registration inside `aligned_scores` has something to do."""
    from tests import meshalign_restate as AR
    from tests import meshalign_cases as AC
    return AR.rigid(10, t=AC.STARTS[10])


def test_mesh_scores_with_the_bvh_equal_mesh_scores(hip_lib):
    """The icosphere against its rippled copy: every key of the dict but ``fallbacks`` (0 with the BVH), and the samples' bits."""
    from lara_amd import meshdist
    V, F = R.icosphere(3)
    d = V.astype(np.float64)
    Vr = (d * (1.0 + 0.01 * np.sin(7 * d[:, :1]) * np.cos(5 * d[:, 1:2] + 3 * d[:, 2:3]))).astype(np.float32)
    pred, gt = (_t(Vr), _t(F)), (_t(V), _t(F))
    plain = meshdist.mesh_scores(pred, gt, n=4096, return_samples=True)
    grid = meshdist.mesh_scores(pred, gt, n=4096, return_samples=True, search="grid")
    bvh = meshdist.mesh_scores(pred, gt, n=4096, return_samples=True, search="bvh")
    assert set(plain) == set(grid) == set(bvh) and bvh["fallbacks"] == 0 and bvh["distance"] == "triangle"
    for k in plain:
        if k == "samples":
            assert _same([t for t in plain[k] if t is not None], [t for t in grid[k] if t is not None])
            assert _same([t for t in plain[k] if t is not None], [t for t in bvh[k] if t is not None])
        else:
            assert plain[k] == grid[k], k
            assert k == "fallbacks" or plain[k] == bvh[k], k
    assert plain["accuracy"] > 0 and plain["chamfer"] > 0
    got = meshdist.point_to_mesh(plain["samples"][0], *gt, return_closest=True, search="bvh")
    assert _same(got, meshdist.point_to_mesh(plain["samples"][0], *gt, return_closest=True))


def test_bench_tool_runs_at_its_quick_size(hip_lib, tmp_path):
    out = tmp_path / "bench.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "meshbvh_bench.py"), "--quick", "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(run.stdout.strip().splitlines()[-1]) == res
    assert res["T"] <= 20000 and res["build"]["grid_ms"] > 0 and res["build"]["bvh_ms"] > 0
    assert res["build"]["bvh_bytes"] == RB.nbytes(res["T"]) < res["build"]["grid_bytes"]
    assert len(res["rows"]) == 5 and res["all_rows_same_bits"]
    for row in res["rows"]:
        assert row["grid_ms"] > 0 and row["bvh_ms"] > 0 and row["bvh_fallbacks"] == 0 and row["same_bits"]
    assert res["icp"]["same_transformation_bits"] and res["icp"]["bvh"]["fallbacks"] == 0
    assert res["icp"]["bvh"]["iterations"] == res["icp"]["grid"]["iterations"]
