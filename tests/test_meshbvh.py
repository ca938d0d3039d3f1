"""include/lara_meshbvh.h without a GPU: the header's constants held to the module's, the library's refusals and its size formula;
the margined bound of csrc/boxbound.h, through its host entry, held under the distance csrc/tridist.h computes (the host entry of
meshdist) on random, flat, shifted and degenerate pairs -- and an unmargined float64 bound shown to FAIL on the flat ones, so the
cases bite; the restated walk (tests/meshbvh_restate.py) held to restated brute force on every case of tests/meshdist_cases.py;
the ``search=`` keyword's refusals and the Evaluator hook.  tests/test_meshbvh_gpu.py holds the kernels to the same restatement.

The bound's bar is the contract itself, with no tolerance: bound(q, box) <= d2(q, t) as computed, for every triangle t in the box."""
import sys

import numpy as np
import pytest
import torch

from lara_amd import _native, evaluate
from tests import meshbvh_cases as BC
from tests import meshbvh_restate as RB
from tests import meshdist_cases as C
from tests import meshdist_restate as R

F32 = np.float32


def test_header_constants_equal_the_modules():
    from lara_amd import meshbvh
    from tests import test_abi_cpu as abi
    assert (meshbvh.MAX_LEVELS, meshbvh.HEADER_INTS) == (9, 4) == (RB.MAX_LEVELS, 4)
    assert (meshbvh.HDR_BAD, meshbvh.HDR_VALID, meshbvh.HDR_TRIANGLES, meshbvh.HDR_LEVELS) == (0, 1, 2, 3)
    text = abi.header_texts()["lara_meshbvh.h"]
    for macro, value in (("MAX_LEVELS", 9), ("HEADER_INTS", 4), ("HDR_BAD", 0), ("HDR_VALID", 1), ("HDR_TRIANGLES", 2), ("HDR_LEVELS", 3)):
        assert f"#define LARA_MESHBVH_{macro} {value}\n" in text


def test_refusals_and_the_size_formula(hip_lib):
    """T <= 0, T >= 2^26, N >= 2^30 and null pointers come back as LARA2DGS_E_INVALID (-1) from host code, before any pointer is
    used; N = 0 is a no-op; python refuses CPU tensors and unknown ``search`` values.  lara_meshbvh_bytes equals the header's
    formula, is monotone, and stays within 60 bytes a triangle plus 32 KB."""
    from lara_amd import meshalign, meshbvh, meshdist
    out = (_native._i64 * 22)()
    for T in (0, -3, 1 << 26, 1 << 28):
        assert hip_lib.lara_meshbvh_bytes(T) == -1
        assert hip_lib.lara_meshbvh_layout(T, out) == -1
        assert hip_lib.lara_meshbvh_keys(8, T, 1, 1, 1, None) == -1          # (non-null pointers that must not be used)
        assert hip_lib.lara_meshbvh_build(8, T, 1, 1, 1, None) == -1
    assert hip_lib.lara_meshbvh_layout(4, None) == -1
    for fn in (hip_lib.lara_meshbvh_keys, hip_lib.lara_meshbvh_build):
        assert fn(8, 4, None, None, None, None) == -1 and fn(0, 4, 1, 1, 1, None) == -1 and fn(1 << 30, 4, 1, 1, 1, None) == -1
    assert hip_lib.lara_meshbvh_query(1 << 30, 1, 1, 1, 1, None, None) == -1 and hip_lib.lara_meshbvh_query(-1, 1, 1, 1, 1, None, None) == -1
    assert hip_lib.lara_meshbvh_query(0, None, None, None, None, None, None) == 0
    assert hip_lib.lara_meshbvh_query(5, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshbvh_box_bound_host(-1, None, None, None) == -1
    assert hip_lib.lara_meshbvh_box_bound_host(3, None, None, None) == -1
    assert hip_lib.lara_meshbvh_box_bound_host(0, None, None, None) == 0
    Ts = (1, 2, 7, 8, 9, 63, 64, 65, 257, 512, 513, 1280, 4096, 4097, 262144, 556516, (1 << 26) - 1)
    sizes = [hip_lib.lara_meshbvh_bytes(t) for t in Ts]
    assert sizes == [RB.nbytes(t) for t in Ts] and sizes == sorted(sizes)
    assert all(59 * t <= s <= 60 * t + 32768 for t, s in zip(Ts, sizes))
    assert all(hip_lib.lara_meshbvh_bytes(t) <= hip_lib.lara_meshbvh_bytes(t + 1) for t in range(1, 3000))
    for t in Ts:
        assert hip_lib.lara_meshbvh_layout(t, out) == 0
        counts = RB.level_counts(t)
        assert out[2] == len(counts) <= 9 and [out[5 + 2 * k] for k in range(out[2])] == counts and out[3] == RB.nbytes(t)
        offs = [out[0], out[1]] + [out[4 + 2 * k] for k in range(out[2])]
        assert offs == sorted(offs) and offs[0] == 256 and all(o % 256 == 0 for o in offs)
        assert out[1] - out[0] >= 8 * t and offs[2] - out[1] >= 48 * t + 24 * 1024
        assert out[3] - offs[-1] >= 24 * 8
    assert [n for _, n in meshbvh.layout(1280)["levels"]] == [160, 20, 3, 1]
    V, F = R.icosphere(0)
    mesh = (torch.from_numpy(V), torch.from_numpy(F))
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshbvh.TriangleBVH(*mesh)
    for search in ("grid", "bvh"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            meshdist.point_to_mesh(torch.zeros(4, 3), *mesh, search=search)
        with pytest.raises(RuntimeError, match="no CPU path"):
            meshdist.mesh_scores(mesh, torch.zeros(4, 3), device="cpu", search=search)
        with pytest.raises(RuntimeError, match="no CPU path"):
            meshalign.icp(torch.zeros(4, 3), mesh, max_dist=1.0, device="cpu", search=search)
    for fn in (lambda: meshdist.point_to_mesh(torch.zeros(4, 3), *mesh, search="tree"),
               lambda: meshdist.mesh_scores(mesh, mesh, device="cpu", search="tree"),
               lambda: meshalign.icp(mesh, mesh, max_dist=1.0, device="cpu", search="tree"),
               lambda: meshalign.align_mesh(mesh, mesh, max_dist=1.0, device="cpu", search=None),
               lambda: meshalign.aligned_scores(mesh, mesh, max_dist=1.0, device="cpu", search="BVH")):
        with pytest.raises(ValueError, match="'grid' or 'bvh'"):
            fn()


def test_the_default_route_does_not_touch_meshbvh():
    """``search="grid"`` and no keyword never import `lara_amd.meshbvh` (both routes end at the "no CPU path" check here)."""
    import lara_amd
    from lara_amd import meshalign, meshdist
    V, F = R.icosphere(0)
    mesh = (torch.from_numpy(V), torch.from_numpy(F))
    saved = sys.modules.pop("lara_amd.meshbvh", None)          # (as in a process that has not imported it yet)
    vars(lara_amd).pop("meshbvh", None)
    try:
        for kw in ({}, {"search": "grid"}):
            for fn in (lambda **k: meshdist.point_to_mesh(torch.zeros(4, 3), *mesh, **k),
                       lambda **k: meshdist.mesh_scores(mesh, mesh, n=16, device="cpu", **k),
                       lambda **k: meshalign.icp(mesh, mesh, max_dist=1.0, device="cpu", **k),
                       lambda **k: meshalign.aligned_scores(mesh, mesh, max_dist=1.0, device="cpu", **k)):
                with pytest.raises(RuntimeError, match="no CPU path"):
                    fn(**kw)
                assert "lara_amd.meshbvh" not in sys.modules
        with pytest.raises(RuntimeError, match="no CPU path"):
            meshdist.point_to_mesh(torch.zeros(4, 3), *mesh, search="bvh")
        assert "lara_amd.meshbvh" in sys.modules
    finally:
        if saved is not None:
            sys.modules["lara_amd.meshbvh"] = lara_amd.meshbvh = saved


# ---- the bound ------------------------------------------------------------------------------------------------------------------

def _host_bound(hip_lib, q, lo, hi):
    q = np.ascontiguousarray(q, F32)
    boxes = np.ascontiguousarray(np.concatenate([lo, hi], 1), F32)
    out = np.empty(len(q))
    assert hip_lib.lara_meshbvh_box_bound_host(len(q), q.ctypes.data, boxes.ctypes.data, out.ctypes.data) == 0
    return out


def _host_d2(hip_lib, q, tri):
    q = np.ascontiguousarray(q, F32)
    t9 = np.ascontiguousarray(tri.reshape(len(tri), 9), F32)
    d2 = np.empty(len(q))
    assert hip_lib.lara_meshdist_point_triangle_host(len(q), q.ctypes.data, t9.ctypes.data, d2.ctypes.data, None) == 0
    return d2


_pairs = {}


def _bound_pairs():
    if not _pairs:
        _pairs.update(BC.bound_pairs())
    return _pairs


def test_bound_never_exceeds_the_computed_distance(hip_lib):
    """Every pair of tests/meshbvh_cases.bound_pairs: the host entry's bound of the box (tight, or larger where the name says so)
    is <= the d2 the host entry of meshdist computes for the triangle inside it; the host entry equals the restated bound bit for
    bit; a query on or in the box has bound 0."""
    for name, (q, tri, lo, hi) in sorted(_bound_pairs().items()):
        assert np.all(lo <= tri.min(1)) and np.all(hi >= tri.max(1))
        b = _host_bound(hip_lib, q, lo, hi)
        d2 = _host_d2(hip_lib, q, tri)
        assert np.array_equal(b.view(np.int64), RB.bounds(q, lo, hi).view(np.int64)), name
        worst = float((b / np.where(d2 > 0, d2, 1.0)).max())
        print(f"meshbvh bound, {name}: {len(q)} pairs, largest bound / d2 = {worst:.12f}, {int((b == 0).sum())} zero bounds")
        assert np.all(b <= d2), (name, int((b > d2).sum()))
        assert np.all(b >= 0) and np.all(np.isfinite(b))
        if name == "on the box":
            assert np.all(b == 0)
        if name in ("random", "flat"):          # the margin gives little away: most bounds are within 2^-11 of the unmargined s
            s = RB.bounds(q, lo, hi, margin=False)
            far = s > 1e-6 * np.abs(np.concatenate([q, lo, hi], 1)).max(1) ** 2
            assert far.sum() > len(q) // 4 and np.all(b[far] >= s[far] * (1 - 2.0 ** -11))


def test_bound_of_special_boxes(hip_lib):
    """The empty box (lo > hi, as the build stores it) is +inf wherever the query is; a box that is a point is the squared distance
    to it less the margin; the bound of a box grows when the box shrinks."""
    g = np.random.default_rng(60)
    q = (g.random((100, 3)) * 20 - 10).astype(F32)
    inf = np.full((100, 3), np.inf, F32)
    assert np.all(np.isposinf(_host_bound(hip_lib, q, inf, -inf)))
    assert np.isposinf(RB.bound(q[0], inf[0], -inf[0]))
    p = (g.random((100, 3)) * 2 - 1).astype(F32)
    b = _host_bound(hip_lib, q, p, p)
    exact = ((q.astype(np.float64) - p.astype(np.float64)) ** 2).sum(1)
    assert np.all(b <= exact) and np.all(b >= exact * (1 - 2.0 ** -11) - 2.0 ** -39 * 100)
    lo, hi = p - F32(0.5), p + F32(0.5)
    assert np.all(_host_bound(hip_lib, q, lo, hi) <= b)
    assert np.all(_host_bound(hip_lib, q, lo - F32(1), hi + F32(1)) <= _host_bound(hip_lib, q, lo, hi))


def test_an_unmargined_bound_fails_on_the_flat_cases(hip_lib):
    """Teeth: the same comparison with the unmargined float64 s must find violations on the flat, axis-aligned triangles -- the
    computed (s s) / nn rounds below the box's exact distance --, so those cases can tell a bound without a margin."""
    total = 0
    for name in BC.FLAT:
        q, tri, lo, hi = _bound_pairs()[name]
        s = RB.bounds(q, lo, hi, margin=False)
        d2 = _host_d2(hip_lib, q, tri)
        bad = s > d2
        excess = float(((s - d2)[bad] / d2[bad]).max()) if bad.any() else 0.0
        print(f"meshbvh unmargined bound, {name}: {int(bad.sum())} of {len(q)} pairs exceed the computed d2, by up to {excess:.2e} relative")
        assert excess < 2.0 ** -40
        total += int(bad.sum())
        if name in ("flat", "flat, 0.001 above"):
            assert bad.sum() > 20, name
    assert total > 100


# ---- the restated walk against restated brute force -----------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(C.CASES))
def test_restated_search_equals_brute_force(key):
    """Identical faces and d2 bits: both sides run the same float64 function and the same (d2, id) order."""
    Q, V, F = C.CASES[key]()
    step = max(1, len(Q) // 80)
    Q = Q[::step] if key not in ("sphere_square", "termination") else np.concatenate([Q[:30], Q[-40:]])
    bvh = RB.BVH(V, F)
    d64, face, _ = R.brute(Q, V, F)
    got = [bvh.search(q) for q in Q]
    assert [g[0] for g in got] == face.tolist()
    assert np.array_equal(np.sqrt([g[1] for g in got]), d64)
    valid = R.valid_triangles(V, F)
    assert bvh.counts == [int((~valid).sum()), int(valid.sum()), len(F), len(RB.level_counts(len(F)))]
    assert sorted(bvh.order.tolist()) == list(range(len(F))) and np.all(bvh.rec_id[:bvh.n_valid] >= 0) and np.all(bvh.rec_id[bvh.n_valid:] == -1)
    tests = np.mean([g[2]["tests"] for g in got])
    print(f"meshbvh restated walk {key}: {len(bvh.levels)} levels, {tests:.0f} triangle tests and "
          f"{np.mean([g[2]['nodes'] for g in got]):.0f} slots per query of {int(valid.sum())} triangles")
    if key in ("icosphere", "uv_sphere", "soup_1280_4096"):          # the walk prunes: a small part of the mesh is tested
        assert tests < 0.1 * valid.sum()
    if key == "bad_triangles":
        assert bvh.counts[:2] == [3, 60] and not set(face) & set(C.BAD)


def test_restated_search_on_ties_and_without_candidates():
    for swap in (False, True):
        Q, V, F, minus, plus = BC.mirror_pair(swap)
        bvh = RB.BVH(V, F)
        pos = {int(i): r for r, i in enumerate(bvh.rec_id)}
        assert pos[minus] >> 6 != pos[plus] >> 6          # different level-1 nodes
        d2 = R.all_d2(Q, V, F)
        assert np.all(d2[:, minus].view(np.int64) == d2[:, plus].view(np.int64)) and np.all(d2.argmin(1) == 0)
        assert [bvh.search(q)[0] for q in Q] == [0] * len(Q)
    # copies of one triangle, queries on it: d2 = 0 = the bound of every node, and only the strict rule keeps face 0
    Q, V, F, _ = BC.copies(100)
    bvh = RB.BVH(V, F)
    assert bvh.order.tolist() == list(range(100))
    assert [bvh.search(q)[0] for q in Q[:20]] == [0] * 20
    assert [bvh.search(q)[1] for q in Q[:6]] == [0.0] * 6
    assert any(bvh.search(q, strict=False)[0] != 0 for q in Q[:6])
    V1, F1 = R.icosphere(1)
    bvh = RB.BVH(V1, F1)
    for q in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
        assert bvh.search(q)[:2] == (-1, np.inf)
    none = RB.BVH(V1, np.full((5, 3), len(V1) + 1, np.int64))
    assert none.search([0.5, 0.5, 0.5])[:2] == (-1, np.inf) and none.counts == [5, 0, 5, 1]


# ---- hooks ----------------------------------------------------------------------------------------------------------------------

def test_score_dicts_reach_the_evaluator():
    """What ``mesh_scores(search="bvh")`` returns -- the grid's dict with ``fallbacks`` 0 -- is taken by ``Evaluator.add_geometry``,
    and so is ``aligned_scores``'s with its ``alignment``."""
    s = {"accuracy": 0.01, "completeness": 0.03, "chamfer": 0.04, "chamfer_sq": 0.0016, "normal_consistency": 0.9,
         "thresholds": [0.01, 0.02], "precision": [0.5, 1.0], "recall": [0.25, 0.5], "fscore": [1.0 / 3.0, 2.0 / 3.0], "n_pred": 10,
         "n_gt": 10, "fallbacks": 7}
    grid, bvh, aligned = evaluate.Evaluator(4), evaluate.Evaluator(4), evaluate.Evaluator(4)
    grid.add_geometry("a", dict(s, distance="triangle"))
    bvh.add_geometry("a", dict(s, distance="triangle", fallbacks=0))
    aligned.add_geometry("a", dict(s, distance="triangle", fallbacks=0, alignment={"transformation": np.eye(4), "fallbacks": 0}))
    assert grid.summary() == bvh.summary() == aligned.summary() and bvh.summary()["chamfer_mean"] == 0.04
