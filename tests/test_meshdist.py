"""The float64 restatement of include/lara_meshdist.h (tests/meshdist_restate.py) held to closed forms and to an
independent seven-region routine; the host entry -- csrc/tridist.h, the function the kernels run -- held to the restatement; the
restated grid search held to restated brute force on the cases of tests/meshdist_cases.py; the header's constants held to the module's,
the library's refusals, and the hooks into `meshmetrics`, `depthsurface` and the Evaluator -- no GPU.
tests/test_meshdist_gpu.py holds the kernels to the same restatement.

Bars (u = 2^-24, S = the largest coordinate magnitude of the pair): |d - d64| <= 8 u d64 + 2^-40 S.  The host entry works in double
like the restatement, so it sits orders of magnitude inside the bar; the d2 bits are compared too and the outcome is printed."""
import ctypes
import sys

import numpy as np
import pytest
import torch

from lara_amd import evaluate, meshmetrics
from tests import meshdist_cases as C
from tests import meshdist_restate as R

F32 = np.float32


def test_header_constants_equal_the_modules():
    from lara_amd import meshdist
    from tests import test_abi_cpu as abi
    assert (meshdist.RMAX, meshdist.MAX_SPAN, meshdist.MAX_GRID, meshdist.HEADER_INTS) == (4, 4, 256, 4) == \
        (R.RMAX, R.MAX_SPAN, R.MAX_GRID, 4)
    assert (meshdist.HDR_BAD, meshdist.HDR_LARGE, meshdist.HDR_PAIRS, meshdist.HDR_TRIANGLES) == (0, 1, 2, 3)
    text = abi.header_texts()["lara_meshdist.h"]
    for macro, value in (("RMAX", 4), ("MAX_SPAN", 4), ("MAX_GRID", 256), ("HEADER_INTS", 4), ("HDR_BAD", 0), ("HDR_LARGE", 1),
                         ("HDR_PAIRS", 2), ("HDR_TRIANGLES", 3)):
        assert f"#define LARA_MESHDIST_{macro} {value}\n" in text


def test_refusals(hip_lib):
    """T <= 0, T >= 2^28 (in fact from 2^26 on: 64 T pairs are counted in 32 bits), N >= 2^30 and null pointers come back as
    LARA2DGS_E_INVALID (-1) from host code, before any pointer is used; N = 0 is a no-op; python refuses CPU tensors."""
    from lara_amd import meshdist
    for T in (0, -3, 1 << 28, 1 << 26):
        assert hip_lib.lara_meshdist_grid_bytes(T) == -1
        assert hip_lib.lara_meshdist_build(8, T, 1, 1, 1, None) == -1          # (non-null pointers that must not be used)
        assert hip_lib.lara_meshdist_face_normals(8, T, 1, 1, 1, None) == -1
    assert hip_lib.lara_meshdist_grid_bytes((1 << 26) - 1) > 0
    assert hip_lib.lara_meshdist_build(8, 4, None, None, None, None) == -1
    assert hip_lib.lara_meshdist_build(0, 4, 1, 1, 1, None) == -1
    assert hip_lib.lara_meshdist_face_normals(8, 4, None, None, None, None) == -1
    assert hip_lib.lara_meshdist_query_workspace_bytes(1 << 30) == -1 and hip_lib.lara_meshdist_query_workspace_bytes(-1) == -1
    assert hip_lib.lara_meshdist_query_workspace_bytes(0) > 0 and hip_lib.lara_meshdist_query_workspace_bytes(1000) >= 4004
    assert hip_lib.lara_meshdist_query(1 << 30, 1, 1, 1, 1, None, None, 1, None) == -1
    assert hip_lib.lara_meshdist_query(0, None, None, None, None, None, None, None, None) == 0
    assert hip_lib.lara_meshdist_query(5, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshdist_point_triangle_host(-1, None, None, None, None) == -1
    assert hip_lib.lara_meshdist_point_triangle_host(3, None, None, None, None) == -1
    assert hip_lib.lara_meshdist_point_triangle_host(0, None, None, None, None) == 0
    # the stated rules: the grid's resolution, and a size that is a function of T alone within the stated 316 bytes a triangle
    Ts = (1, 4, 5, 63, 257, 1000, 1280, 262144, 262145, 556516)
    assert [hip_lib.lara_meshdist_grid_resolution(t) for t in Ts] == [1, 1, 2, 4, 9, 16, 18, 256, 256, 256] == \
        [R.grid_resolution(t) for t in Ts]
    assert hip_lib.lara_meshdist_grid_resolution(0) == -1
    for t in (1, 1280, 556516):
        cells = R.grid_resolution(t) ** 3
        assert 316 * t + 8 * cells <= hip_lib.lara_meshdist_grid_bytes(t) <= 316 * t + 8 * cells + 4 * cells // 1024 + 4 * t // 1024 + 32768
    V, F = R.icosphere(0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshdist.TriangleGrid(torch.from_numpy(V), torch.from_numpy(F))
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshdist.point_to_mesh(torch.zeros(4, 3), torch.from_numpy(V), torch.from_numpy(F))
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshdist.mesh_scores((torch.from_numpy(V), torch.from_numpy(F)), torch.zeros(4, 3), device="cpu")
    with pytest.raises(ValueError, match="thresholds"):
        meshdist.mesh_scores(torch.zeros(4, 3), torch.zeros(4, 3), thresholds=range(9))


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------

TRI = (np.array([0, 0, 0.0]), np.array([4, 0, 0.0]), np.array([0, 3, 0.0]))          # a 3-4-5 triangle in z = 0


@pytest.mark.parametrize("q, d2, c", [
    ((1, 1, 2), 4.0, (1, 1, 0)),                      # over the interior
    ((1, 1, 0), 0.0, (1, 1, 0)),                      # in the plane, inside
    ((2, -3, 4), 25.0, (2, 0, 0)),                    # over the edge p0 p1
    ((-2, 1, 1), 5.0, (0, 1, 0)),                     # over the edge p2 p0
    ((2 + 3, 1.5 + 4, 0), 25.0, (2, 1.5, 0)),         # over the hypotenuse: 5 along its normal (3, 4) / 5
    ((-1, -2, 2), 9.0, (0, 0, 0)),                    # the vertex regions
    ((6, -1, 0), 5.0, (4, 0, 0)),
    ((-1, 5, -2), 9.0, (0, 3, 0)),
    ((4, 0, 0), 0.0, (4, 0, 0)),                      # at a vertex
    ((2, 0, 0), 0.0, (2, 0, 0)),                      # on an edge
])
def test_restatement_equals_closed_forms(q, d2, c):
    for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)):          # every starting vertex, both windings
        got, cc = R.point_triangle(np.array(q, float), *(TRI[k] for k in perm))
        assert got == d2 and np.array_equal(cc, np.array(c, float)), (perm, got, cc)
        assert np.allclose(R.ericson(q, *(TRI[k] for k in perm)), c, atol=1e-15)


def test_restatement_on_triangles_without_area():
    a, b = np.array([1, 1, 1.0]), np.array([3, 1, 1.0])
    for tri in ((a, b, (a + b) / 2), (a, (a + b) / 2, b), (a, b, a), (a, a, b), (a, b, b), (a, b, a + 2 * (b - a))):
        far = a + 2 * (b - a) if np.array_equal(tri[2], a + 2 * (b - a)) else b
        assert R.point_triangle([2, 4, 1], *tri)[0] == 9.0                                   # over the segment
        assert R.point_triangle([0, 1, 1], *tri)[0] == 1.0                                   # beyond its first end
        d2, c = R.point_triangle(far + [2, 0, 0], *tri)
        assert d2 == 4.0 and np.array_equal(c, far)                                          # beyond its far end
    d2, c = R.point_triangle([1, 3, 1], a, a, a)                                             # a vertex three times: the point
    assert d2 == 4.0 and np.array_equal(c, a)
    assert R.point_triangle(a, a, a, a)[0] == 0.0


def _random_pairs(n, seed):
    """(q, p0, p1, p2) fp32: generic pairs, queries within 2^-20 S of the plane and of an edge, and slivers of aspect 10^6."""
    g = np.random.default_rng(seed)
    tri = (g.random((n, 3, 3)) * 2 - 1) * 10.0 ** g.integers(-3, 4, (n, 1, 1))
    kind = g.integers(0, 4, n)
    sl = kind == 3                                                      # slivers: p2 = a point of p0 p1 + 1e-6 |p0 p1| sideways
    side = np.cross(tri[:, 1] - tri[:, 0], g.normal(size=(n, 3)))
    side *= 1e-6 * np.linalg.norm(tri[:, 1] - tri[:, 0], axis=1, keepdims=True) / np.linalg.norm(side, axis=1, keepdims=True)
    tri[sl, 2] = (tri[sl, 0] + (tri[sl, 1] - tri[sl, 0]) * g.random((sl.sum(), 1))) + side[sl]
    tri = tri.astype(F32)
    t64 = tri.astype(np.float64)
    S = np.abs(t64).max((1, 2))
    b = g.dirichlet(np.ones(3), n)
    q = (b[:, :, None] * t64).sum(1) + g.normal(size=(n, 3)) * S[:, None] * 0.3          # generic (and the slivers')
    nrm = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    near_plane = kind == 1                                                              # inside, 2^-20 S off the plane
    q[near_plane] = ((b[:, :, None] * t64).sum(1) + nrm * (S * 2.0 ** -20 * g.random(n))[:, None])[near_plane]
    near_edge = kind == 2                                                               # 2^-20 S off the edge p0 p1
    e = t64[:, 0] + (t64[:, 1] - t64[:, 0]) * g.random((n, 1))
    q[near_edge] = (e + g.normal(size=(n, 3)) * (S * 2.0 ** -20)[:, None])[near_edge]
    return q.astype(F32), tri[:, 0], tri[:, 1], tri[:, 2]


def test_restatement_equals_the_seven_region_routine():
    """On random pairs (slivers excluded: the seven-region routine's own barycentric form loses digits there) the two closest
    points give the same distance to 1e-12 relative."""
    q, p0, p1, p2 = _random_pairs(3000, 31)
    d2, c = R.point_triangle(q, p0, p1, p2)
    worst = 0.0
    for i in range(len(q)):
        t = [x[i].astype(np.float64) for x in (p0, p1, p2)]
        n = np.cross(t[1] - t[0], t[2] - t[0])
        if np.linalg.norm(n) < 1e-4 * np.linalg.norm(t[1] - t[0]) * np.linalg.norm(t[2] - t[0]):
            continue
        e = R.ericson(q[i].astype(np.float64), *t)
        de = np.linalg.norm(q[i].astype(np.float64) - e)
        S = max(np.abs(q[i]).max(), max(np.abs(x).max() for x in t))
        worst = max(worst, abs(de - np.sqrt(d2[i])) / (1e-12 * max(de, 1e-3 * S)))
        assert np.linalg.norm(c[i] - e) <= 1e-9 * S
    print(f"meshdist restatement vs seven regions: worst {worst:.3f} of 1e-12 relative")
    assert worst <= 1.0


# ---- the host entry (csrc/tridist.h) against the restatement --------------------------------------------------------------------

def _host(hip_lib, q, p0, p1, p2):
    q = np.ascontiguousarray(q, F32)
    t9 = np.ascontiguousarray(np.concatenate([p0, p1, p2], 1), F32)
    d2, c = np.empty(len(q)), np.empty((len(q), 3))
    rc = hip_lib.lara_meshdist_point_triangle_host(len(q), q.ctypes.data, t9.ctypes.data, d2.ctypes.data, c.ctypes.data)
    assert rc == 0
    d2_only = np.empty(len(q))
    assert hip_lib.lara_meshdist_point_triangle_host(len(q), q.ctypes.data, t9.ctypes.data, d2_only.ctypes.data, None) == 0
    assert np.array_equal(d2, d2_only)
    return d2, c


def _hold_host(hip_lib, what, q, p0, p1, p2):
    d2, c = _host(hip_lib, q, p0, p1, p2)
    ref, cref = R.point_triangle(q, p0, p1, p2)
    S = np.maximum(np.abs(q).max(1), np.maximum(np.abs(p0).max(1), np.maximum(np.abs(p1).max(1), np.abs(p2).max(1)))).astype(np.float64)
    d, d64 = np.sqrt(d2), np.sqrt(ref)
    bar = 8 * R.U * d64 + 2.0 ** -40 * S
    ok = bar > 0
    assert np.all(d[~ok] == d64[~ok])
    ratio = float((np.abs(d - d64)[ok] / bar[ok]).max()) if ok.any() else 0.0
    rc = float((np.abs(c - cref).max(1)[ok] / bar[ok]).max()) if ok.any() else 0.0
    equal = int((d2.view(np.int64) == ref.view(np.int64)).sum())
    print(f"meshdist host entry, {what}: distance {ratio:.2e} of the bar, closest point {rc:.2e}; d2 bits equal in {equal} of {len(q)}")
    assert ratio <= 1.0 and rc <= 1.0, (what, ratio, rc)
    assert np.all(d2[ref == 0] == 0)
    return d2, ref


def test_host_entry_equals_the_restatement_on_random_pairs(hip_lib):
    """10^5 pairs: generic ones, queries within 2^-20 S of the plane and of an edge, slivers of aspect 10^6."""
    d2, ref = _hold_host(hip_lib, "10^5 random pairs", *_random_pairs(100000, 32))
    assert np.isfinite(d2).all()


def test_host_entry_equals_the_restatement_on_the_cases(hip_lib):
    """Every case of tests/meshdist_cases.py: each query against its nearest valid triangle and against five others; exact zeros
    where the lattice makes them exact (a query on a vertex, on an edge or inside a face of lattice triangles)."""
    g = np.random.default_rng(33)
    for key, make in sorted(C.CASES.items()):
        Q, V, F = make()
        Q = Q[:: max(1, len(Q) // 256)]
        ok = np.flatnonzero(R.valid_triangles(V, F))
        _, face, _ = R.brute(Q, V, F)
        p = R.corners(V, F)
        ids = np.concatenate([face[:, None], ok[g.integers(0, len(ok), (len(Q), 5))]], 1).ravel()
        qq = np.repeat(Q, 6, axis=0)
        d2, ref = _hold_host(hip_lib, key, qq, p[0][ids], p[1][ids], p[2][ids])
        if key == "cell_faces":
            on_vertex = (Q[:, None, None, :] == np.stack(p, 1)[None]).all(-1).any((1, 2))
            assert on_vertex.sum() > 5 and np.all(d2.reshape(-1, 6)[on_vertex, 0] == 0)
    q = np.array([[1, 1, 0], [2, 0, 0], [4, 0, 0], [0, 0, 0], [2, 1.5, 0]], F32)
    tri = [np.repeat(np.asarray(t, F32)[None], len(q), 0) for t in TRI]
    assert np.all(_host(hip_lib, q, *tri)[0] == 0)


# ---- the restated grid search against restated brute force ----------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(C.CASES))
def test_restated_grid_search_equals_brute_force(key):
    """Identical faces and distances (both sides run the same float64 function and the same tie rule, so nothing is near here),
    the expected fallback pattern, and the figures the caps of the issue rest on: pairs per triangle, the large list."""
    Q, V, F = C.CASES[key]()
    step = max(1, len(Q) // 80)
    Q = Q[::step] if key not in ("sphere_square", "termination") else np.concatenate([Q[:30], Q[-40:]])
    grid = R.Grid(V, F)
    d64, face, _ = R.brute(Q, V, F)
    got = [grid.search(q) for q in Q]
    assert [g[0] for g in got] == face.tolist()
    assert np.array_equal(np.sqrt([g[1] for g in got]), d64)
    fell = sum(g[2] for g in got)
    n_valid = int(grid.ok.sum())
    per_tri = [sum(i in ids for ids in grid.cells.values()) for i in range(0, grid.T, max(1, grid.T // 50))]
    assert max(per_tri, default=0) <= 64
    print(f"meshdist restated grid {key}: R = {grid.R.tolist()}, {grid.pairs / max(n_valid - len(grid.large), 1):.1f} pairs per "
          f"triangle, large list {len(grid.large)}, {fell} of {len(Q)} fell back, {np.mean([g[3] for g in got]):.0f} tests per query")
    if key in C.NEAR_SURFACE:
        assert fell <= C.FALLBACK_CAP * len(Q)
    if key == "inside":
        assert fell == len(Q)
    if key == "sphere_square":
        assert grid.large == [1280, 1281] and set(face[-40:]) <= {1280, 1281}
    if key == "fan":
        assert 64 <= len(grid.large) <= 256
    if key == "termination":
        assert fell == 0 and np.all(face[:7] >= 3) and np.all(face[:7] % 2 == 1)
    if key == "identical":
        assert set(face) == {0}
    if key == "bad_triangles":
        assert n_valid == 60 and not set(face) & set(C.BAD)


def test_a_query_that_is_not_finite_has_no_candidate():
    V, F = R.icosphere(1)
    grid = R.Grid(V, F)
    for q in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]):
        assert grid.search(q)[:3] == (-1, np.inf, False)


# ---- hooks ----------------------------------------------------------------------------------------------------------------------

def test_score_dicts_reach_the_evaluator():
    s = {"accuracy": 0.01, "completeness": 0.03, "chamfer": 0.04, "chamfer_sq": 0.0016, "normal_consistency": 0.9,
         "thresholds": [0.01, 0.02], "precision": [0.5, 1.0], "recall": [0.25, 0.5], "fscore": [1.0 / 3.0, 2.0 / 3.0], "n_pred": 10,
         "n_gt": 10, "fallbacks": 0}
    point, tri = evaluate.Evaluator(4), evaluate.Evaluator(4)
    point.add_geometry("a", s)
    tri.add_geometry("a", dict(s, distance="triangle"))
    assert point.summary() == tri.summary() and "distance" not in tri.summary() and tri.summary()["chamfer_mean"] == 0.04


def test_the_point_path_does_not_touch_meshdist():
    """`surface_scores` and `depth_scores` import `lara_amd.meshdist` only on the "triangle" route (here both routes end at the "no
    CPU path" check, after the import where there is one); any other value is refused."""
    from lara_amd import depthsurface
    V, F = R.icosphere(0)
    mesh = (torch.from_numpy(V), torch.from_numpy(F))
    import lara_amd
    saved = sys.modules.pop("lara_amd.meshdist", None)          # (as in a process that has not imported it yet)
    vars(lara_amd).pop("meshdist", None)
    try:
        for fn in (lambda **kw: meshmetrics.surface_scores(mesh, mesh, n=16, device="cpu", **kw),
                   lambda **kw: depthsurface.depth_scores(mesh, torch.ones(1, 4, 4), torch.ones(1, 4, 4), torch.eye(3)[None],
                                                          torch.eye(4)[None], n=16, **kw)):
            for kw in ({}, {"distance": "point"}):
                with pytest.raises(RuntimeError, match="no CPU path"):
                    fn(**kw)
                assert "lara_amd.meshdist" not in sys.modules
            with pytest.raises(ValueError, match="'point' or 'triangle'"):
                fn(distance="plane")
            assert "lara_amd.meshdist" not in sys.modules
        with pytest.raises(RuntimeError, match="no CPU path"):
            meshmetrics.surface_scores(mesh, mesh, n=16, device="cpu", distance="triangle")
        assert "lara_amd.meshdist" in sys.modules
    finally:
        if saved is not None:
            sys.modules["lara_amd.meshdist"] = lara_amd.meshdist = saved
