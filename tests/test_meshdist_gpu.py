"""csrc/meshdist.hip held to the float64 restatement of its header (tests/meshdist_restate.py): the triangle search against float64
brute force on every case of tests/meshdist_cases.py, exact ties, reproducibility, the closest point, the face normals, the scores
from the device's own samples, and the bench tool at its --quick size.

Bars (u = 2^-24, S = the largest coordinate magnitude among the queries and the mesh).
  distance   |d - d64(query, the face the device chose)| <= 8 u d64 + 2^-40 S: the fp32 rounding of the result with the project's
             usual factor, and a few double roundings of magnitude S for the cancellation in n . (q - p0) near the plane.
  choice     d64(query, chosen face) <= (1 + 8 u) min_t d64(query, t) + 2^-40 S.
  closest    the point is a double result stored as fp32, which moves each coordinate by up to u |c_j|; no bar in units of d can
             hold that when d << S, so the rounding is added: |c_j - c64_j| <= (distance bar) + u |c64_j| per coordinate, and
             | |q - c| - d | <= (distance bar) + sqrt(3) u S.  (The rounding alone can reach this bar: a measured 0.93 of it says that
             the stored point is the correctly rounded double, nothing more.)
  normals    8 u per component.
  fallbacks  at most 1 % of the queries of the near-surface cases (icosphere, UV sphere, sphere + square, fan): beyond it the
             test would exercise the brute-force kernel, not the grid.

Measured on an MI355X (worst |difference| / bar; the tests print them and write test_out/meshdist_parity.txt, kept as
profiles/meshdist_parity.txt): distance 0.12, choice 0.00 (always the float64 nearest face), closest point 0.93, face normals 0.06,
score means at most 0.007, a mesh against itself 0.09 of 8 u S, no fallback in the near-surface cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import meshdist_cases as C
from tests import meshdist_restate as R
from tests import meshmetrics_restate as MR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8 * R.U
_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))
    out = os.path.join(ROOT, "test_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "meshdist_parity.txt"), "w") as f:
        f.write("worst observed |difference| / bar of tests/test_meshdist_gpu.py (bar = 1 fails; a share: of its 1 % cap)\n")
        for k in sorted(_worst):
            f.write(f"{k}: {_worst[k]:.4f}\n")
    print(f"meshdist parity {key}: {ratio:.4f} of the bar")


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the search ---------------------------------------------------------------------------------------------------------------

_runs = {}


def _case(key):
    """One device run of the case and its float64 brute force, shared by the tests."""
    if key not in _runs:
        from lara_amd import meshdist
        Q, V, F = C.CASES[key]()
        grid = meshdist.TriangleGrid(_t(V), _t(F))
        d, face, closest, fb = grid.query(_t(Q), return_closest=True, return_fallbacks=True)
        _runs[key] = {"Q": Q, "V": V, "F": F, "grid": grid, "d": d.cpu().numpy().astype(np.float64),
                      "face": face.cpu().numpy().astype(np.int64), "closest": closest.cpu().numpy().astype(np.float64),
                      "fallbacks": int(fb.item()), "counts": grid.counts.cpu().numpy(), "brute": R.brute(Q, V, F)}
    return _runs[key]


@pytest.mark.parametrize("key", sorted(C.CASES))
def test_query_equals_float64_brute_force(hip_lib, key):
    r = _case(key)
    Q, V, F, d, face = r["Q"], r["V"], r["F"], r["d"], r["face"]
    d64_min, face64, d2_all = r["brute"]
    bad, n_large, pairs, T = (int(x) for x in r["counts"])
    print(f"meshdist {key}: T = {T}, {r['fallbacks']} of {len(Q)} queries fell back, large list {n_large}, {pairs} pairs, {bad} refused")
    assert T == len(F) and bad == int((~R.valid_triangles(V, F)).sum()) and 0 <= pairs <= 64 * T
    r_dist, r_choice = C.check_against_brute_force(key, Q, V, F, d, face, d64_min, d2_all)
    _note("distance", r_dist)
    _note("choice", r_choice)
    assert r_dist <= 1.0 and r_choice <= 1.0, (key, r_dist, r_choice)
    if key in C.NEAR_SURFACE:
        _note("fallback share of the near-surface cases", r["fallbacks"] / len(Q) / C.FALLBACK_CAP)
        assert r["fallbacks"] <= C.FALLBACK_CAP * len(Q), (key, r["fallbacks"])
    if key == "inside":
        assert r["fallbacks"] > len(Q) // 2
    if key == "sphere_square":
        assert n_large == 2 and set(face[-257:]) <= {1280, 1281} and np.array_equal(face[-257:], face64[-257:])
    if key == "fan":
        assert n_large == len(R.Grid(V, F).large) == 120
    if key == "termination":         # the face beyond the ring that first held a candidate
        assert np.array_equal(face, face64) and np.all(face[:7] >= 3) and np.all(face[:7] % 2 == 1)
    if key == "identical":
        assert np.all(face == 0)
    if key == "bad_triangles":
        assert bad == 3 and not set(face) & set(C.BAD)
    if key == "one_triangle":        # the seven regions, closed forms: three heights over the interior point, and the vertices
        assert np.all(face == 0) and d[0] == 0 and d[7] == 0.5 and d[14] == 2.0 and np.all(d[21:24] == 0)
    if key == "cell_faces":          # lattice queries that are vertices: exactly 0
        on_vertex = (Q[:, None, :] == V[None]).all(-1).any(1)
        assert on_vertex.sum() > 5 and np.all(d[on_vertex] == 0)


def test_closest_point(hip_lib):
    worst_c = worst_d = 0.0
    for key in sorted(C.CASES):
        r = _case(key)
        Q, V, F, d, face, c = r["Q"], r["V"], r["F"], r["d"], r["face"], r["closest"]
        p = R.corners(V, F)
        d2, c64 = R.point_triangle(Q, p[0][face], p[1][face], p[2][face])
        S = R.scale(Q, V, F)
        bar = BAR * np.sqrt(d2) + 2.0 ** -40 * S
        worst_c = max(worst_c, float((np.abs(c - c64) / (bar[:, None] + R.U * np.abs(c64))).max()))
        again = np.sqrt(((Q.astype(np.float64) - c) ** 2).sum(1))
        worst_d = max(worst_d, float((np.abs(again - d) / (bar + np.sqrt(3.0) * R.U * S)).max()))
    _note("closest point", worst_c)
    _note("closest point reproduces the distance", worst_d)
    assert worst_c <= 1.0 and worst_d <= 1.0


def test_exact_ties_go_to_the_smaller_face(hip_lib):
    """Lattice data: coordinates, differences and products are exact in fp32 and double alike, so ties are exact in both.  A fan of
    eight triangles around the origin with rim vertices on the integer lattice; queries straight above the shared vertex (all
    eight tie), above the shared edges (two tie) and above interiors.  The face is the smallest id attaining the float64 minimum."""
    from lara_amd import meshdist
    rim = [[2, 0], [2, 2], [0, 2], [-2, 2], [-2, 0], [-2, -2], [0, -2], [2, -2]]
    V = np.array([[0, 0, 0]] + [[x, y, 0] for x, y in rim], np.float32)
    F = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], np.int64)
    Q = [[0, 0, z] for z in (0.0, 1.0, -3.0)] + [[x / 2, y / 2, z] for x, y in rim for z in (0.0, 2.0)]
    Q += [[1.5, 0.5, 1.0], [-0.5, 1.5, 4.0], [4, 0, 0], [4, 4, 1], [0, -8, 2]]
    Q = np.array(Q, np.float32)
    for order in (np.arange(8), np.arange(8)[::-1].copy(), np.array([3, 7, 0, 5, 2, 6, 1, 4])):
        d, face = meshdist.point_to_mesh(_t(Q), _t(V), _t(F[order]))
        d64, face64, d2_all = R.brute(Q, V, F[order])
        ties = (d2_all == d2_all.min(1, keepdims=True)).sum(1)
        assert ties[0] == 8 and ties[1] == 8 and ties[3] == 2 and ties.max() == 8
        assert np.array_equal(face.cpu().numpy(), face64)
        assert np.array_equal(d.cpu().numpy().astype(np.float64), d64.astype(np.float32).astype(np.float64))
    r = _case("identical")
    assert np.all(r["face"] == 0)


def test_query_is_reproducible_and_follows_a_permutation(hip_lib):
    from lara_amd import meshdist
    V, F = R.icosphere(3)
    F = np.concatenate([F[:1279], F[100:101]])                 # two identical triangles: exact ties
    Q = R.rippled_sphere_points(4096, 41)
    q, v = _t(Q), _t(V)
    grid = meshdist.TriangleGrid(v, _t(F))
    d1, f1, c1 = grid.query(q, return_closest=True)
    d2, f2, c2 = grid.query(q, return_closest=True)
    assert torch.equal(_bits(d1), _bits(d2)) and torch.equal(f1, f2) and torch.equal(_bits(c1), _bits(c2))
    again = meshdist.TriangleGrid(v, _t(F))                    # another build: another order inside the cells
    d3, f3 = again.query(q)
    assert torch.equal(_bits(d1), _bits(d3)) and torch.equal(f1, f3)
    perm = np.random.default_rng(42).permutation(len(F))
    d4, f4 = meshdist.point_to_mesh(q, v, _t(F[perm]))
    assert torch.equal(_bits(d1), _bits(d4))
    back, f1h = perm[f4.cpu().numpy()], f1.cpu().numpy()
    moved = back != f1h
    d2_all = R.all_d2(Q[moved], V, F)
    k = np.arange(moved.sum())
    assert np.all(d2_all[k, back[moved]] == d2_all[k, f1h[moved]])          # only where the minimum is not unique
    assert np.all(f1h != 1279)                                               # of the identical pair, the smaller id
    # the same bits on a side stream.  torch hands streams out of a pool of 32 in turn, and which of them a LATER test gets decides
    # which hardware queue its work shares (tests/test_stream_safety_gpu.py needs a side stream that does not queue behind the
    # caller's): a whole turn of the pool is taken here, so that every test after this one is handed the stream it would be without it
    torch.cuda.synchronize()
    side = [torch.cuda.Stream(device=_dev()) for _ in range(32)][0]
    with torch.cuda.stream(side):
        d5, f5 = meshdist.TriangleGrid(v, _t(F)).query(q)
    side.synchronize()
    assert torch.equal(_bits(d1), _bits(d5)) and torch.equal(f1, f5)


def test_queries_and_meshes_without_a_candidate(hip_lib):
    """The stated rules: a query with a coordinate that is not finite, and a mesh with no valid triangle, give face -1, dist +inf,
    closest NaN; N = 0 is a no-op."""
    from lara_amd import meshdist
    V, F = R.icosphere(1)
    grid = meshdist.TriangleGrid(_t(V), _t(F))
    Q = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.5, 0.5, 0.5], [np.nan, np.nan, np.nan]], np.float32)
    d, face, c, fb = grid.query(_t(Q), return_closest=True, return_fallbacks=True)
    d, face, c = d.cpu().numpy(), face.cpu().numpy(), c.cpu().numpy()
    assert face.tolist()[:3] == [-1, -1, -1] and face[4] == -1 and face[3] >= 0 and np.isfinite(d[3]) and np.isfinite(c[3]).all()
    assert np.all(np.isposinf(d[[0, 1, 2, 4]])) and np.isnan(c[[0, 1, 2, 4]]).all() and int(fb.item()) == 0
    none = meshdist.TriangleGrid(_t(V), _t(np.full((5, 3), len(V) + 1, np.int64)))
    d, face, c = none.query(_t(Q[3:4]), return_closest=True)
    assert face.item() == -1 and np.isposinf(d.item()) and bool(torch.isnan(c).all()) and none.counts.cpu().tolist() == [5, 0, 0, 5]
    d, face = grid.query(_t(Q[:0]))
    assert d.shape == (0,) and face.shape == (0,)
    with pytest.raises(ValueError):
        meshdist.TriangleGrid(_t(V), _t(F[:0]))


def test_face_normals(hip_lib):
    worst = 0.0
    for key in ("icosphere", "degenerate", "bad_triangles", "fan"):
        r = _case(key)
        got = r["grid"].face_normals.cpu().numpy().astype(np.float64)
        ref = R.face_normals(r["V"], r["F"])
        sound = np.isfinite(ref).all(1)          # (a NaN vertex: whatever the quotient gives or zero; never read, the face is no candidate)
        worst = max(worst, float(np.abs(got - ref)[sound].max() / BAR))
        assert np.all(got[(ref == 0).all(1)] == 0)
    _note("face normals", worst)
    assert worst <= 1.0


# ---- scores -------------------------------------------------------------------------------------------------------------------

THR = (0.01, 0.02, 0.03, 0.05)


def _check_scores(out, pred, gt, thresholds):
    """``out`` against the restatement computed from the device's own samples; a side is (V, F) or None for a point set."""
    P, Pn, G, Gn, d_p, i_p, d_g, i_g = [None if t is None else t.cpu().numpy() for t in out["samples"]]

    def direction(Q, side, points, normals):
        if side is None:
            d, i = MR.nearest(Q, points)
            return (d, i), normals
        d, i, _ = R.brute(Q, *side)
        return (d, i), R.face_normals(*side)
    near_p, nt_p = direction(P, gt, G, Gn)
    near_g, nt_g = direction(G, pred, P, Pn)
    ref = R.scores(P, Pn, G, Gn, near_p, near_g, nt_p, nt_g, thresholds)
    S = max(float(np.abs(P).max()), float(np.abs(G).max()))
    for k in ("accuracy", "completeness", "chamfer") + (("normal_consistency",) if ref["normal_consistency"] is not None else ()):
        ratio = abs(out[k] - ref[k]) / (BAR * abs(ref[k]) + 2.0 ** -40 * S)
        _note("scores " + k, ratio)
        assert ratio <= 1.0, (k, out[k], ref[k])
    for side, (d64, _), n in (("precision", near_p, len(P)), ("recall", near_g, len(G))):
        for t, got in zip(thresholds, out[side]):
            t32 = float(np.float32(t))
            lo = int((d64 <= t32 * (1 - BAR) - 2.0 ** -40 * S).sum())
            hi = int((d64 <= t32 * (1 + BAR) + 2.0 ** -40 * S).sum())
            assert lo <= round(got * n) <= hi and abs(got * n - round(got * n)) < 1e-6, (side, t, got * n, lo, hi)
    for p, r, f in zip(out["precision"], out["recall"], out["fscore"]):
        assert f == (2.0 * p * r / (p + r) if p + r > 0 else 0.0)
    return ref


def test_scores_equal_the_restatement_from_the_devices_samples(hip_lib):
    from lara_amd import meshdist, meshmetrics
    V, F = MR.uv_sphere()
    Vp = V * np.float32(1.02)
    pred, gt = (_t(Vp), _t(F)), (_t(V), _t(F), None)          # (a read_obj mesh carries a third entry)
    out = meshdist.mesh_scores(pred, gt, n=4096, thresholds=THR, seed=0, return_samples=True)
    ref = _check_scores(out, (Vp, F), (V, F), THR)
    assert out["distance"] == "triangle" and out["n_pred"] == out["n_gt"] == 4096 and out["normal_consistency"] > 0.99
    assert 0.005 < out["accuracy"] < 0.03 and out["fscore"][-1] == 1.0 == ref["fscore"][-1]
    # a second call, and the keyword of surface_scores: the same bits
    for again in (meshdist.mesh_scores(pred, gt, n=4096, thresholds=THR, seed=0),
                  meshmetrics.surface_scores(pred, gt, n=4096, thresholds=THR, seed=0, distance="triangle")):
        assert {k: v for k, v in out.items() if k != "samples"} == again
    # the samples are those of the point mode, and its dict has the same keys but "distance"
    point = meshmetrics.surface_scores(pred, gt, n=4096, thresholds=THR, seed=0, return_samples=True)
    assert set(point) == set(out) - {"distance"}
    for a, b in zip(point["samples"][:4], out["samples"][:4]):
        assert torch.equal(_bits(a), _bits(b))
    # a side given as points is measured point-to-point, the mesh side against its triangles
    mixed = meshdist.mesh_scores(pred, (out["samples"][2], out["samples"][3]), n=4096, thresholds=THR, return_samples=True)
    _check_scores(mixed, (Vp, F), None, THR)
    assert mixed["accuracy"] == point["accuracy"] and mixed["completeness"] == out["completeness"]


def test_a_mesh_against_itself(hip_lib):
    """Every sample is a point of its own mesh rounded to fp32, at most sqrt(3) u S off its face: every distance is <= 8 u S.  The
    same call in point mode measures the spacing of the other side's samples instead: orders of magnitude more."""
    from lara_amd import meshmetrics
    V, F = R.icosphere(3)
    mesh = (_t(V), _t(F))
    S = float(np.abs(V).max())
    tri = meshmetrics.surface_scores(mesh, mesh, n=4096, thresholds=(1e-6,), seed=1, distance="triangle", return_samples=True)
    d_p, d_g = tri["samples"][4], tri["samples"][6]
    worst = max(float(d_p.max()), float(d_g.max())) / (BAR * S)
    _note("self distance", worst)
    assert worst <= 1.0 and tri["fscore"] == [1.0] and tri["fallbacks"] == 0 and abs(tri["normal_consistency"] - 1.0) < 1e-3
    # other samples of the same mesh, point mode: the sample spacing
    a = meshmetrics.sample_surface(*mesh, 4096, seed=2)
    point = meshmetrics.surface_scores((a[0], a[1]), mesh, n=4096, seed=1)
    exact = meshmetrics.surface_scores((a[0], a[1]), mesh, n=4096, seed=1, distance="triangle", return_samples=True)
    print(f"meshdist self distance: accuracy {exact['accuracy']:.3e} (triangle) against {point['accuracy']:.3e} (point)")
    assert exact["accuracy"] <= BAR * S and point["accuracy"] > 100 * max(exact["accuracy"], BAR * S)
    # on one set of predicted samples: the ground truth's samples lie on its mesh, so the triangle distance is never larger
    d_tri = exact["samples"][4].cpu().numpy().astype(np.float64)
    d_pt, _ = meshmetrics.nearest(a[0], exact["samples"][2])
    assert np.all(d_tri <= d_pt.cpu().numpy().astype(np.float64) * (1 + BAR) + BAR * S)


def test_triangle_distances_never_exceed_point_distances(hip_lib):
    from lara_amd import meshmetrics
    V, F = MR.uv_sphere()
    pred, gt = (_t(V * np.float32(1.02)), _t(F)), (_t(V), _t(F))
    S = 1.02
    tri = meshmetrics.surface_scores(pred, gt, n=4096, distance="triangle", return_samples=True)
    pt = meshmetrics.surface_scores(pred, gt, n=4096, return_samples=True)
    for k in (4, 6):
        assert np.all(tri["samples"][k].cpu().numpy().astype(np.float64) <= pt["samples"][k].cpu().numpy().astype(np.float64) * (1 + BAR) + BAR * S)
    assert tri["accuracy"] < pt["accuracy"] and tri["completeness"] < pt["completeness"]


def test_unit_sphere_points_against_the_inscribed_icosphere(hip_lib):
    """A face of the inscribed mesh lies in the plane at distance |n . p0| from the centre, and every point of the unit sphere is
    within 1 - min_face |n . p0| of the mesh (the mesh separates the sphere from the ball of that radius)."""
    from lara_amd import meshdist
    V, F = R.icosphere(3)
    g = np.random.default_rng(43)
    Q = g.normal(size=(4096, 3))
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    d, face, fb = meshdist.point_to_mesh(_t(Q), _t(V), _t(F), return_fallbacks=True)
    inner = np.abs((R.face_normals(V, F) * V[F[:, 0]].astype(np.float64)).sum(1)).min()
    assert 0.99 < inner < 1.0 and float(d.max()) <= 1.0 - inner + BAR and int(fb.item()) == 0 and float(d.max()) > 0.2 * (1.0 - inner)


def test_depth_scores_with_triangle_distances(hip_lib):
    """The scene of tests/depthsurface_cases.py: the ground truth is a point cloud, so accuracy stays sample-to-point (the same
    bits) and completeness, ground-truth points against the predicted mesh's triangles, can only fall."""
    from lara_amd import depthsurface
    from tests import depthsurface_cases as DC
    c = DC.sphere4()
    V, F, _ = DC.nested_spheres()
    pred = (_t(V), _t(F))
    views = (_t(c["depth"]), _t(c["mask"]), c["ixt"], c["c2w"])
    point = depthsurface.depth_scores(pred, *views, n=8192, return_samples=True)
    tri = depthsurface.depth_scores(pred, *views, n=8192, distance="triangle", return_samples=True)
    assert tri["distance"] == "triangle" and set(tri) == set(point) | {"distance"}
    assert tri["accuracy"] == point["accuracy"] and tri["precision"] == point["precision"] and tri["n_gt"] == point["n_gt"]
    assert torch.equal(_bits(tri["samples"][4]), _bits(point["samples"][4])) and torch.equal(tri["samples"][5], point["samples"][5])
    assert 0 < tri["completeness"] <= point["completeness"] and all(a >= b for a, b in zip(tri["recall"], point["recall"]))
    d_t, d_p = tri["samples"][6].cpu().numpy().astype(np.float64), point["samples"][6].cpu().numpy().astype(np.float64)
    assert np.all(d_t <= d_p * (1 + BAR) + BAR * float(np.abs(V).max()))
    # held to float64 brute force on a part of the ground-truth points
    G = tri["samples"][2].cpu().numpy()[::37]
    d64, _, _ = R.brute(G, V, F)
    assert np.all(np.abs(d_t[::37] - d64) <= BAR * d64 + 2.0 ** -40 * R.scale(G, V, F))
    assert tri["normal_consistency"] is not None and 0 < tri["normal_consistency"] <= 1.0
    # a prediction given as points has no triangles: as in point mode
    pts = depthsurface.depth_scores((point["samples"][0], point["samples"][1]), *views, distance="triangle")
    assert pts["completeness"] == point["completeness"] and pts["accuracy"] == point["accuracy"]


def test_bench_tool_runs_at_its_quick_size(hip_lib, tmp_path):
    out = tmp_path / "bench.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "meshdist_bench.py"), "--quick", "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(run.stdout.strip().splitlines()[-1]) == res
    assert res["T"] <= 20000 and res["build_ms"] > 0 and 0 <= res["large_list"] <= res["T"] // 100 and 1 <= res["pairs_per_triangle"] <= 64
    for q in res["queries"]:
        assert q["query_ms"] > 0 and 0.0 <= q["fallback_share"] <= 0.01 and q["mean_distance"] > 0
    assert res["brute_force"]["ms"] > 0 and res["torch_operators"]["worst_difference"] <= 1e-5
    rows = {r["pair"]: r for r in res["accuracy_table"]}
    assert rows["input against itself"]["triangle"]["chamfer"] < 1e-6 < rows["input against itself"]["point"]["chamfer"]
    assert all(r["triangle"]["chamfer"] <= r["point"]["chamfer"] for r in rows.values())
