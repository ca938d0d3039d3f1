"""csrc/meshmetrics.hip held to the float64 / integer restatement of its header (tests/meshmetrics_restate.py): the sampler from the
device's own integers, the nearest-neighbour search against float64 brute force on every case of the issue, the scores from the
device's own samples, reproducibility, and the bench tool at its --quick size.

Bars, from the roundings (u = 2^-24).  Nearest: the three fp32 differences are rounded once each and the squares and sums add a few
ulps, so |dist - d64(query, index)| <= 8 u d64 and d64(query, index) <= d64_min (1 + 8 u): a near-tie may resolve either way, no
case is excluded.  Sampler: the points are float64 results rounded once, held to 8 u max|coordinate| (8 u for the normals).
Scores: means within 8 u relative; threshold counts between the float64 counts at t (1 -+ 8 u).

Measured on an MI355X (worst |diff| / bar over all cases; the tests print them and write test_out/meshmetrics_parity.txt, kept as
profiles/meshmetrics_parity.txt): nearest distance 0.23, nearest choice 0.00 (always the float64 nearest target), sampler points
0.08, normals 0.06, score means at most 0.002."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import meshmetrics_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8 * R.U
_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))
    out = os.path.join(ROOT, "test_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "meshmetrics_parity.txt"), "w") as f:
        f.write("worst observed |difference| / bar of tests/test_meshmetrics_gpu.py (bar = 1 fails)\n")
        for k in sorted(_worst):
            f.write(f"{k}: {_worst[k]:.4f}\n")
    print(f"meshmetrics parity {key}: {ratio:.4f} of the bar")


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), dtype)


# ---- sampler ------------------------------------------------------------------------------------------------------------------

def _mesh_ratio():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [0, 0, 1]], np.float32)
    return V, np.array([[0, 1, 2], [0, 3, 4]], np.int64)


def _mesh_degenerate():
    """The cube, a degenerate triangle in the middle of the list and a tiny one (legs 1e-6: area 5e-13 < 2^-36) at its end."""
    V, F = R.cube()
    V = np.concatenate([V, np.array([[1e-6, 0, 0], [0, 1e-6, 0]], np.float32)])
    F = np.concatenate([F[:5], [[2, 2, 7]], F[5:], [[0, 8, 9]]])
    return V, F


SAMPLER_MESHES = {"ratio_1_3": _mesh_ratio, "cube": R.cube, "degenerate": _mesh_degenerate, "sphere": R.uv_sphere}


@pytest.mark.parametrize("n", [1, 63, 64, 257, 4096])
@pytest.mark.parametrize("key", sorted(SAMPLER_MESHES))
def test_sampler_equals_the_restatement(hip_lib, key, n):
    from lara_amd import meshmetrics
    V, F = SAMPLER_MESHES[key]()
    v, f = _t(V), _t(F)
    pts, nrm, face, q, s = meshmetrics.sample_surface(v, f, n, seed=5, return_quantised=True)
    q_h, face_h = q.cpu().numpy(), face.cpu().numpy().astype(np.int64)
    A = R.areas(V, F)
    assert s == R.scale_exp(A.sum())
    assert np.all(np.abs(q_h - R.quantise(A, s)) <= 1) and q_h.sum() < 2 ** 40
    if key == "ratio_1_3":
        assert q_h.tolist() == [2 ** 36, 3 * 2 ** 36]
    if key == "degenerate":
        assert q_h[5] == 0 and q_h[-1] == 0 and not np.isin(face_h, [5, len(F) - 1]).any()
    # given the device's q the faces are the integer rule, exactly
    assert np.array_equal(face_h, R.faces_from_q(q_h, n))
    ref_p, ref_n = R.points_on_faces(V, F, face_h, 5)
    scale = float(np.abs(V).max())
    rp = np.abs(pts.cpu().numpy().astype(np.float64) - ref_p).max() / (BAR * scale)
    rn = np.abs(nrm.cpu().numpy().astype(np.float64) - ref_n).max() / BAR
    _note("sampler points", rp)
    _note("sampler normals", rn)
    assert rp <= 1.0 and rn <= 1.0
    # two calls: the same bits; another seed: other points, the same faces
    pts2, nrm2, face2 = meshmetrics.sample_surface(v, f, n, seed=5)
    assert torch.equal(pts, pts2) and torch.equal(nrm, nrm2) and torch.equal(face, face2)
    pts3, _, face3 = meshmetrics.sample_surface(v, f, n, seed=6)
    assert torch.equal(face, face3) and not torch.equal(pts, pts3)


def test_sampler_refuses_what_it_cannot_sample(hip_lib):
    from lara_amd import meshmetrics
    V, F = R.cube()
    v, f = _t(V), _t(F)
    with pytest.raises(ValueError):
        meshmetrics.sample_surface(v, f[:0], 16)
    with pytest.raises(ValueError):
        meshmetrics.sample_surface(v, f, (1 << 22) + 1)
    with pytest.raises(RuntimeError, match="invalid argument"):          # no area at all: S = 0
        meshmetrics.sample_surface(v, torch.zeros(3, 3, dtype=torch.int64, device=_dev()), 16)
    with pytest.raises(RuntimeError, match="invalid argument"):          # an index outside [0, Nv)
        meshmetrics.sample_surface(v, _t(np.array([[0, 1, 8]])), 16)
    with pytest.raises(ValueError):
        meshmetrics.nearest(v, v[:0])
    d, i = meshmetrics.nearest(v[:0], v)
    assert d.shape == (0,) and i.shape == (0,)


# ---- nearest ------------------------------------------------------------------------------------------------------------------

def _rng(seed):
    return np.random.default_rng(seed)


def case_random(N, M, seed):
    g = _rng(seed)
    return g.random((N, 3), np.float32), g.random((M, 3), np.float32)


def case_one_cell():
    """All but one of 257 targets inside one cell (a 1e-3 cluster at the origin; the last one spans the box)."""
    g = _rng(10)
    P = np.concatenate([g.random((256, 3), np.float32) * 1e-3, np.ones((1, 3), np.float32)])
    return g.random((63, 3), np.float32), P


def case_flat_cluster():
    """Every target in the ONE cell of a one-cell grid: 1000 copies of one point (the box has no extent: h = 1, R = 1)."""
    g = _rng(11)
    P = np.zeros((1000, 3), np.float32)
    P[:, 0] = 0.25
    P[:, 1] = -3.0
    return g.random((257, 3), np.float32) * 4 - 2, P


def case_single_target():
    g = _rng(12)
    return g.random((257, 3), np.float32) * 2 - 1, np.array([[0.3, -0.2, 0.9]], np.float32)


def case_cell_faces():
    """1000 targets on the lattice i / 16 (R = 16 over [0, 1]^3: every target on a cell face, some on the box's maximum corner,
    many duplicates); queries: random, lattice points themselves, and cell centres (equidistant from eight corners)."""
    g = _rng(13)
    P = g.integers(0, 17, (1000, 3)).astype(np.float32) / 16
    P[:3] = [[0, 0, 0], [1, 1, 1], [1, 1, 1]]
    Q = np.concatenate([g.random((129, 3), np.float32), P[g.integers(0, 1000, 64)],
                        (g.integers(0, 16, (64, 3)).astype(np.float32) + 0.5) / 16])
    return Q, P


def case_duplicates():
    """Every target twice (500 + 500); queries equal to targets: d = 0 exactly, the smaller index."""
    g = _rng(14)
    half = g.random((500, 3), np.float32)
    P = np.concatenate([half, half])
    return np.concatenate([half[g.integers(0, 500, 200)], g.random((57, 3), np.float32)]), P


def case_outside():
    """Queries outside the box on every side, near and 10 x the extent away, along axes and diagonals."""
    g = _rng(15)
    P = g.random((1000, 3), np.float32)
    Q = []
    for axis in range(3):
        for side in (-1, 1):
            for far in (0.01, 0.5, 10.0):
                q = g.random(3).astype(np.float32)
                q[axis] = 1 + far if side > 0 else -far
                Q.append(q)
    for sign in ((1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1)):
        for far in (0.1, 10.0):
            Q.append(np.array([(1 + far) if s > 0 else -far for s in sign], np.float32))
    Q = np.array(Q, np.float32)
    return np.concatenate([Q, g.random((63 - len(Q), 3), np.float32) * 30 - 15]), P


def case_fallback():
    """Two small clusters in opposite corners, the queries in the empty middle: more than half must take the brute-force route."""
    g = _rng(16)
    P = np.concatenate([g.random((500, 3), np.float32) * 0.02, 1 - g.random((500, 3), np.float32) * 0.02])
    return (0.4 + 0.2 * g.random((257, 3), np.float32)).astype(np.float32), P


def case_termination():
    """R = 16 over [0, 1]^3 (h = 1/16).  Each query sits near a corner of its cell; its own cell (ring r = 0) holds a target at
    the far corner, 1.4 h away, and the true neighbour lies 0.26 h away in the DIAGONAL cell of ring 1 (or, for the second half, in
    the edge-diagonal cell): stopping at the first ring that holds a candidate returns the wrong one.  A third group: ring 1 holds
    a candidate 2.5 h away in its corner cell while the neighbour lies 1.55 h away in a cell of ring 2."""
    g = _rng(17)
    h = 1.0 / 16
    Q, P = [], [[0, 0, 0], [1, 1, 1]]
    cells = [(8, 8, 8), (3, 12, 5), (12, 4, 10), (5, 5, 13), (10, 10, 2), (13, 7, 7), (6, 2, 9)]
    for k, (cx, cy, cz) in enumerate(cells):
        c = np.array([cx, cy, cz], np.float64)
        j = g.random(3) * 0.02
        if k % 3 == 0:
            Q.append((c + 0.9 + j) * h); P.append((c + 0.1) * h); P.append((c + 1.05) * h)
        elif k % 3 == 1:
            Q.append((c + [0.9, 0.9, 0.5] + j) * h); P.append((c + [0.1, 0.1, 0.5]) * h); P.append((c + [1.05, 1.05, 0.5]) * h)
        else:
            Q.append((c + 0.5 + j) * h); P.append((c - 0.95) * h); P.append((c + [2.05, 0.5, 0.5]) * h)
    Q, P = np.array(Q, np.float32), np.array(P, np.float32)
    filler = g.random((1000 - len(P), 3), np.float32) * np.float32([0.08, 1, 1])          # far away: x < 0.08
    return np.concatenate([Q] * 9)[:63], np.concatenate([P, filler])


NEAREST_CASES = {
    "random_1_4096": lambda: case_random(1, 4096, 1), "random_63_1000": lambda: case_random(63, 1000, 2),
    "random_257_257": lambda: case_random(257, 257, 3), "random_1000_63": lambda: case_random(1000, 63, 4),
    "random_4096_1": lambda: case_random(4096, 1, 5), "random_4096_4096": lambda: case_random(4096, 4096, 6),
    "random_1000_4096": lambda: case_random(1000, 4096, 7), "random_1_1": lambda: case_random(1, 1, 8),
    "one_cell": case_one_cell, "flat_cluster": case_flat_cluster, "single_target": case_single_target,
    "cell_faces": case_cell_faces, "duplicates": case_duplicates, "outside": case_outside, "fallback": case_fallback,
    "termination": case_termination,
}
_near = {}


def _nearest_case(key):
    """One device run of the case and its float64 brute force, shared by the tests."""
    if key not in _near:
        from lara_amd import meshmetrics
        Q, P = NEAREST_CASES[key]()
        d, i, fb = meshmetrics.nearest(_t(Q), _t(P), return_fallbacks=True)
        _near[key] = (Q, P, d.cpu().numpy(), i.cpu().numpy().astype(np.int64), int(fb.item()), R.nearest(Q, P))
    return _near[key]


@pytest.mark.parametrize("key", sorted(NEAREST_CASES))
def test_nearest_equals_float64_brute_force(hip_lib, key):
    Q, P, d, i, fallbacks, (d64_min, i64) = _nearest_case(key)
    assert Q.shape[0] in (1, 63, 257, 1000, 4096) and P.shape[0] in (1, 63, 257, 1000, 4096)
    assert np.all((i >= 0) & (i < len(P)))
    d64 = R.distances_to(Q, P, i)
    zero = d64 == 0
    assert np.all(d[zero] == 0)
    r_dist = (np.abs(d.astype(np.float64) - d64)[~zero] / (BAR * d64[~zero])).max() if (~zero).any() else 0.0
    pos = d64_min > 0
    assert np.all(d64[~pos] == 0)
    r_near = ((d64[pos] / d64_min[pos] - 1.0) / BAR).max() if pos.any() else 0.0
    _note("nearest distance", r_dist)
    _note("nearest choice", r_near)
    assert r_dist <= 1.0 and r_near <= 1.0, (key, r_dist, r_near)
    print(f"meshmetrics nearest {key}: {fallbacks} of {len(Q)} queries fell back")
    if key == "fallback":
        assert fallbacks > len(Q) // 2
    if key == "duplicates":          # d = 0 exactly, and the smaller of the two equal targets
        assert np.all(d[:200] == 0) and np.array_equal(i[:200], i64[:200]) and np.all(i[:200] < 500)
    if key == "termination":         # the neighbour beyond the ring that first held a candidate
        assert np.array_equal(i, i64) and np.all(i[:7] >= 2) and np.all((i[:7] - 2) % 2 == 1)
    if key == "flat_cluster":        # a thousand identical targets: index 0
        assert np.all(i == 0)


def test_exact_ties_go_to_the_smaller_index(hip_lib):
    """Lattice data: coordinates and differences are exact in fp32 and float64 alike, so ties are exact in both and the device's
    choice must be the restatement's first minimum."""
    Q, P, d, i, _, (d64_min, i64) = _nearest_case("cell_faces")
    lattice = slice(129, 257)          # the queries that are lattice points or cell centres
    assert np.array_equal(i[lattice], i64[lattice])
    assert np.array_equal(d[lattice].astype(np.float64), d64_min[lattice].astype(np.float32).astype(np.float64))


def test_nearest_is_reproducible_and_follows_a_permutation(hip_lib):
    from lara_amd import meshmetrics
    Q, P = case_random(4096, 4096, 21)
    P[100:200] = P[300:400]                                   # exact ties among the targets
    q, p = _t(Q), _t(P)
    d1, i1 = meshmetrics.nearest(q, p)
    d2, i2 = meshmetrics.nearest(q, p)
    assert torch.equal(d1, d2) and torch.equal(i1, i2)
    perm = _rng(22).permutation(len(P))
    d3, i3 = meshmetrics.nearest(q, _t(P[perm]))
    assert torch.equal(d1, d3)
    back = perm[i3.cpu().numpy()]
    i1h = i1.cpu().numpy()
    moved = back != i1h
    assert np.all(P[back[moved]] == P[i1h[moved]])            # only among identical targets
    assert moved.sum() <= 200


# ---- scores -------------------------------------------------------------------------------------------------------------------

THR = (0.01, 0.02, 0.03, 0.05)


def _check_scores(out, thresholds):
    P, Pn, G, Gn, d_p, i_p, d_g, i_g = [None if t is None else t.cpu().numpy() for t in out["samples"]]
    near = (R.nearest(P, G), R.nearest(G, P))
    ref = R.scores(P, Pn, G, Gn, thresholds, near=near)
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq") + (("normal_consistency",) if ref["normal_consistency"] is not None else ()):
        ratio = abs(out[k] - ref[k]) / (BAR * abs(ref[k])) if ref[k] != 0 else float(out[k] != 0)
        _note("scores " + k, ratio)
        assert ratio <= 1.0, (k, out[k], ref[k])
    for side, (d64, _), n in (("precision", near[0], len(P)), ("recall", near[1], len(G))):
        for t, got in zip(thresholds, out[side]):
            t32 = float(np.float32(t))
            lo, hi = int((d64 <= t32 * (1 - BAR)).sum()), int((d64 <= t32 * (1 + BAR)).sum())
            assert lo <= round(got * n) <= hi and abs(got * n - round(got * n)) < 1e-6, (side, t, got * n, lo, hi)
    for p, r, f in zip(out["precision"], out["recall"], out["fscore"]):
        assert f == (2.0 * p * r / (p + r) if p + r > 0 else 0.0)
    return ref


def test_scores_equal_the_restatement_from_the_devices_samples(hip_lib):
    from lara_amd import meshmetrics
    V, F = R.uv_sphere()
    assert 450 <= len(F) <= 550
    pred, gt = (_t(V * np.float32(1.02)), _t(F)), (_t(V), _t(F), None)          # (a read_obj mesh carries a third entry)
    out = meshmetrics.surface_scores(pred, gt, n=4096, thresholds=THR, seed=0, return_samples=True)
    ref = _check_scores(out, THR)
    assert out["n_pred"] == out["n_gt"] == 4096 and 0.018 < out["accuracy"] < 0.03 and out["normal_consistency"] > 0.99
    assert out["fscore"][0] == 0.0 and out["fscore"][-1] == 1.0 and ref["fscore"][-1] == 1.0
    # a second call: the same bits
    again = meshmetrics.surface_scores(pred, gt, n=4096, thresholds=THR, seed=0)
    assert {k: v for k, v in out.items() if k != "samples"} == again


def test_a_sphere_against_itself_and_bare_point_sets(hip_lib):
    from lara_amd import meshmetrics
    V, F = R.uv_sphere()
    mesh = (_t(V), _t(F))
    spacing = float(np.sqrt(R.areas(V, F).sum() / 4096))
    out = meshmetrics.surface_scores(mesh, mesh, n=4096, thresholds=(1e-6, spacing), return_samples=True)
    assert out["fscore"] == [1.0, 1.0] and out["chamfer"] == 0.0 < spacing and abs(out["normal_consistency"] - 1.0) < 2.0 ** -22
    _check_scores(out, (1e-6, spacing))
    # other samples of the same surface: each direction's mean stays below the sample spacing
    a = meshmetrics.sample_surface(*mesh, 4096, seed=1)
    b = meshmetrics.sample_surface(*mesh, 4096, seed=2)
    out = meshmetrics.surface_scores((a[0], a[1]), (b[0], b[1]), thresholds=(spacing,), return_samples=True)
    assert 0 < out["accuracy"] < spacing and 0 < out["completeness"] < spacing and out["normal_consistency"] > 0.98
    _check_scores(out, (spacing,))
    # bare point sets, in every accepted spelling: no normals, no normal consistency
    for pred, gt in ((a[0], b[0]), ((a[0],), (b[0], b[1])), ((a[0], a[1]), b[0].cpu().numpy())):
        bare = meshmetrics.surface_scores(pred, gt, thresholds=(spacing,))
        assert bare["normal_consistency"] is None and bare["chamfer"] == out["chamfer"] and bare["fscore"] == out["fscore"]


def test_scores_on_a_side_stream_give_the_same_bits(hip_lib):
    from lara_amd import meshmetrics
    V, F = R.uv_sphere()
    pred, gt = (_t(V * np.float32(1.02)), _t(F)), (_t(V), _t(F))
    want = meshmetrics.surface_scores(pred, gt, n=4096, thresholds=THR, return_samples=True)
    torch.cuda.synchronize()
    busy = torch.randn(2048, 2048, device=_dev())
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    for _ in range(20):
        busy = torch.tanh(busy @ busy) * 0.5          # the default stream is busy while the side stream scores
    with torch.cuda.stream(side):
        got = meshmetrics.surface_scores(pred, gt, n=4096, thresholds=THR, return_samples=True)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b in zip(want.pop("samples"), got.pop("samples")):
        assert torch.equal(a, b)
    assert want == got and bool(torch.isfinite(busy).all())


def test_bench_tool_runs_at_its_quick_size(hip_lib, tmp_path):
    out = tmp_path / "bench.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "meshmetrics_bench.py"), "--quick", "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(run.stdout.strip().splitlines()[-1]) == res
    (size,) = res["sizes"]
    assert size["samples_per_side"] <= 20000 and size["grid_ms"] > 0 and size["cdist_ms"] > 0
    assert 0.0 <= size["fallback_share"] <= 1.0 and size["chamfer"] > 0
    # (the baseline's distances come from |a|^2 + |b|^2 - 2 a.b in fp32: cancellation costs it about 1e-3 of a distance here)
    assert abs(size["chamfer"] - size["cdist_chamfer"]) <= 1e-2 * size["chamfer"]
