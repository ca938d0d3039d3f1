"""include/lara_meshsign.h without a GPU: the header's constants held to the module's and the library's refusals; the crossing
of csrc/raycross.h, through its host entry, equal to the float64 restatement (tests/meshsign_restate.py) as integers on every group
of tests/meshray_cases.bound_groups; the host brute force equal to the restated one on every mesh of tests/meshray_cases.CASES; the
restated counting walk equal to restated brute force on the same cases -- and the same walk with a plain slab test shown to LOSE
crossings on the flat groups, so the cases bite; analytic truth on the two spheres under both rules; the open mesh's unanimity
rate; the crafted rays that meet a corner or an edge of the dyadic cube exactly; the mesh that leaves a point without a usable ray;
the vote over all combinations of three rays; `Evaluator.add_volume`.  tests/test_meshsign_gpu.py holds the kernels to the same
restatement.

Every comparison is between integers: there is no tolerance in this file."""
import itertools
import json
import sys

import numpy as np
import pytest

from lara_amd import evaluate
from tests import meshbvh_restate as RB
from tests import meshdist_restate as R
from tests import meshray_cases as MC
from tests import meshray_restate as RR
from tests import meshsign_cases as SC
from tests import meshsign_restate as S

F32 = np.float32


def test_header_constants_equal_the_modules():
    import os
    from lara_amd import meshsign
    from tests import test_abi_cpu as abi
    text = open(os.path.join(abi.ROOT, "include", "lara_meshsign.h")).read()
    assert f"#define LARA_MESHSIGN_MAX_RAYS {meshsign.MAX_RAYS}\n" in text and meshsign.MAX_RAYS == S.MAX_RAYS == 3
    assert f"#define LARA_MESHSIGN_RULE_PARITY {meshsign.RULES['parity']}\n" in text and meshsign.RULES["parity"] == S.PARITY
    assert f"#define LARA_MESHSIGN_RULE_WINDING {meshsign.RULES['winding']}\n" in text and meshsign.RULES["winding"] == S.WINDING
    rows = ", ".join("{" + ", ".join(f"{x!r}f" for x in d) + "}" for d in meshsign.DIRECTIONS)
    assert "#define LARA_MESHSIGN_DIRECTIONS {" + rows + "}\n" in text
    assert np.array_equal(np.array(meshsign.DIRECTIONS, F32), S.DIRECTIONS)
    assert np.all(np.abs(S.DIRECTIONS).max(1) == 1) and np.all(S.DIRECTIONS * 16 == np.round(S.DIRECTIONS * 16))


def test_refusals(hip_lib):
    """K outside 1 .. 3, N K of 2^30 and more, negative counts, an unknown rule and null pointers come back as
    LARA2DGS_E_INVALID (-1) from host code, before any pointer is used; N = 0 is a no-op; python refuses CPU tensors, a ray count
    outside 1 .. 3 and an unknown rule."""
    import torch
    from lara_amd import meshbvh, meshsign
    rows = hip_lib.lara_meshsign_rows
    for K in (0, 4, -1):
        assert rows(5, 1, K, 1, 1, 1, None) == -1
    assert rows(-1, 1, 3, 1, 1, 1, None) == -1 and rows(1 << 30, 1, 1, 1, 1, 1, None) == -1
    assert rows((1 << 30) // 3 + 1, 1, 3, 1, 1, 1, None) == -1 and rows(1 << 29, 1, 2, 1, 1, 1, None) == -1
    assert rows(0, None, 3, None, None, None, None) == 0
    for hole in range(4):
        args = [1, 1, 1, 1]
        args[hole] = None
        assert rows(5, args[0], 3, args[1], args[2], args[3], None) == -1
    vote = hip_lib.lara_meshsign_vote
    for K in (0, 4):
        assert vote(5, K, 1, 1, 0, None, 1, 1, None, None) == -1
    assert vote(5, 3, 1, 1, 2, None, 1, 1, None, None) == -1 and vote(5, 3, 1, 1, -1, None, 1, 1, None, None) == -1
    assert vote(-1, 3, 1, 1, 0, None, 1, 1, None, None) == -1 and vote(1 << 29, 3, 1, 1, 0, None, 1, 1, None, None) == -1
    assert vote(0, 3, None, None, 0, None, None, None, None, None) == 0
    for hole in range(4):
        args = [1, 1, 1, 1]
        args[hole] = None
        assert vote(5, 3, args[0], args[1], 0, None, args[2], args[3], None, None) == -1
    assert vote(5, 3, 1, 1, 0, None, 1, 1, 1, None) == -1                        # an sdf without a dist
    counts = hip_lib.lara_meshsign_counts
    assert counts(-1, 1, 1, 1, 1, 1, None) == -1 and counts(1 << 30, 1, 1, 1, 1, 1, None) == -1
    assert counts(0, None, None, None, None, None, None) == -1
    for hole in range(5):
        args = [1, 1, 1, 1, 1]
        args[hole] = None
        assert counts(5, *args, None) == -1
    assert hip_lib.lara_meshsign_volume(None, 1, None) == -1 and hip_lib.lara_meshsign_volume(1, None, None) == -1
    cross = hip_lib.lara_meshsign_cross_host
    assert cross(-1, None, None, None, None, None, None) == -1 and cross(3, None, None, None, None, None, None) == -1
    assert cross(0, None, None, None, None, None, None) == 0
    host = hip_lib.lara_meshsign_rows_host
    assert host(-1, 1, 3, 1, 1, 1, 1) == -1 and host(5, 1, 0, 1, 1, 1, 1) == -1 and host(5, 1, 4, 1, 1, 1, 1) == -1
    assert host(5, 1, 3, -1, 1, 1, 1) == -1 and host(1 << 29, 1, 2, 1, 1, 1, 1) == -1 and host(5, None, 3, 1, 1, 1, 1) == -1
    assert host(5, 1, 3, 1, None, 1, 1) == -1 and host(5, 1, 3, 1, 1, None, 1) == -1 and host(5, 1, 3, 1, 1, 1, None) == -1
    assert host(0, None, 3, 0, None, None, None) == 0
    V, F = R.icosphere(0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshsign.contains(meshbvh.TriangleBVH(torch.from_numpy(V), torch.from_numpy(F)), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="rays must be"):
        meshsign.crossings(None, torch.zeros(4, 3), rays=4)
    with pytest.raises(ValueError, match="rule must be"):
        meshsign.contains(None, torch.zeros(4, 3), rule="odd")


def test_the_package_does_not_import_meshsign():
    """Opt-in: importing the package and its mesh modules leaves `lara_amd.meshsign` out."""
    import lara_amd
    saved = sys.modules.pop("lara_amd.meshsign", None)
    vars(lara_amd).pop("meshsign", None)
    try:
        from lara_amd import meshbvh, meshdist, meshray      # noqa: F401
        assert "lara_amd.meshsign" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["lara_amd.meshsign"] = saved
            setattr(lara_amd, "meshsign", saved)


# ---- the crossing ---------------------------------------------------------------------------------------------------------------

def _host_cross(hip_lib, o, d, tri):
    n = len(o)
    o, d, tri = (np.ascontiguousarray(x, F32) for x in (o, d, tri.reshape(n, 9)))
    hit, orient, touch = np.empty(n, np.uint8), np.empty(n, np.int8), np.empty(n, np.uint8)
    assert hip_lib.lara_meshsign_cross_host(n, o.ctypes.data, d.ctypes.data, tri.ctypes.data, hit.ctypes.data, orient.ctypes.data,
                                            touch.ctypes.data) == 0
    return hit, orient, touch


def _host_rows(hip_lib, P, K, V, F):
    ok = R.valid_triangles(V, F)
    tri = np.ascontiguousarray(np.stack(R.corners(V, F), 1)[ok].reshape(-1, 9), F32)
    P = np.ascontiguousarray(P, F32)
    cross, wind = np.empty((len(P), K), np.int32), np.empty((len(P), K), np.int32)
    assert hip_lib.lara_meshsign_rows_host(len(P), P.ctypes.data, K, len(tri), tri.ctypes.data if len(tri) else None, cross.ctypes.data,
                                           wind.ctypes.data) == 0
    return cross, wind


def test_host_crossing_equals_the_restatement_on_the_bound_groups(hip_lib):
    """Hit, orientation and touch flag as integers on every group; with the window [0, +inf) the crossing accepts exactly where
    the ray-triangle function's host entry does; aimed at edges and vertices, the groups hold touching rays."""
    hits = touches = 0
    for name, (o, d, _, _, tri, _, _) in sorted(MC.bound_groups().items()):
        hit, orient, touch = _host_cross(hip_lib, o, d, tri)
        rhit, rorient, rtouch = S.cross(RR.setup(o, d), tri[:, 0], tri[:, 1], tri[:, 2])
        assert np.array_equal(hit, rhit.astype(np.uint8)) and np.array_equal(orient, rorient), name
        assert np.array_equal(touch, rtouch.astype(np.uint8)), name
        n = len(o)
        h2, t2, b2 = np.empty(n, np.uint8), np.empty(n), np.empty((n, 3))
        oc, dc, tc = (np.ascontiguousarray(x, F32) for x in (o, d, tri.reshape(n, 9)))
        assert hip_lib.lara_meshray_raytri_host(n, oc.ctypes.data, dc.ctypes.data, None, None, tc.ctypes.data, h2.ctypes.data,
                                                t2.ctypes.data, b2.ctypes.data) == 0
        assert np.array_equal(hit, h2)
        assert np.all(np.abs(orient[hit == 1]) == 1) and np.all(orient[hit == 0] == 0) and np.all(touch[hit == 0] == 0)
        assert np.array_equal(touch[hit == 1] == 1, (b2[hit == 1] == 0).any(1))          # a zero edge function is a zero weight
        print(f"meshsign crossing, {name}: {n} pairs, {int(hit.sum())} crossings, {int(touch.sum())} touching, "
              f"{int((orient == 1).sum())} leaving")
        hits, touches = hits + int(hit.sum()), touches + int(touch.sum())
    assert hits > 20000 and touches > 100


def test_orientation_closed_form(hip_lib):
    """A ray up the z axis through a triangle in the plane z = 1: wound counter-clockwise seen from above its normal is +z, the ray
    leaves through it (+1); the other winding is -1; through a vertex it touches; below the origin it misses."""
    ccw, cw = [[0, 0, 1], [4, 0, 1], [0, 4, 1]], [[0, 0, 1], [0, 4, 1], [4, 0, 1]]
    tri = np.array([ccw, cw, ccw, ccw, ccw], F32)
    o = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0], [1, 1, 2], [2, 0, 0]], F32)
    d = np.array([[0, 0, 1]] * 5, F32)
    hit, orient, touch = _host_cross(hip_lib, o, d, tri)
    assert hit.tolist() == [1, 1, 1, 0, 1] and orient.tolist() == [1, -1, 1, 0, 1] and touch.tolist() == [0, 0, 1, 0, 1]


@pytest.mark.parametrize("key", sorted(MC.CASES))
def test_host_brute_force_equals_the_restatement(hip_lib, key):
    c = SC.case(key)
    for K in (1, 2, 3):
        cross, wind = _host_rows(hip_lib, c["P"], K, c["V"], c["F"])
        assert np.array_equal(cross, c["cross"][:, :K]) and np.array_equal(wind, c["wind"][:, :K]), (key, K)
    fin = np.isfinite(c["P"]).all(1)
    assert np.all(c["cross"][~fin] == -1) and np.all(c["wind"][~fin] == 0)
    print(f"meshsign {key}: {len(c['P'])} points, crossings up to {int(c['cross'].max())}, "
          f"{int((c['cross'][fin] < 0).sum())} touching rays")
    if key == "copies_4096":          # a ray through the triangle meets every copy
        assert (c["cross"] == 4096).sum() > 0 and set(np.unique(c["cross"]).tolist()) <= {-1, 0, 4096}
        assert np.all(np.abs(c["wind"][c["cross"] == 4096]) == 4096)


# ---- the restated walk against restated brute force -----------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(MC.CASES))
def test_restated_walk_equals_brute_force(key):
    """The pruning logic without a GPU: the counting walk over the restated hierarchy gives brute force's rows."""
    c = SC.case(key)
    bvh = RB.BVH(c["V"], c["F"])
    n = len(c["P"])
    idx = np.arange(n) if n <= 60 else np.unique(np.concatenate([np.arange(30), np.arange(30, n, max(1, n // 40))]))
    if key == "copies_4096":
        idx = np.concatenate([idx[:12], np.nonzero((c["cross"] == 4096).any(1))[0][:4]])
    fin = np.isfinite(c["P"]).all(1)
    tests = []
    for i in idx:
        for k in range(S.MAX_RAYS):
            cr, wi, touched, stats = S.walk(bvh, c["P"][i], S.DIRECTIONS[k])
            got = S.usable_rows(np.array([cr]), np.array([wi]), np.array([touched]), fin[i:i + 1])
            assert (int(got[0][0]), int(got[1][0])) == (int(c["cross"][i, k]), int(c["wind"][i, k])), (key, int(i), k)
            tests.append(stats["tests"])
    print(f"meshsign restated walk {key}: {np.mean(tests):.1f} triangle tests per ray of {bvh.n_valid} triangles")
    if key in ("icosphere", "uv_sphere", "sphere_square"):          # the walk prunes: a small part of the mesh is tested
        assert np.mean(tests) < 0.1 * bvh.n_valid


def test_a_walk_without_the_margins_loses_crossings_on_the_flat_groups():
    """Teeth: a flat, axis-aligned triangle under a hierarchy of its own has boxes without thickness.  Pruned with the plain slab
    test the counting walk loses crossings brute force counts: the flat axis gives a one-point parameter interval, and for a ray
    aimed at an edge or a vertex the computed intervals of the other two axes end a rounding before it.  With the margins it loses
    none.  (Rays ALONG the flat axis cannot show it with the window [0, +inf): their other two axes have no interval at all, and
    one point is not empty; that group must come through whole either way.)"""
    total = 0
    for name in MC.FLAT:
        o, d, _, _, tri, _, _ = MC.bound_groups()[name]
        lost = kept = crossings = 0
        for i in range(0, 800):
            V, F = tri[i], np.arange(3, dtype=np.int64)[None]
            want = S.ray_rows(o[i], d[i], V, F)[0][0]
            if want == 0:
                continue
            bvh = RB.BVH(V, F)
            crossings += 1
            kept += int(S.walk(bvh, o[i], d[i])[0] != want)
            lost += int(S.walk(bvh, o[i], d[i], margin=False)[0] != want)
        print(f"meshsign walk, {name}: {crossings} crossings of 800 rays, {lost} lost without the margins, {kept} with them")
        assert kept == 0 and crossings > 400, name
        assert lost == 0 if name == "flat, axis-aligned rays" else lost > 0, name
        total += lost
    assert total >= 2


# ---- truth ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["icosphere", "uv_sphere"])
def test_analytic_truth_on_the_spheres(hip_lib, name):
    """1 500 seeded points in [-1.3, 1.3]^3: beyond radius 1.001 every point is outside, below 0.999 of the inscribed radius every
    point is inside, under both rules, with all three rays usable and unanimous, and wind = +1 inside, 0 outside."""
    V, F = MC.watertight_meshes()[name]
    P = SC.analytic_points()
    cross, wind = _host_rows(hip_lib, P, 3, V, F)
    rc, rw = S.rows(P, 3, V, F)
    assert np.array_equal(cross, rc) and np.array_equal(wind, rw)
    r = np.linalg.norm(P.astype(np.float64), axis=1)
    r_in = SC.inscribed_radius(V, F)
    vol = S.volume(V, F)
    assert abs(vol[0] - {"icosphere": 4.1527, "uv_sphere": 4.0229}[name]) < 1e-4 and vol[2] == len(F)
    out, ins = r > 1.001, r < 0.999 * r_in
    assert out.sum() > 1000 and ins.sum() > 300 and np.all(cross >= 0)
    assert np.all(cross[out] % 2 == 0) and np.all(wind[out] == 0) and np.all(cross[ins] % 2 == 1) and np.all(wind[ins] == 1)
    for rule in (S.PARITY, S.WINDING):
        inside, status, _ = S.vote(cross, wind, rule)
        assert np.all(status == 0), (name, rule)
        assert np.all(inside[out] == 0) and np.all(inside[ins] == 1)
    print(f"meshsign {name}: inscribed radius {r_in:.6f}, signed volume {vol[0]:.4f}, {int(out.sum())} outside, {int(ins.sum())} inside, "
          f"{len(P) - int(out.sum()) - int(ins.sum())} in the shell between")


def test_the_open_mesh_is_flagged():
    """The sphere plus an open square: the rays disagree on part of the points, and status bit 0 is set exactly there."""
    V, F = MC._mesh("sphere_square")
    P = SC.analytic_points()
    cross, wind = S.rows(P, 3, V, F)
    assert np.all(cross >= 0)
    for rule, votes in ((S.PARITY, cross % 2 == 1), (S.WINDING, wind != 0)):
        differ = votes.any(1) & ~votes.all(1)
        inside, status, _ = S.vote(cross, wind, rule)
        assert np.array_equal(status & 1 == 1, differ) and np.all(status & 6 == 0)
        rate = 1.0 - differ.mean()
        print(f"meshsign sphere plus open square, rule {rule}: unanimous on {100 * rate:.1f} % of {len(P)} points; winding sums "
              f"{int(wind.min())} .. {int(wind.max())}")
        assert 0.2 < rate < 0.9


def test_crafted_touching_rays_on_the_cube(hip_lib):
    """Exactly 8, 8 and 12 rays are unusable in the three set-ups, all of them the aimed ray; the vote over the other two rays
    still classifies every point as the cube's box says."""
    V, F = SC.cube()
    assert S.volume(V, F)[:3] == (1.0, 6.0, 12)
    for (k, P), n in zip(SC.touching_points(), (8, 8, 12)):
        cross, wind = _host_rows(hip_lib, P, 3, V, F)
        rc, rw = S.rows(P, 3, V, F)
        assert np.array_equal(cross, rc) and np.array_equal(wind, rw)
        unusable = (cross < 0).sum(0).tolist()
        assert len(P) == n and unusable == [n if j == k else 0 for j in range(3)], (k, unusable)
        in_box = (np.abs(P) < 0.5).all(1)
        for rule in (S.PARITY, S.WINDING):
            inside, status, _ = S.vote(cross, wind, rule)
            assert np.array_equal(inside == 1, in_box) and np.all(status == 2), (k, rule)
        print(f"meshsign cube, ray {k}: {n} points, unusable per ray {unusable}, {int(in_box.sum())} inside")
    assert (np.abs(SC.touching_points()[0][1]) < 0.5).all(1).sum() == 1 and (np.abs(SC.touching_points()[2][1]) < 0.5).all(1).sum() == 5


def test_a_point_without_a_usable_ray(hip_lib):
    """Three triangles, each with a vertex on one of the rays from the origin: status bit 2, outside, sdf = +dist."""
    V, F = SC.no_usable_ray()
    P = np.zeros((1, 3), F32)
    cross, wind = _host_rows(hip_lib, P, 3, V, F)
    assert cross.tolist() == [[-1, -1, -1]] and wind.tolist() == [[0, 0, 0]]
    assert [x.tolist() for x in S.rows(P, 3, V, F)] == [[[-1, -1, -1]], [[0, 0, 0]]]
    dist = R.brute(P, V, F)[0].astype(F32)
    for rule in (S.PARITY, S.WINDING):
        inside, status, sdf = S.vote(cross, wind, rule, dist)
        assert inside.tolist() == [0] and status.tolist() == [6] and sdf.tolist() == dist.tolist() and dist[0] > 0


def test_the_vote_over_all_combinations():
    """Three rays, each odd, even or unusable, under both rules, and the sign on the distance; written out independently."""
    kinds = {"odd": (3, 1), "even": (2, 0), "unusable": (-1, 0)}
    for combo in itertools.product(kinds, repeat=3):
        cross = np.array([[kinds[c][0] for c in combo]])
        wind = np.array([[kinds[c][1] for c in combo]])
        odd, usable = combo.count("odd"), 3 - combo.count("unusable")
        want_inside = 1 if 2 * odd > usable else 0
        want_status = (1 if 0 < odd < usable else 0) | (2 if usable < 3 else 0) | (4 if usable == 0 else 0)
        for rule in (S.PARITY, S.WINDING):
            inside, status, sdf = S.vote(cross, wind, rule, np.array([0.25], F32))
            assert (int(inside[0]), int(status[0]), float(sdf[0])) == (want_inside, want_status, -0.25 if want_inside else 0.25), combo
    # the rules differ where they should: two crossings with one orientation (overlapping parts) are even, and wound
    inside_p = S.vote(np.array([[2, 2, 2]]), np.array([[2, 2, 2]]), S.PARITY)[0]
    inside_w = S.vote(np.array([[2, 2, 2]]), np.array([[2, 2, 2]]), S.WINDING)[0]
    assert inside_p.tolist() == [0] and inside_w.tolist() == [1]
    for K in (1, 2):
        inside, status, _ = S.vote(np.array([[1, -1][:K], [1, 2][:K]]), np.array([[1, 0][:K], [1, 0][:K]]), S.PARITY)
        assert inside.tolist() == ([1, 1] if K == 1 else [1, 0]) and status.tolist() == ([0, 0] if K == 1 else [2, 1])
    nan = S.vote(np.array([[1, 1, 1]]), np.array([[1, 1, 1]]), S.PARITY, np.array([np.nan], F32))[2]
    assert np.isnan(nan[0])


def test_the_lattice_and_the_counts_restated():
    P, step = S.lattice([-1, 0, 2], [1, 4, 2.5], 4)
    assert step.tolist() == [0.5, 1.0, 0.125] and P.shape == (4, 4, 4, 3) and P.dtype == F32
    assert P[0, 0, 0].tolist() == [-0.75, 0.5, 2.0625] and P[3, 1, 2].tolist() == [0.75, 1.5, 2.3125]
    assert S.counts([1, 1, 0, 0], [0, 1, 4, 6], [1, 0, 1, 0], [1, 1, 5, 0]) == [2, 2, 1, 3, 1, 3, 2, 1]


# ---- hooks ----------------------------------------------------------------------------------------------------------------------

def test_add_volume_writes_its_keys_and_nothing_without_it(tmp_path):
    geometry = {"accuracy": 0.01, "completeness": 0.03, "chamfer": 0.04, "chamfer_sq": 0.0016, "normal_consistency": 0.9,
                "thresholds": [0.01, 0.02], "precision": [0.5, 1.0], "recall": [0.25, 0.5], "fscore": [1.0 / 3.0, 2.0 / 3.0]}

    def make(volume):
        e = evaluate.Evaluator(4)
        e.add_scores("a", 30.0, 0.9, None, 0.1, 0.2)
        e.add_scores("b", 20.0, 0.8, None, 0.3, 0.4)
        e.add_geometry("a", dict(geometry))
        for name, iou in volume:
            e.add_volume(name, {"volume_iou": iou, "volume_pred": 1.0, "n_lattice": 8})
        return e
    plain, with_volume = make([]), make([("a", 0.5), ("b", 0.75)])
    assert not any(k.startswith("volume") for k in plain.summary())
    plain.write(str(tmp_path / "plain.json"))
    with_volume.write(str(tmp_path / "volume.json"))
    a, b = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "volume.json"))
    assert list(b)[:len(a)] == list(a) and list(b)[len(a):] == ["volume_name", "volume_iou", "volume_iou_mean"]
    assert {k: b[k] for k in a} == a
    assert b["volume_name"] == ["a", "b"] and b["volume_iou"] == [0.5, 0.75] and b["volume_iou_mean"] == 0.625
    # without a call of add_volume the file holds the keys it held before there was one, in their order
    scalars, lists = evaluate.Evaluator.GEOMETRY_SCALARS, evaluate.Evaluator.GEOMETRY_LISTS
    assert list(a) == (["name", "psnr", "ssim", "lpips_vgg", "lpips_alex", "depth_acc", "psnr_mean", "ssim_mean", "lpips_vgg_mean",
                        "lpips_alex_mean", "geometry_name", "geometry_thresholds"] + [k + s for k in scalars + lists for s in ("", "_mean")])
    assert open(tmp_path / "plain.json").read() == json.dumps(plain.summary(), indent=4)
    only = evaluate.Evaluator(4)
    assert only.summary() is None
    only.add_volume("a", {"volume_iou": None})
    assert only.summary() == {"volume_name": ["a"], "volume_iou": [None], "volume_iou_mean": None}
