"""include/lara_meshray.h without a GPU: the header's constants held to the module's and the library's refusals; the ray-triangle
function of csrc/raytri.h, through its host entry, equal to the float64 restatement (tests/meshray_restate.py) bit for bit on every
ray set of tests/meshray_cases.py; watertightness on the two spheres -- and the unsheared triple-product form shown to LOSE a ray
there, so the rays bite; the margined entry parameter of csrc/raybox.h, through its host entry, held under the t the host function
computes on adversarial (ray, triangle, box) groups -- and a plain slab test shown to FAIL on the flat ones; the restated walk held
to restated brute force on every case with both sibling orders; the visibility restatement's ambiguous share; the keyword refusals
of `depthsurface`.  tests/test_meshray_gpu.py holds the kernels to the same restatement.

The bound's bar is the contract itself, with no tolerance: a finite entry <= t wherever the function computes a hit."""
import sys

import numpy as np
import pytest
import torch

from lara_amd import evaluate
from tests import meshbvh_restate as RB
from tests import meshdist_restate as R
from tests import meshray_cases as MC
from tests import meshray_restate as RR

F32 = np.float32
AMBIGUOUS_CAP = 0.005


def test_header_constants_equal_the_modules():
    from lara_amd import meshray
    from tests import test_abi_cpu as abi
    text = abi.header_texts()["lara_meshray.h"]
    assert f"#define LARA_MESHRAY_MAX_EYES {meshray.MAX_EYES}\n" in text and meshray.MAX_EYES == RR.MAX_EYES == 64
    assert f"#define LARA_MESHRAY_MASKED_ORDER {meshray.MASKED_ORDER}\n" in text


def test_refusals(hip_lib):
    """Counts of 2^30 and more, negative counts, null pointers, more than 64 eyes and a shrink outside [0, 1) come back as
    LARA2DGS_E_INVALID (-1) from host code, before any pointer is used; R = 0 and N = 0 are no-ops; python refuses CPU tensors."""
    from lara_amd import depthsurface, meshbvh, meshray
    for fn in (hip_lib.lara_meshray_cast, hip_lib.lara_meshray_cast_other_order):
        assert fn(1 << 30, 1, 1, None, None, 1, 1, 1, None, None) == -1 and fn(-1, 1, 1, None, None, 1, 1, 1, None, None) == -1
        assert fn(0, None, None, None, None, None, None, None, None, None) == 0
        assert fn(5, None, None, None, None, None, None, None, None, None) == -1
        for hole in range(5):          # (non-null pointers that must not be used: one of the five required ones is null)
            args = [1, 1, 1, 1, 1]
            args[hole] = None
            assert fn(5, args[0], args[1], None, None, args[2], args[3], args[4], None, None) == -1
    occ = hip_lib.lara_meshray_occluded
    assert occ(1 << 30, 1, 1, None, None, 1, 1, None) == -1 and occ(-2, 1, 1, None, None, 1, 1, None) == -1
    assert occ(0, None, None, None, None, None, None, None) == 0 and occ(3, 1, 1, None, None, 1, None, None) == -1
    vis = hip_lib.lara_meshray_visible
    assert vis(1 << 30, 1, None, 4, 1, 0.0, 1, 1, None) == -1 and vis(-1, 1, None, 4, 1, 0.0, 1, 1, None) == -1
    assert vis(5, 1, None, 65, 1, 0.0, 1, 1, None) == -1 and vis(5, 1, None, -1, 1, 0.0, 1, 1, None) == -1
    for shrink in (1.0, -0.5, 2.0, float("nan")):
        assert vis(5, 1, None, 4, 1, shrink, 1, 1, None) == -1
    assert vis(0, None, None, 4, None, 0.0, None, None, None) == 0
    assert vis(5, None, None, 4, 1, 0.0, 1, 1, None) == -1 and vis(5, 1, None, 4, None, 0.0, 1, 1, None) == -1
    assert vis(5, 1, None, 4, 1, 0.0, None, 1, None) == -1 and vis(5, 1, None, 4, 1, 0.0, 1, None, None) == -1
    assert hip_lib.lara_meshray_raytri_host(-1, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshray_raytri_host(3, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshray_raytri_host(0, None, None, None, None, None, None, None, None) == 0
    assert hip_lib.lara_meshray_box_entry_host(-1, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshray_box_entry_host(3, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshray_box_entry_host(0, None, None, None, None, None, None) == 0
    V, F = R.icosphere(0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshray.raycast(meshbvh.TriangleBVH(torch.from_numpy(V), torch.from_numpy(F)), torch.zeros(4, 3), torch.ones(4, 3))
    depth = torch.ones(1, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        depthsurface.depth_scores((torch.from_numpy(V), torch.from_numpy(F)), depth, None, torch.eye(3)[None], torch.eye(4)[None],
                                  self_occlusion=True)


def test_the_default_route_does_not_touch_meshray():
    """`depth_scores` without the keyword, and with ``self_occlusion=False``, never imports `lara_amd.meshray` or
    `lara_amd.meshbvh` (the route ends at the "no CPU path" check here); with the keyword a point set is refused."""
    import lara_amd
    from lara_amd import depthsurface
    V, F = R.icosphere(0)
    mesh = (torch.from_numpy(V), torch.from_numpy(F))
    depth, K, M = torch.ones(1, 4, 4), torch.eye(3)[None], torch.eye(4)[None]
    saved = {m: sys.modules.pop("lara_amd." + m, None) for m in ("meshray", "meshbvh")}
    for m in saved:
        vars(lara_amd).pop(m, None)
    try:
        for kw in ({}, {"self_occlusion": False}):
            with pytest.raises(RuntimeError, match="no CPU path"):
                depthsurface.depth_scores(mesh, depth, None, K, M, **kw)
            assert "lara_amd.meshray" not in sys.modules and "lara_amd.meshbvh" not in sys.modules
        for points in (mesh[0], (mesh[0],), (mesh[0], mesh[0])):
            with pytest.raises(ValueError, match="self_occlusion needs a prediction that is a mesh"):
                depthsurface.depth_scores(points, depth, None, K, M, self_occlusion=True)
            assert "lara_amd.meshray" not in sys.modules and "lara_amd.meshbvh" not in sys.modules
    finally:
        for m, mod in saved.items():
            if mod is not None:
                sys.modules["lara_amd." + m] = mod
                setattr(lara_amd, m, mod)


# ---- the function ---------------------------------------------------------------------------------------------------------------

def _host_raytri(hip_lib, o, d, t_min, t_max, tri):
    n = len(o)
    o, d, tri = (np.ascontiguousarray(x, F32) for x in (o, d, tri.reshape(n, 9)))
    lo, hi = np.ascontiguousarray(t_min, F32), np.ascontiguousarray(t_max, F32)
    hit, t, b = np.empty(n, np.uint8), np.empty(n), np.empty((n, 3))
    assert hip_lib.lara_meshray_raytri_host(n, o.ctypes.data, d.ctypes.data, lo.ctypes.data, hi.ctypes.data, tri.ctypes.data,
                                            hit.ctypes.data, t.ctypes.data, b.ctypes.data) == 0
    return hit.astype(bool), t, b


def _host_entry(hip_lib, o, d, lo, hi, t_min, t_max):
    n = len(o)
    o, d = np.ascontiguousarray(o, F32), np.ascontiguousarray(d, F32)
    boxes = np.ascontiguousarray(np.concatenate([lo, hi], 1), F32)
    a, b = np.ascontiguousarray(t_min, F32), np.ascontiguousarray(t_max, F32)
    out = np.empty(n)
    assert hip_lib.lara_meshray_box_entry_host(n, o.ctypes.data, d.ctypes.data, boxes.ctypes.data, a.ctypes.data, b.ctypes.data,
                                               out.ctypes.data) == 0
    return out


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("key", sorted(MC.CASES))
def test_host_function_equals_the_restatement_on_the_ray_sets(hip_lib, key):
    """Every ray of the case against a triangle of the mesh (the one brute force found, else one in turn), and every ray against
    every triangle of the small meshes: hit flag, t and barycentrics as integers."""
    c = MC.case(key)
    p = np.stack(R.corners(c["V"], c["F"]), 1)
    n, T = len(c["o"]), len(p)
    which = np.where(c["face"] >= 0, c["face"], np.arange(n) % T)
    pairs = [(np.arange(n), which), (np.arange(n), (which + 1) % T)]
    if T <= 64:
        pairs.append((np.repeat(np.arange(n), T), np.tile(np.arange(T), n)))
    for ri, ti in pairs:
        o, d, lo, hi, tri = c["o"][ri], c["d"][ri], c["t_min"][ri], c["t_max"][ri], p[ti]
        hit, t, b = _host_raytri(hip_lib, o, d, lo, hi, tri)
        rhit, rt, rb, _ = RR.raytri(RR.setup(o, d), lo, hi, tri[:, 0], tri[:, 1], tri[:, 2])
        assert np.array_equal(hit, rhit), (key, int((hit != rhit).sum()))
        assert _same_bits(t, rt) and _same_bits(b, rb), key
        assert np.all(np.isposinf(t[~hit])) and np.isnan(b[~hit]).all() and np.isfinite(t[hit]).all()
    hit, t, b = _host_raytri(hip_lib, c["o"], c["d"], c["t_min"], c["t_max"], p[which])
    found = (c["face"] >= 0) & R.valid_triangles(c["V"], c["F"])[which]
    assert np.all(hit[found]) and _same_bits(t[found], c["t64"][found])
    assert np.allclose(b[hit].sum(1), 1.0, atol=1e-9)


def test_host_function_without_windows_and_its_closed_forms(hip_lib):
    """NULL windows are [0, +inf); a ray down the z axis onto a triangle in the plane z = 0 has t = the height and the barycentric
    weights of the foot point; both sides count; d is not normalised: scaling d by s scales t by 1 / s."""
    tri = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]] * 6, F32)
    o = np.array([[1, 1, 2], [1, 1, -2], [1, 1, 2], [3, 3, 2], [1, 1, 2], [0, 0, 2]], F32)
    d = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -4], [0, 0, -1], [0, 0, 1], [0, 0, -1]], F32)
    n = len(o)
    hit, t, b = np.empty(n, np.uint8), np.empty(n), np.empty((n, 3))
    assert hip_lib.lara_meshray_raytri_host(n, o.ctypes.data, d.ctypes.data, None, None, np.ascontiguousarray(tri.reshape(n, 9)).ctypes.data,
                                            hit.ctypes.data, t.ctypes.data, b.ctypes.data) == 0
    assert hit.tolist() == [1, 1, 1, 0, 0, 1]          # (3, 3) lies outside; the fifth points away; the last meets a vertex
    assert t[[0, 1, 2, 5]].tolist() == [2.0, 2.0, 0.5, 2.0]
    assert b[0].tolist() == [0.5, 0.25, 0.25] and b[5].tolist() == [1.0, 0.0, 0.0]


@pytest.mark.parametrize("name", ["icosphere", "uv_sphere"])
def test_watertightness(name):
    """From three origins inside the sphere to every vertex, to the midpoints of two edges of every face and to every centroid, d
    and 3 d: every ray hits at least once, the sanity clause rejects nothing, at most 64 triangles share a ray (the pole of the UV
    sphere).  Teeth: under the unsheared triple-product form at least one of the same rays is left without a hit (1 of the 3 138
    from the origin of the UV sphere: the one to a vertex on the equator whose coordinates carry the rounding of sin and cos)."""
    V, F = MC.watertight_meshes()[name]
    p0, p1, p2 = R.corners(V, F)
    slipped = 0
    for origin in MC.WATERTIGHT_ORIGINS:
        for scale in (1.0, 3.0):
            o, d = MC.watertight_rays(V, F, origin, scale)
            assert len(o) == {"icosphere": 4482, "uv_sphere": 3138}[name]
            t, _, rej = RR.all_hits(o, d, V, F)
            hits = np.isfinite(t).sum(1)
            print(f"meshray watertight {name} from {origin} x {scale}: {int((hits == 0).sum())} rays without a hit, {int(rej.sum())} "
                  f"rejections, at most {int(hits.max())} hits on a ray")
            assert np.all(hits >= 1) and rej.sum() == 0 and hits.max() <= 64
            lost = np.zeros(len(o), bool)
            for s in range(0, len(o) if name == "uv_sphere" else 0, 512):
                lost[s:s + 512] = ~RR.triple_product_hits(o[s:s + 512, None], d[s:s + 512, None], p0[None], p1[None], p2[None]).any(1)
            slipped += int(lost.sum())
            if name == "uv_sphere" and origin == (0.0, 0.0, 0.0) and scale == 1.0:
                assert hits[0] == 64                       # the ray through the pole (vertex 0) meets all 64 wedges
                # the ray to vertex 241 = (-1.8e-16, -1, 6.1e-17), where six triangles meet: all six, or under the other form none
                assert lost[241] and hits[241] == 6 and lost.sum() == 1
            print(f"    the triple-product form leaves {int(lost.sum())} of these rays without a hit")
    if name == "uv_sphere":
        assert slipped >= 1


# ---- the bound ------------------------------------------------------------------------------------------------------------------

_groups = {}


def _bound_groups():
    if not _groups:
        _groups.update(MC.bound_groups())
    return _groups


def test_entry_never_exceeds_the_computed_t(hip_lib):
    """Every group of tests/meshray_cases.bound_groups: wherever the host function computes a hit at t, the host entry of the box
    is finite and <= t; the host entry equals the restated one bit for bit; the scalar form the restated walk uses equals it too."""
    total = 0
    for name, (o, d, lo_t, hi_t, tri, lo, hi) in sorted(_bound_groups().items()):
        assert np.all(lo <= tri.min(1)) and np.all(hi >= tri.max(1))
        hit, t, _ = _host_raytri(hip_lib, o, d, lo_t, hi_t, tri)
        e = _host_entry(hip_lib, o, d, lo, hi, lo_t, hi_t)
        ray = RR.setup(o, d)
        assert _same_bits(e, RR.box_entries(ray, lo, hi, lo_t, hi_t)), name
        for i in range(0, len(o), 97):
            one = RR.scalar_ray(RR._at(ray, i))
            assert _same_bits(RR.box_entry(one, lo[i], hi[i], float(lo_t[i]), float(hi_t[i])), e[i])
        gap = float(((t[hit] - e[hit]) / np.maximum(np.abs(t[hit]), 1e-300)).min()) if hit.any() else 0.0
        print(f"meshray bound, {name}: {len(o)} groups, {int(hit.sum())} hits, smallest (t - entry) / |t| = {gap:.3e}")
        assert np.all(np.isfinite(e[hit])) and np.all(e[hit] <= t[hit]), (name, int((hit & ~(e <= t)).sum()))
        assert np.all(e >= lo_t.astype(np.float64))
        total += int(hit.sum())
    assert total > 20000


def test_entry_of_special_boxes(hip_lib):
    """The empty box (lo > hi, as the build stores it) is +inf whatever the ray; a ray that never hits is +inf whatever the box; a
    box behind the origin, or beyond t_max, is +inf; an origin inside the box enters at t_min; growing the box never raises the
    entry."""
    g = np.random.default_rng(61)
    n = 200
    o, d = (g.random((n, 3)) * 4 - 2).astype(F32), g.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    inf, zero, far = np.full((n, 3), np.inf, F32), np.zeros(n, F32), np.full(n, np.inf, F32)
    assert np.all(np.isposinf(_host_entry(hip_lib, o, d, inf, -inf, zero, far)))
    lo, hi = np.full((n, 3), -3, F32), np.full((n, 3), 3, F32)
    assert np.all(_host_entry(hip_lib, o, d, lo, hi, zero, far) == 0)
    assert np.all(_host_entry(hip_lib, o, d, lo, hi, zero + F32(0.25), far) == 0.25)
    assert np.all(np.isposinf(_host_entry(hip_lib, o, np.zeros((n, 3), F32), lo, hi, zero, far)))
    bad = d.copy()
    bad[:, 1] = np.nan
    assert np.all(np.isposinf(_host_entry(hip_lib, o, bad, lo, hi, zero, far)))
    ahead = o + d * F32(5)
    e = _host_entry(hip_lib, o, d, ahead - F32(0.5), ahead + F32(0.5), zero, far)
    assert np.all(np.isfinite(e)) and np.all(e > 4) and np.all(e < 5)
    assert np.all(np.isposinf(_host_entry(hip_lib, o, d, ahead - F32(0.5), ahead + F32(0.5), zero, zero + F32(3))))
    assert np.all(np.isposinf(_host_entry(hip_lib, o, -d, ahead - F32(0.5), ahead + F32(0.5), zero, far)))
    assert np.all(_host_entry(hip_lib, o, d, ahead - F32(1.5), ahead + F32(1.5), zero, far) <= e)


def test_a_plain_slab_test_fails_on_the_flat_cases(hip_lib):
    """Teeth: the same comparison with the slab test neither inflated nor widened must find violations on the flat, axis-aligned
    triangles -- a box without thickness has a one-point parameter interval, and the computed t of the hit lies beside it --, so
    those groups can tell a bound without its margins."""
    total = 0
    for name in MC.FLAT:
        o, d, lo_t, hi_t, tri, lo, hi = _bound_groups()[name]
        hit, t, _ = _host_raytri(hip_lib, o, d, lo_t, hi_t, tri)
        e = RR.box_entries(RR.setup(o, d), lo, hi, lo_t, hi_t, margin=False)
        bad = hit & ~(e <= t)
        print(f"meshray plain slab test, {name}: {int(bad.sum())} of {int(hit.sum())} hits violate the contract")
        assert bad.sum() > 100, name
        total += int(bad.sum())
    assert total > 1000


# ---- the restated walk against restated brute force -----------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(MC.CASES))
def test_restated_walk_equals_brute_force(key):
    """Identical faces and t bits with both sibling orders, and the any-hit walk agrees with face >= 0."""
    c = MC.case(key)
    bvh = RB.BVH(c["V"], c["F"])
    n = len(c["o"])
    idx = np.arange(n) if n <= 80 else np.unique(np.concatenate([np.arange(40), np.arange(40, n, max(1, n // 60))]))
    if key == "copies_4096":          # (a ray that hits meets all 4 096 copies: fewer of them)
        idx = idx[:24]
    tests = {}
    for masked in (True, False):
        got = [RR.walk(bvh, c["o"][i], c["d"][i], c["t_min"][i], c["t_max"][i], masked=masked) for i in idx]
        assert [g[0] for g in got] == c["face"][idx].tolist(), (key, masked)
        assert _same_bits([g[1] for g in got], c["t64"][idx]), (key, masked)
        tests[masked] = float(np.mean([g[2]["tests"] for g in got]))
    any_hit = [RR.walk(bvh, c["o"][i], c["d"][i], c["t_min"][i], c["t_max"][i], any_hit=True)[0] >= 0 for i in idx]
    assert any_hit == (c["face"][idx] >= 0).tolist()
    print(f"meshray restated walk {key}: {tests[True]:.1f} triangle tests per ray with the sign mask, {tests[False]:.1f} in the stored "
          f"order, of {bvh.n_valid} triangles")
    if key in ("icosphere", "uv_sphere", "sphere_square"):          # the walk prunes: a small part of the mesh is tested
        assert max(tests.values()) < 0.1 * bvh.n_valid


def test_restated_walk_on_ties_and_without_candidates():
    """4 096 copies of one triangle: every t is equal and only the strict skip rule reaches face 0; a mesh without a valid
    triangle and rays that can never hit come back as misses."""
    c = MC.case("copies_4096")
    bvh = RB.BVH(c["V"], c["F"])
    hit = np.nonzero(c["face"] >= 0)[0][:6]
    assert len(hit) == 6 and np.all(c["face"][hit] == 0) and np.all(c["hits"][hit] == 4096)
    for i in hit:
        for masked in (True, False):
            assert RR.walk(bvh, c["o"][i], c["d"][i], masked=masked)[0] == 0
    # an entry that EQUALS the best t: 100 copies in the plane z = 0, the ray meets them at t = 2 = t_min exactly and, its d_z
    # being negative, meets the later leaves first: only the strict skip rule still enters the leaf of face 0
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], F32)
    flat = RB.BVH(np.tile(tri, (100, 1)), np.arange(300, dtype=np.int64).reshape(100, 3))
    ray = ([1, 1, 2], [0, 0, -1])
    assert RR.walk(flat, *ray, t_min=2.0)[:2] == (0, 2.0) and RR.walk(flat, *ray, t_min=2.0, masked=False)[:2] == (0, 2.0)
    assert RR.walk(flat, *ray, t_min=2.0, strict=False)[0] > 0
    V1, F1 = R.icosphere(1)
    none = RB.BVH(V1, np.full((5, 3), len(V1) + 1, np.int64))
    assert none.counts == [5, 0, 5, 1] and RR.walk(none, [0, 0, 0], [1, 0, 0])[:2] == (-1, np.inf)
    bvh = RB.BVH(V1, F1)
    for o, d in (([0, 0, 0], [0, 0, 0]), ([0, 0, 0], [np.nan, 1, 0]), ([0, np.inf, 0], [1, 0, 0]), ([0, 0, 0], [1, -np.inf, 0])):
        assert RR.walk(bvh, o, d)[:2] == (-1, np.inf)
    assert RR.walk(bvh, [0, 0, 0], [1, 0, 0])[0] >= 0 and RR.walk(bvh, [0, 0, 0], [1, 0, 0], t_max=0.5)[0] == -1
    assert RR.walk(bvh, [3, 0, 0], [1, 0, 0])[0] == -1 and RR.walk(bvh, [3, 0, 0], [1, 0, 0], t_min=-10)[0] >= 0


def test_a_walk_without_the_margins_goes_wrong_on_the_fan():
    """Teeth for the walk itself: the fan lies in the plane z = 0 and every box is flat.  A ray through the centre meets all 256
    wedges at values of t that differ in their last bits; pruned with the plain slab test, whose entry lies beside the computed t,
    the walk steps over the leaf that holds brute force's answer."""
    V, F = R.fan(256)
    bvh = RB.BVH(V, F)
    g = np.random.default_rng(62)
    o = (g.normal(size=(200, 3)) * [0.5, 0.5, 1.0]).astype(F32)
    d = (-o).astype(F32)
    _, face, _, _, hits, _ = RR.brute(o, d, V, F)
    assert (hits == 256).sum() > 100          # (the others pass the centre by a rounding of the shear and meet one wedge)
    lost = sum(RR.walk(bvh, o[i], d[i], margin=False)[0] != face[i] for i in range(200))
    kept = sum(RR.walk(bvh, o[i], d[i])[0] != face[i] for i in range(200))
    print(f"meshray walk on the fan: {lost} of 200 rays differ from brute force without the margins, {kept} with them")
    assert kept == 0 and lost > 0


# ---- visibility -----------------------------------------------------------------------------------------------------------------

def test_the_visibility_restatement_stays_under_the_ambiguous_cap():
    """The cases tests/test_meshray_gpu.py runs: at most 0.5 % of a case's (point, eye) pairs have a hit within 2^-18 of the cut;
    a point on the far side of the sphere is hidden from an outside eye, one on the near side is seen once its own face is
    skipped; non-finite points see nothing."""
    for name, (V, F, P, skip, eyes, shrink) in sorted(MC.visibility_cases().items()):
        seen, amb = RR.visibility(P, eyes, V, F, skip, shrink)
        share = amb.mean()
        print(f"meshray visibility {name}: {len(P)} x {len(eyes)} pairs, {100 * share:.3f} % ambiguous, "
              f"{int(_mask_bits(seen, len(eyes)).sum())} visible")
        assert share <= AMBIGUOUS_CAP, name
        fin = np.isfinite(P).all(1)
        assert np.all(seen[~fin] == 0)
        if len(eyes) < 64:
            assert np.all(seen >> len(eyes) == 0)
        if name == "icosphere, own faces skipped":
            vis = _mask_bits(seen, len(eyes))
            # (the outward normal is the point itself, within 4 degrees)
            facing = (P.astype(np.float64) * (eyes[0].astype(np.float64) - P)).sum(1)
            assert np.all(vis[facing > 0.3, 0]) and not np.any(vis[facing < -0.3, 0]) and (np.abs(facing) > 0.3).sum() > 200
            assert np.all(vis[:, 3])                                                             # the eye at the centre sees every sample
        if name == "icosphere, nothing skipped":
            facing = (P.astype(np.float64) * (eyes[0] - P)).sum(1)
            assert not np.any(_mask_bits(seen, len(eyes))[:, 0] & (facing < -0.5))          # (a shrink of 2^-6 lets grazing rays through)


def _mask_bits(seen, E):
    return ((np.asarray(seen, np.int64)[:, None] >> np.arange(E, dtype=np.int64)[None, :]) & 1).astype(bool)


def test_pixel_rays_restated():
    """The restated pixel rays follow `depthsurface`'s convention: the ray of pixel (y, x) passes through the back-projection of
    that pixel at any depth, and its t is that depth."""
    from tests import depthsurface_cases as DC
    from tests import depthsurface_restate as DR
    c = DC.sphere4()
    k, pose = DR.cameras(c["ixt"], c["c2w"])
    o, d = RR.pixel_rays(k, pose, 24, 32)
    P = DR.points_map(c["depth"], k, pose, np.float64)[0]
    reach = o.astype(np.float64) + c["depth"].astype(np.float64)[..., None] * d.astype(np.float64)
    ok = c["mask"] != 0
    assert ok.sum() > 1000 and np.abs(reach - P)[ok].max() < 1e-6


# ---- hooks ----------------------------------------------------------------------------------------------------------------------

def test_score_dict_with_the_occlusion_count_reaches_the_evaluator():
    s = {"accuracy": 0.01, "completeness": 0.03, "chamfer": 0.04, "chamfer_sq": 0.0016, "normal_consistency": 0.9,
         "thresholds": [0.01, 0.02], "precision": [0.5, 1.0], "recall": [0.25, 0.5], "fscore": [1.0 / 3.0, 2.0 / 3.0], "n_pred": 10,
         "n_gt": 10, "fallbacks": 0, "n_pred_observed": 6, "n_pred_unobserved": 4}
    plain, occluded = evaluate.Evaluator(4), evaluate.Evaluator(4)
    plain.add_geometry("a", dict(s))
    occluded.add_geometry("a", dict(s, n_pred_self_occluded=3))
    assert plain.summary() == occluded.summary()
