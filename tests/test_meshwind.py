"""include/lara_meshwind.h without a GPU: the header's constants held to the module's, the library's and the module's refusals;
the term of csrc/solidangle.h, through its host entry, within 4 ulp of the float64 restatement (tests/meshwind_restate.py) and
exactly 0 wherever the restated `num == 0`; the host brute force within the summation bar of the restated one; analytic facts on
the two spheres and the cube; 4 096 copies; the flipped mesh; the holed icosphere, where the solid-angle rule decides every point
the crossing counts of `meshsign` disagree about; the `num == 0` rule shown to matter; the approximation error E(beta) of the
restated walk against float64 brute force, and the default band held to it; the restated walk at beta = inf against brute force;
`Evaluator.add_volume`.  tests/test_meshwind_gpu.py holds the kernels to the same restatement.

The lines that start with "meshwind parity:" are the ones profiles/meshwind_parity.txt records."""
import os
import sys

import numpy as np
import pytest

from lara_amd import _native, evaluate
from tests import meshbvh_cases as BC
from tests import meshdist_restate as R
from tests import meshsign_cases as SC
from tests import meshsign_restate as S
from tests import meshwind_cases as WC
from tests import meshwind_restate as W

F32 = np.float32
INF = float("inf")


def test_header_constants_equal_the_modules():
    from lara_amd import meshwind
    from tests import test_abi_cpu as abi
    text = open(os.path.join(abi.ROOT, "include", "lara_meshwind.h")).read()
    assert f"#define LARA_MESHWIND_SLOT_BYTES {meshwind.SLOT_BYTES}\n" in text and meshwind.SLOT_BYTES == W.SLOT_BYTES == 64
    assert f"#define LARA_MESHWIND_HEADER_BYTES {meshwind.HEADER_BYTES}\n" in text and meshwind.HEADER_BYTES == W.HEADER_BYTES
    assert repr(W.FOUR_PI) in text


def test_the_unit_is_built_without_contraction():
    text = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "Makefile")).read()
    assert "FLAGS_meshwind := -ffp-contract=off\n" in text and " meshwind " in text.split("OBJS")[1].splitlines()[0]


def test_refusals(hip_lib):
    """A beta that is zero, negative or NaN, a negative or NaN band, a NaN threshold, N of 2^30 and more, negative counts, a T the
    hierarchy refuses and null pointers come back as LARA2DGS_E_INVALID (-1) from host code, before any pointer is used; N = 0 is a
    no-op; python refuses the same values in the siblings' wording, CPU tensors, and a field used with another BVH."""
    import torch
    from lara_amd import meshbvh, meshwind
    L = hip_lib
    for T in (0, -1, 1 << 26):
        assert L.lara_meshwind_moments_bytes(T) == -1 and L.lara_meshwind_moments(T, 1, 1, None) == -1
    assert L.lara_meshwind_moments(5, None, 1, None) == -1 and L.lara_meshwind_moments(5, 1, None, None) == -1
    for T in (1, 8, 9, 64, 65, 1280, 4096):
        assert L.lara_meshwind_moments_bytes(T) == W.layout(T)[1]
    rows = L.lara_meshwind_rows
    for beta in (0.0, -2.0, float("nan"), -INF):
        assert rows(5, 1, 1, 1, beta, 1, None, None, None) == -1
    assert rows(-1, 1, 1, 1, 2.0, 1, None, None, None) == -1 and rows(1 << 30, 1, 1, 1, 2.0, 1, None, None, None) == -1
    assert rows(0, None, None, None, 2.0, None, None, None, None) == 0 and rows(0, None, None, None, INF, None, None, None, None) == 0
    for hole in range(4):
        args = [1, 1, 1, 1]
        args[hole] = None
        assert rows(5, args[0], args[1], args[2], 2.0, args[3], None, None, None) == -1
    classify = L.lara_meshwind_classify
    for band in (-0.01, float("nan")):
        assert classify(5, 1, 0.5, band, None, 1, 1, None, None) == -1
    assert classify(5, 1, float("nan"), 0.05, None, 1, 1, None, None) == -1
    assert classify(-1, 1, 0.5, 0.05, None, 1, 1, None, None) == -1 and classify(1 << 30, 1, 0.5, 0.05, None, 1, 1, None, None) == -1
    assert classify(0, None, 0.5, 0.05, None, None, None, None, None) == 0
    for hole in range(3):
        args = [1, 1, 1]
        args[hole] = None
        assert classify(5, args[0], 0.5, 0.05, None, args[1], args[2], None, None) == -1
    assert classify(5, 1, 0.5, 0.05, None, 1, 1, 1, None) == -1                       # an sdf without a dist
    solid = L.lara_meshwind_solid_host
    assert solid(-1, None, None, None) == -1 and solid(3, None, None, None) == -1 and solid(0, None, None, None) == 0
    brute = L.lara_meshwind_brute_host
    assert brute(-1, 1, 1, 1, 1) == -1 and brute(1 << 30, 1, 1, 1, 1) == -1 and brute(5, 1, -1, 1, 1) == -1
    assert brute(5, None, 1, 1, 1) == -1 and brute(5, 1, 1, None, 1) == -1 and brute(5, 1, 1, 1, None) == -1
    assert brute(0, None, 0, None, None) == 0
    P = torch.zeros(4, 3)
    for beta in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="beta must be"):
            meshwind.winding(None, P, beta=beta)
        with pytest.raises(ValueError, match="beta must be"):
            meshwind.volume_scores(None, None, beta=beta)
    for band in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="band must be"):
            meshwind.contains(None, P, band=band)
        with pytest.raises(ValueError, match="band must be"):
            meshwind.signed_distance(None, P, band=band)
    V, F = R.icosphere(0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshwind.contains(meshbvh.TriangleBVH(torch.from_numpy(V), torch.from_numpy(F)), P)
    with pytest.raises(TypeError, match="expected a meshbvh.TriangleBVH"):
        meshwind.WindingField((V, F))
    field = meshwind.WindingField.__new__(meshwind.WindingField)          # (a field as built for some hierarchy, without a device)
    field.bvh = object()
    with pytest.raises(RuntimeError, match="built for another BVH"):
        meshwind.winding(object(), P, field=field)
    with pytest.raises(RuntimeError, match="built for another BVH"):
        meshwind.contains(meshwind.WindingField.__new__(meshwind.WindingField), P, field=field)


def test_the_package_does_not_import_meshwind():
    """Opt-in: importing the package and its mesh modules leaves `lara_amd.meshwind` out."""
    import lara_amd
    saved = sys.modules.pop("lara_amd.meshwind", None)
    vars(lara_amd).pop("meshwind", None)
    try:
        from lara_amd import evaluate as _e, meshbvh, meshdist, meshray, meshsign      # noqa: F401
        assert "lara_amd.meshwind" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["lara_amd.meshwind"] = saved
            setattr(lara_amd, "meshwind", saved)


# ---- the term -------------------------------------------------------------------------------------------------------------------

def _host_solid(hip_lib, q, tri):
    n = len(q)
    q, tri = np.ascontiguousarray(q, F32), np.ascontiguousarray(np.asarray(tri, F32).reshape(n, 9))
    omega = np.empty(n)
    assert hip_lib.lara_meshwind_solid_host(n, q.ctypes.data, tri.ctypes.data, omega.ctypes.data) == 0
    return omega


def _host_brute(hip_lib, P, V, F):
    p0, p1, p2 = W.triangles(V, F)
    tri = np.ascontiguousarray(np.stack([p0, p1, p2], 1).reshape(-1, 9), F32)
    P = np.ascontiguousarray(P, F32)
    w = np.empty(len(P))
    assert hip_lib.lara_meshwind_brute_host(len(P), P.ctypes.data, len(tri), tri.ctypes.data if len(tri) else None, w.ctypes.data) == 0
    return w


def test_host_term_equals_the_restatement(hip_lib):
    """4 ulp of double on |Omega| (the libm's atan2 is the only operation that is not correctly rounded), and exactly 0 wherever
    the restated num == 0."""
    zeros = total = 0
    for name, (q, tri) in sorted(WC.term_pairs().items()):
        got = _host_solid(hip_lib, q, tri)
        want, num = W.solid(q, tri[:, 0], tri[:, 1], tri[:, 2], return_num=True)
        z = num == 0
        assert np.all(got[z] == 0.0) and not np.signbit(got[z]).any(), name
        assert np.all(np.isfinite(got)) and np.all(np.abs(got) <= 2 * np.pi), name
        ulp = np.abs(got - want) / np.spacing(np.abs(want))
        print(f"meshwind term, {name}: {len(q)} pairs, {int(z.sum())} with num == 0, worst {ulp.max():.2f} ulp, |Omega| up to "
              f"{np.abs(got).max():.4f}")
        assert ulp.max() <= 4.0, name
        zeros, total = zeros + int(z.sum()), total + len(q)
    assert zeros > 500 and total > 100000


def test_term_closed_forms(hip_lib):
    """One octant seen from the origin is 4 pi / 8; the flipped triangle gives the exact negative; a point on the face, beside it in
    its plane, at a vertex, and a triangle without area give exactly 0 -- where a bare atan2 gives 2 pi on the face."""
    tri = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]] * 6 + [[[1, 1, 1], [1, 1, 1], [2, 2, 2]]], F32)
    tri[1] = tri[1][[0, 2, 1]]
    q = np.array([[0, 0, 0], [0, 0, 0], [0.25, 0.25, 0.5], [2, -1, 0], [1, 0, 0], [1, 1, 1], [0.25, 0.125, 0.75]], F32)
    got = _host_solid(hip_lib, q, tri)
    assert abs(got[0] - np.pi / 2) < 1e-15 and got[1] == -got[0] and got[5] < 0
    assert got[2:5].tolist() == [0.0, 0.0, 0.0] and got[6] == 0.0
    bare = W.solid(q, tri[:, 0], tri[:, 1], tri[:, 2], rule=False)
    assert abs(abs(bare[2]) - 2 * np.pi) < 1e-15 and np.array_equal(W.solid(q, tri[:, 0], tri[:, 1], tri[:, 2]), got)


# ---- brute force ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", WC.KEYS)
def test_host_brute_force_equals_the_restatement(hip_lib, key):
    """Within (n + 4) 2^-53 sum |term| / 4 pi: the terms are the restatement's but for atan2's last bits, the order is id order in
    both, numpy adds pairwise.  NaN exactly on the points that are not finite; zeros for T = 0."""
    c = WC.case(key)
    w = _host_brute(hip_lib, c["P"], c["V"], c["F"])
    fin = np.isfinite(c["P"]).all(1)
    assert np.array_equal(np.isnan(w), ~fin) and (~fin).sum() == 3 and np.array_equal(np.isnan(c["w"]), ~fin)
    ratio = np.abs(w[fin] - c["w"][fin]) / np.maximum(W.bar(c["n_valid"], c["mag"][fin]), 1e-300)
    print(f"meshwind brute force {key}: {len(c['P'])} points x {c['n_valid']} triangles, w {np.nanmin(w):.4f} .. {np.nanmax(w):.4f}, "
          f"worst ratio to the bar {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    if c["n_valid"] == 0:
        assert np.all(w[fin] == 0.0)


def test_analytic_facts():
    """From the restatement: inside both spheres w = 1 and outside 0 (the issue's figures: 1 +- 2e-16, 0 +- 1e-16 on the icosphere;
    the bar here is the summation bar), the cube at its centre 1 and outside 0."""
    for key in ("icosphere", "uv_sphere"):
        c = WC.case(key)
        P, w = c["P"][:1500], c["w"][:1500]
        r = np.linalg.norm(P.astype(np.float64), axis=1)
        r_in = SC.inscribed_radius(c["V"], c["F"])
        ins, out = r < 0.95 * r_in, r > 1.05
        bar = W.bar(c["n_valid"], c["mag"][:1500])
        assert ins.sum() > 200 and out.sum() > 900
        assert np.all(np.abs(w[ins] - 1.0) <= bar[ins]) and np.all(np.abs(w[out]) <= bar[out])
        print(f"meshwind {key}: inscribed radius {r_in:.4f}; {int(ins.sum())} inside, |w - 1| up to {np.abs(w[ins] - 1).max():.2e}; "
              f"{int(out.sum())} outside, |w| up to {np.abs(w[out]).max():.2e}")
    V, F = SC.cube()
    Q = np.array([[0, 0, 0], [0.25, -0.125, 0.375], [2, 0, 0], [0.75, 0.75, 0.75], [0, 0, -0.625]], F32)
    w = W.brute(Q, V, F)[0]
    assert np.all(np.abs(w - [1, 1, 0, 0, 0]) < 1e-15)


def test_copies_and_the_flipped_mesh(hip_lib):
    """4 096 copies give 4 096 x the single triangle's value within the summation bar; a mesh with p1 and p2 of every triangle
    exchanged gives the exact negative, in the restatement and from the host entry."""
    c = WC.case("copies_4096")
    tri = np.asarray(c["V"], F32)[c["F"][0]]
    single = W.solid(c["P"], tri[0], tri[1], tri[2]) / W.FOUR_PI
    fin = np.isfinite(c["P"]).all(1)
    assert np.all(np.abs(c["w"][fin] - 4096 * single[fin]) <= W.bar(4096, c["mag"][fin]))
    assert np.abs(c["w"][fin]).max() > 1000 and np.all(c["w"][-6:-3] == 0.0) and np.all(c["w"][1500:1503] == 0.0)   # in its plane, at its vertices
    for key in ("icosphere", "holed_icosphere", "degenerate"):
        c = WC.case(key)
        flipped = np.asarray(c["F"])[:, [0, 2, 1]]
        w = W.brute(c["P"], c["V"], flipped)[0]
        fin = np.isfinite(c["P"]).all(1)
        assert np.array_equal(w[fin], -c["w"][fin]), key
        host = _host_brute(hip_lib, c["P"], c["V"], c["F"])
        assert np.array_equal(_host_brute(hip_lib, c["P"], c["V"], flipped)[fin], -host[fin]), key


# ---- teeth ----------------------------------------------------------------------------------------------------------------------

def test_the_holed_icosphere_is_decided_where_the_rays_disagree():
    """Every point with r < 0.5 has w > 0.5 on the icosphere with a tenth of it cut away, exactly and under every beta, while the
    restated parity vote of `meshsign` is not unanimous on a part of the same points: a ray through the hole counts one crossing
    fewer."""
    c = WC.case("holed_icosphere")
    assert len(c["F"]) == 1148
    r = np.linalg.norm(c["P"].astype(np.float64), axis=1)
    deep = np.nonzero(r < 0.5)[0]
    assert len(deep) > 30 and np.all(c["w"][deep] > 0.5)
    for beta in (2.0, 3.0, INF):
        assert np.all(WC.walked("holed_icosphere", beta)[0][deep] > 0.5)
    cross, wind = S.rows(c["P"][deep], 3, c["V"], c["F"])
    inside, status, _ = S.vote(cross, wind, S.PARITY)
    split = (status & 1) == 1
    print(f"meshwind parity: holed icosphere, {len(deep)} points with r < 0.5: solid angle decides {100.0 * (c['w'][deep] > 0.5).mean():.1f} % "
          f"as inside (w {c['w'][deep].min():.3f} .. {c['w'][deep].max():.3f}); meshsign's three rays are unanimous on "
          f"{100.0 * (1 - split.mean()):.1f} % and vote outside on {100.0 * (inside == 0).mean():.1f} %")
    assert split.sum() > 0
    seeded = c["w"][:1500]
    print(f"meshwind parity: holed icosphere, 1500 seeded points: {100.0 * (np.abs(seeded - 0.5) < 0.1).mean():.2f} % within 0.1 of 0.5")


def test_the_rule_on_num_has_teeth():
    """With a bare atan2 in the place of the rule, points ON a face move by +-0.5 (atan2(+-0, negative) = +-pi): on the cube, whose
    in-plane points are exact, and on the 4 096 copies, where the mistake is counted 4 096 times."""
    c = WC.case("cube")
    bare = W.brute(c["P"], c["V"], c["F"], rule=False)[0]
    fin = np.isfinite(c["P"]).all(1)
    moved = np.abs(bare[fin] - c["w"][fin])
    assert (np.abs(moved - 0.5) < 1e-12).sum() >= 12 and np.all((moved < 1e-12) | (np.abs(moved - 0.5) < 1e-12))
    on_face = c["w"][1500 + 8:1500 + 8 + 12]
    assert np.all(np.abs(on_face - 0.5) < 1e-12)          # a point on a face of a closed mesh sees half of it
    c = WC.case("copies_4096")
    bare = W.brute(c["P"][1503:1506], c["V"], c["F"], rule=False)[0]          # on the triangle, in its plane
    assert np.all(c["w"][1503:1506] == 0.0) and np.all(np.abs(np.abs(bare) - 2048.0) < 1e-9)


# ---- the walk -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", WC.KEYS)
def test_the_restated_walk_at_beta_inf_equals_brute_force(key):
    """The exact sum in tree order: every valid triangle outside flagged slots is tested once, no far node is accepted, and w is
    brute force's within the summation bar."""
    c = WC.case(key)
    w, n_tri, n_far, mag = WC.walked(key, INF)
    fin = np.isfinite(c["P"]).all(1)
    assert np.array_equal(np.isnan(w), ~fin) and np.all(n_far == 0) and np.all(n_tri[~fin] == 0)
    M = WC.moments(key)
    if M is None:
        assert np.all(w[fin] == 0.0) and not n_tri.any()
        return
    flagged_leaves = M.levels[0][:len(M.bvh.levels[0]), 3] == 0
    skipped = sum(int((M.bvh.rec_id[8 * j:8 * j + 8] >= 0).sum()) for j in np.nonzero(flagged_leaves)[0])
    assert np.all(n_tri[fin] == c["n_valid"] - skipped)
    ratio = np.abs(w[fin] - c["w"][fin]) / np.maximum(W.bar(c["n_valid"], np.maximum(mag, c["mag"])[fin]), 1e-300)
    print(f"meshwind restated walk {key}, beta inf: {c['n_valid']} valid triangles, {skipped} in flagged leaves, worst ratio to the bar "
          f"{ratio.max():.3f}")
    assert ratio.max() <= 1.0


def test_the_moments_restated():
    """Closed meshes have a zero dipole at the root up to rounding; the root's area is the mesh's; a slot without area is all zero;
    every centre lies in its box."""
    for key in ("icosphere", "cube", "degenerate", "copies_4096", "soup_1"):
        M = WC.moments(key)
        c = WC.case(key)
        root = M.levels[-1][0]
        area = S.volume(c["V"], c["F"])[1]
        assert abs(root[3] - area) <= 1e-12 * area and np.all(M.levels[-1][1:] == 0)
        if key in WC.CLOSED:
            assert np.abs(root[:3]).max() < 1e-12
        for k, lev in enumerate(M.levels):
            live = lev[:, 3] > 0
            assert np.all(lev[~live] == 0) and np.all(lev[live, 7] > 0)
            box = M.bvh.levels[k][np.nonzero(live)[0]].astype(np.float64)
            assert np.all(lev[live, 4:7] >= box[:, :3] - 1e-12) and np.all(lev[live, 4:7] <= box[:, 3:] + 1e-12)
        assert M.nbytes == W.HEADER_BYTES + W.SLOT_BYTES * len(M.flat)
    # 1 280 faces: 160 leaves under 20, 3 and 1 slots; 1 148: a ragged last leaf
    assert [len(b) for b in WC.moments("icosphere").bvh.levels] == [160, 20, 3, 1] and 1148 % 8 != 0


def test_the_approximation_error_and_the_default_band():
    """E(beta) = the largest |w_walk(beta) - w_brute64| of the restated walk over all cases, against float64 brute force.  The
    figure over ALL cases is the 4 096 copies' (2.4 at beta = 2: a point there sees up to 1 400 sheets of one surface, and the
    dipole's error is counted as often); over the cases that are surfaces (at most two sheets seen from any point) it is the UV
    sphere's 1.9e-2, the size the issue's prototype measured.  Both fall with beta.  The default band exceeds the surfaces' E(2);
    and on EVERY case, the copies included, a point outside the default band classifies the same under beta = 2, under
    beta = inf and by float64 brute force.  The share of a case's points within the margin of tests/meshwind_cases.margin -- the
    ones tests/test_meshwind_gpu.py exempts from the classification -- is capped at 2 %, every vertex and in-plane point counted."""
    from lara_amd import meshwind
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(meshwind.contains).parameters.items()}
    assert (defaults["beta"], defaults["threshold"], defaults["band"]) == (2.0, 0.5, 0.05)
    assert {k: v.default for k, v in inspect.signature(meshwind.volume_scores).parameters.items()}["band"] == 0.05
    errors = {beta: WC.approximation_error(beta) for beta in WC.BETAS}
    for key in WC.KEYS:
        print(f"meshwind parity: E on {key}: " + ", ".join(f"beta {beta:g}: {errors[beta][key][0]:.2e} ({errors[beta][key][1]:.2e} per sheet)"
                                                             for beta in WC.BETAS))
    surfaces = WC.surfaces()
    assert set(WC.KEYS) - set(surfaces) == {"copies_4096", "copies_4096 permuted"}
    E_all = {beta: WC.E(beta) for beta in WC.BETAS}
    E = {beta: WC.E(beta, surfaces) for beta in WC.BETAS}
    print("meshwind parity: E(beta), restated walk against float64 brute force, over all cases: "
          + ", ".join(f"E({beta:g}) = {E_all[beta]:.3e}" for beta in WC.BETAS) + "; over the surfaces (all but the 4 096 copies): "
          + ", ".join(f"E({beta:g}) = {E[beta]:.3e}" for beta in WC.BETAS))
    assert E[2.0] > E[3.0] > E[4.0] > 0 and E_all[2.0] > E_all[3.0] > E_all[4.0] and E[2.0] < defaults["band"]
    # the prototype's figures for the two spheres (1.2e-2 / 2.7e-3 / 8.5e-4 and 2.0e-2 / 8.1e-3 / 1.8e-3) are of this size
    assert 5e-3 < errors[2.0]["icosphere"][0] < 2.5e-2 and 1e-2 < errors[2.0]["uv_sphere"][0] < 4e-2
    for key in WC.KEYS:
        c = WC.case(key)
        w2, wi = WC.walked(key, 2.0)[0], WC.walked(key, INF)[0]
        decided = np.isfinite(w2) & ~(np.abs(w2 - 0.5) < defaults["band"])
        assert np.array_equal(w2[decided] > 0.5, wi[decided] > 0.5) and np.array_equal(w2[decided] > 0.5, c["w"][decided] > 0.5), key
        fin = np.isfinite(c["P"]).all(1)
        margin = WC.margin(key)
        assert np.all(margin <= 2.0 * E_all[2.0] * WC.multiplicity(key))
        exempt = fin & ~(np.abs(c["w"] - 0.5) > margin)
        assert exempt.sum() <= 0.02 * len(c["P"]), (key, int(exempt.sum()))
        print(f"meshwind parity: {key}: {100.0 * exempt.sum() / len(c['P']):.2f} % of {len(c['P'])} points within the margin of the "
              f"threshold, {100.0 * (fin & ~decided).sum() / len(c['P']):.2f} % inside the default band")


def test_the_walk_prunes():
    """On the spheres the default beta tests a fraction of the triangles; the counters add up to fewer visits than triangles."""
    for key in ("icosphere", "uv_sphere", "holed_icosphere"):
        c = WC.case(key)
        _, n_tri, n_far, _ = WC.walked(key, 2.0)
        fin = np.isfinite(c["P"]).all(1)
        assert n_tri[fin].mean() < 0.3 * c["n_valid"] and n_far[fin].mean() > 10
    assert WC.walked("icosphere", 3.0)[1].mean() > WC.walked("icosphere", 2.0)[1].mean()


def test_classification_restated():
    w = np.array([0.375, 0.4375, 0.5, 0.5625, 0.53125, 0.625, 1.0, np.nan, np.inf, -np.inf])          # (dyadic: the band's edge is exact)
    inside, status, sdf = W.classify(w, 0.5, 0.0625, np.full(10, 0.25, F32))
    assert inside.tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 1, 0]
    assert status.tolist() == [0, 0, 1, 0, 1, 0, 0, 4, 4, 4]
    assert sdf.tolist() == [0.25, 0.25, 0.25, -0.25, -0.25, -0.25, -0.25, 0.25, -0.25, 0.25]
    assert W.classify(w, 0.5, 0.0)[1].tolist() == [0] * 7 + [4] * 3
    assert S.counts(inside, status, inside, status) == [5, 5, 5, 5, 2, 2, 3, 3]      # the bits lara_meshsign_counts reads


# ---- hooks ----------------------------------------------------------------------------------------------------------------------

def test_add_volume_accepts_the_dict():
    """`volume_scores` returns `meshsign.volume_scores`' keys with decided_* in the place of unanimous_* (and its own three
    parameters); `Evaluator.add_volume` takes it as it is."""
    import inspect
    from lara_amd import meshsign, meshwind

    def keys(fn):      # the common part of the dict is meshsign.lattice_scores', the rule's own keys are added by `fn`
        src = inspect.getsource(meshsign.lattice_scores) + inspect.getsource(fn)
        return [k for k in ("volume_iou", "volume_pred", "volume_gt", "volume_pred_mesh", "volume_gt_mesh", "unanimous_pred", "unanimous_gt",
                            "decided_pred", "decided_gt", "n_lattice", "resolution", "rule", "rays", "counts") if f'"{k}":' in src]
    swap = {"unanimous_pred": "decided_pred", "unanimous_gt": "decided_gt"}
    assert [swap.get(k, k) for k in keys(meshsign.volume_scores)] == keys(meshwind.volume_scores) and len(keys(meshwind.volume_scores)) == 12
    scores = {"volume_iou": 0.75, "volume_pred": 4.0, "volume_gt": 4.1, "volume_pred_mesh": 4.15, "volume_gt_mesh": 4.15,
              "decided_pred": 0.97, "decided_gt": 1.0, "n_lattice": 4096, "resolution": 16, "rule": meshwind.RULE, "rays": 0,
              "counts": [1] * 8, "beta": 2.0, "threshold": 0.5, "band": 0.05}
    e = evaluate.Evaluator(4)
    e.add_volume("a", scores)
    e.add_volume("b", dict(scores, volume_iou=None))
    assert e.summary()["volume_name"] == ["a", "b"] and e.summary()["volume_iou"] == [0.75, None]
    assert meshwind.RULE == "solid_angle"
