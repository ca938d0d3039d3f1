"""include/lara_meshtopo.h without a GPU: the header's constants held to the module's, the library's and the module's refusals;
the facts of the restatement (tests/meshtopo_restate.py) on the meshes of tests/meshtopo_cases.py -- Euler characteristics, boundary,
flipped and non-manifold edges, the 4 096 copies; the two host entries, which run csrc/meshtopo_ops.h, equal to the restatement AS BIT
PATTERNS on every case, for both weightings and for lam / mu passes with and without fix_boundary; the smoothing teeth (Taubin keeps
the volume, Laplacian loses it); invariance under a permutation of the triangles; `Evaluator.add_topology` and the new keywords of
`MeshExtractor.extract`.  tests/test_meshtopo_gpu.py holds the kernels to the same restatement.

There is no tolerance in this file except the three bounds of the smoothing teeth, which are properties, not parities."""
import json
import os
import sys

import numpy as np
import pytest

from lara_amd import _native, evaluate
from tests import meshtopo_cases as C
from tests import meshtopo_restate as S

F32 = np.float32


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.int32)


def test_header_constants_equal_the_modules():
    from lara_amd import meshtopo
    from tests import test_abi_cpu as abi
    text = open(os.path.join(abi.ROOT, "include", "lara_meshtopo.h")).read()
    assert "#define LARA_MESHTOPO_SENTINEL 0x7fffffffffffffffll\n" in text and meshtopo.SENTINEL == 0x7fffffffffffffff
    assert f"#define LARA_MESHTOPO_REPORT {len(meshtopo.REPORT_FIELDS)}\n" in text and meshtopo.REPORT_FIELDS == S.REPORT_FIELDS
    assert f"#define LARA_MESHTOPO_CSR_NEIGHBORS {meshtopo.CSR_NEIGHBORS}\n" in text
    assert f"#define LARA_MESHTOPO_CSR_FACES {meshtopo.CSR_FACES}\n" in text
    assert f"#define LARA_MESHTOPO_WEIGHT_AREA {meshtopo.WEIGHTINGS['area']}\n" in text and meshtopo.WEIGHTINGS["area"] == S.AREA
    assert f"#define LARA_MESHTOPO_WEIGHT_UNIFORM {meshtopo.WEIGHTINGS['uniform']}\n" in text and meshtopo.WEIGHTINGS["uniform"] == S.UNIFORM
    for i, field in enumerate(S.REPORT_FIELDS):                       # the header's own list of the row
        assert f"out[{i}] {field}" in text, field


def test_the_unit_is_built_without_contraction():
    text = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "Makefile")).read()
    assert "FLAGS_meshtopo := -ffp-contract=off\n" in text and " meshtopo)" in text


def test_library_refusals(hip_lib):
    """Negative sizes, 3 T or n of 2^31 and more, unknown modes and weightings and null pointers come back as LARA2DGS_E_INVALID
    (-1) from host code, before any pointer is used; a zero-sized call is a no-op that launches nothing."""
    L = hip_lib
    big = (1 << 31) // 3 + 1
    keys = L.lara_meshtopo_halfedge_keys
    assert keys(-1, 1, 1, 1, 1, None) == -1 and keys(4, -1, 1, 1, 1, None) == -1 and keys(4, big, 1, 1, 1, None) == -1
    assert keys(4, 0, None, None, None, None) == 0
    for hole in range(3):
        args = [1, 1, 1]
        args[hole] = None
        assert keys(4, 2, *args, None) == -1
    corner = L.lara_meshtopo_corner_keys
    assert corner(-1, 1, 1, 1, None) == -1 and corner(4, big, 1, 1, None) == -1 and corner(4, 0, None, None, None) == 0
    assert corner(4, 2, None, 1, None) == -1 and corner(4, 2, 1, None, None) == -1
    heads = L.lara_meshtopo_edge_heads
    assert heads(-1, 1, 1, None) == -1 and heads(1 << 31, 1, 1, None) == -1 and heads(0, None, None, None) == 0
    assert heads(6, None, 1, None) == -1 and heads(6, 1, None, None) == -1
    rows = L.lara_meshtopo_edge_rows
    assert rows(-3, 0, *[1] * 10, None) == -1 and rows(1 << 31, 1, *[1] * 10, None) == -1 and rows(7, 1, *[1] * 10, None) == -1
    assert rows(6, 7, *[1] * 10, None) == -1 and rows(6, -1, *[1] * 10, None) == -1 and rows(0, 0, *[None] * 10, None) == 0
    for hole in range(10):
        args = [1] * 10
        args[hole] = None
        assert rows(6, 2, *args, None) == -1, hole
    report = L.lara_meshtopo_report
    assert report(-1, 2, 1, *[1] * 6, None) == -1 and report(4, -1, 1, *[1] * 6, None) == -1 and report(4, big, 1, *[1] * 6, None) == -1
    assert report(4, 2, 7, *[1] * 6, None) == -1 and report(4, 2, -1, *[1] * 6, None) == -1
    for hole in range(6):
        args = [1] * 6
        args[hole] = None
        assert report(4, 2, 3, *args, None) == -1, hole
    boundary = L.lara_meshtopo_boundary_vertices
    assert boundary(-1, 1, 1, 1, 1, None) == -1 and boundary(4, -1, 1, 1, 1, None) == -1 and boundary(0, 0, None, None, None, None) == 0
    assert boundary(4, 2, None, 1, 1, None) == -1 and boundary(4, 2, 1, None, 1, None) == -1 and boundary(4, 2, 1, 1, None, None) == -1
    pairs = L.lara_meshtopo_pair_keys
    assert pairs(-1, 1, 1, None) == -1 and pairs(1 << 31, 1, 1, None) == -1 and pairs(0, None, None, None) == 0
    assert pairs(3, None, 1, None) == -1 and pairs(3, 1, None, None) == -1
    csr = L.lara_meshtopo_csr
    assert csr(-1, 2, 1, 0, 1, 1, None) == -1 and csr(4, -1, 1, 0, 1, 1, None) == -1 and csr(4, 2, 1, 2, 1, 1, None) == -1
    assert csr(4, 2, 1, -1, 1, 1, None) == -1 and csr(4, 2, None, 0, 1, 1, None) == -1 and csr(4, 2, 1, 0, None, 1, None) == -1
    assert csr(4, 2, 1, 1, 1, None, None) == -1 and csr(4, 0, None, 0, None, None, None) == -1
    normals = L.lara_meshtopo_vertex_normals
    assert normals(-1, 1, 1, 1, 1, 0, 1, 1, None) == -1 and normals(4, 1, 1, 1, 1, 2, 1, 1, None) == -1
    assert normals(4, 1, 1, 1, 1, -1, 1, 1, None) == -1 and normals(4, 1, 1, 1, 1, 0, 1, None, None) == -1
    smooth = L.lara_meshtopo_smooth_pass
    assert smooth(-1, 1, 2, 1, 1, 0.5, None, None) == -1 and smooth(0, None, None, None, None, 0.5, None, None) == 0
    assert smooth(4, None, 2, 1, 1, 0.5, None, None) == -1 and smooth(4, 1, None, 1, 1, 0.5, None, None) == -1
    assert smooth(4, 1, 2, None, 1, 0.5, None, None) == -1 and smooth(4, 8, 8, 1, 1, 0.5, None, None) == -1      # in place
    nh, sh = L.lara_meshtopo_normals_host, L.lara_meshtopo_smooth_host
    count = np.zeros(1, np.int64)
    assert nh(-1, 1, 1, 1, 1, 0, 1, count.ctypes.data) == -1 and nh(4, 1, 1, 1, 1, 3, 1, count.ctypes.data) == -1
    assert nh(4, 1, 1, 1, 1, 0, 1, None) == -1 and nh(4, None, 1, 1, 1, 0, 1, count.ctypes.data) == -1
    assert nh(4, 1, 1, None, 1, 0, 1, count.ctypes.data) == -1 and nh(4, 1, 1, 1, 1, 0, None, count.ctypes.data) == -1
    assert nh(0, None, None, None, None, 1, None, count.ctypes.data) == 0 and count[0] == 0
    assert sh(-1, 1, 2, 1, 1, 0.5, None) == -1 and sh(0, None, None, None, None, 0.5, None) == 0 and sh(4, 8, 8, 1, 1, 0.5, None) == -1
    assert sh(4, None, 2, 1, 1, 0.5, None) == -1 and sh(4, 1, None, 1, 1, 0.5, None) == -1 and sh(4, 1, 2, None, 1, 0.5, None) == -1


def test_module_refusals():
    """CPU tensors, wrong shapes, iterations < 0, lam / mu that are not finite and an unknown weighting."""
    import torch
    from lara_amd import meshtopo
    V, F = C.mesh("one_triangle")
    v, f = torch.from_numpy(V), torch.from_numpy(F)
    for fn in (lambda: meshtopo.MeshTopology(v, f), lambda: meshtopo.topology_report(v, f), lambda: meshtopo.vertex_normals(v, f),
               lambda: meshtopo.smooth_laplacian(v, f, 1), lambda: meshtopo.smooth_taubin(v, f, 1)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
    with pytest.raises(ValueError, match="weighting must be"):
        meshtopo.vertex_normals(v, f, weighting="angle")
    with pytest.raises(ValueError, match="iterations must be"):
        meshtopo.smooth_laplacian(v, f, -1)
    with pytest.raises(ValueError, match="iterations must be"):
        meshtopo.smooth_taubin(v, f, -2)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lam must be finite"):
            meshtopo.smooth_laplacian(v, f, 1, lam=bad)
        with pytest.raises(ValueError, match="lam must be finite"):
            meshtopo.smooth_taubin(v, f, 1, lam=bad)
        with pytest.raises(ValueError, match="mu must be finite"):
            meshtopo.smooth_taubin(v, f, 1, mu=bad)
    for vs, fs in (((4,), (2, 3)), ((4, 2), (2, 3)), ((4, 3), (6,)), ((4, 3), (2, 4)), ((4, 3, 1), (2, 3))):
        with pytest.raises(RuntimeError, match=r"expected vertices \[Nv,3\] and triangles \[T,3\]"):
            meshtopo.MeshTopology(torch.zeros(vs), torch.zeros(fs, dtype=torch.int64))
    # sizes beyond int32 indices, on tensors without storage
    for nv, nt in ((1 << 31, 4), (8, (1 << 31) // 3 + 1)):
        with pytest.raises(RuntimeError, match=r"Nv < 2\^31 and 3 T < 2\^31"):
            meshtopo.MeshTopology(torch.empty(nv, 3, device="meta"), torch.empty(nt, 3, dtype=torch.int64, device="meta"))
    src = open(meshtopo.__file__).read()
    assert "is_watertight" not in src
    assert "vertex-manifoldness" in meshtopo.__doc__ and "self-intersection" in meshtopo.__doc__


def test_the_package_does_not_import_meshtopo():
    """Opt-in: importing the package, the mesh path and the evaluator leaves `lara_amd.meshtopo` out."""
    import lara_amd
    saved = sys.modules.pop("lara_amd.meshtopo", None)
    vars(lara_amd).pop("meshtopo", None)
    try:
        from lara_amd import evaluate as _e, mesh as _m, meshio as _io, meshsign as _s      # noqa: F401
        assert "lara_amd.meshtopo" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["lara_amd.meshtopo"] = saved
            setattr(lara_amd, "meshtopo", saved)


# ---- the facts of the restatement -------------------------------------------------------------------------------------------------

def test_restatement_facts():
    r = C.case("icosphere")["report"]
    assert (r["n_referenced"], r["n_edges"], r["n_valid"], r["euler"]) == (642, 1920, 1280, 2) and r["is_closed"] and r["is_oriented"]
    assert r["n_manifold"] == 1920 and r["max_degree"] == 6 and r["n_boundary_vertices"] == 0 and r["n_degenerate"] == 0
    r = C.case("uv_sphere")["report"]
    assert (r["n_referenced"], r["n_edges"], r["n_valid"], r["euler"]) == (450, 1344, 896, 2) and r["is_closed"] and r["is_oriented"]
    assert r["max_degree"] == 64
    r = C.case("face_removed")["report"]
    assert r["euler"] == 1 and r["n_boundary"] == 3 and r["n_boundary_vertices"] == 3 and not r["is_closed"] and not r["is_oriented"]
    r = C.case("face_flipped")["report"]
    assert r["n_inconsistent"] == 3 and r["is_closed"] and not r["is_oriented"] and r["euler"] == 2
    r = C.case("extra_triangles")["report"]
    assert r["n_nonmanifold"] == 1 and not r["is_edge_manifold"] and not r["is_closed"] and r["n_boundary"] == 4
    r = C.case("unreferenced")["report"]
    assert r["n_vertices"] == 647 and r["n_referenced"] == 642 and r["euler"] == 2 and r["is_oriented"]
    c = C.case("copies_4096")
    assert c["topo"].edges.tolist() == [[0, 1], [0, 2], [1, 2]] and c["topo"].edge_n.tolist() == [4096] * 3
    assert c["topo"].edge_face.tolist() == [[0, 1]] * 3 and c["topo"].edge_fwd.tolist() == [4096, 0, 4096]
    assert c["report"]["n_nonmanifold"] == 3 and c["report"]["max_degree"] == 2
    r = C.case("degenerate")["report"]
    assert r["n_degenerate"] == 19 and r["n_valid"] == 257 - 19 and r["n_edges"] == 3 * r["n_valid"] == r["n_boundary"]
    c = C.case("bad_triangles")
    assert c["topo"].bad and c["report"]["n_valid"] == 61 and not C.case("degenerate")["topo"].bad
    r = C.case("fan_300")["report"]
    assert r["max_degree"] == 300 and r["n_boundary"] == 300 and r["n_manifold"] == 300 and r["euler"] == 1
    r = C.case("soup_257")["report"]
    assert r["n_vertices"] == 771 and r["n_edges"] == 771 and r["euler"] == 257
    r = C.case("one_triangle")["report"]
    assert (r["n_edges"], r["n_boundary"], r["euler"], r["is_closed"]) == (3, 3, 1, False)
    r = C.case("no_triangle")["report"]
    assert (r["n_edges"], r["n_valid"], r["euler"], r["is_closed"], r["is_edge_manifold"]) == (0, 0, 0, False, True)
    for key in ("icosphere", "uv_sphere", "face_flipped"):
        assert C.case(key)["topo"].n_components() == 1
    assert C.case("soup_257")["topo"].n_components() == 257 and C.case("extra_triangles")["topo"].n_components() == 1


@pytest.mark.parametrize("key", C.CASES)
def test_restated_tables_are_consistent(key):
    """The tables agree with each other and with a plain loop over the triangles (independent of the vectorised restatement)."""
    c = C.case(key)
    topo, F = c["topo"], c["F"]
    edges = {}
    for t, (a, b, d) in enumerate(F.tolist()):
        if topo.kind[t] != 2:
            assert topo.tri_edge[t].tolist() == [-1, -1, -1]
            continue
        for k, (u, w) in enumerate(((a, b), (b, d), (d, a))):
            edges.setdefault((min(u, w), max(u, w)), []).append((t, u < w, k))
    assert [tuple(e) for e in topo.edges.tolist()] == sorted(edges)
    for e, key2 in enumerate(sorted(edges)):
        inc = edges[key2]
        assert topo.edge_n[e] == len(inc) and topo.edge_fwd[e] == sum(f for _, f, _ in inc)
        assert topo.edge_face[e].tolist() == (sorted(t for t, _, _ in inc) + [-1])[:2]
        assert all(topo.tri_edge[t, k] == e for t, _, k in inc)
    (vo, vn), (fo, ff) = c["vv"], c["vf"]
    assert vo[0] == 0 and vo[-1] == 2 * topo.E == len(vn) and fo[0] == 0 and fo[-1] == 3 * topo.n_valid == len(ff)
    for v in range(0, len(c["V"]), max(1, len(c["V"]) // 97)):
        row = vn[vo[v]:vo[v + 1]].tolist()
        assert row == sorted({w for (a, b) in edges for w in ((b,) if a == v else (a,) if b == v else ())})
        frow = ff[fo[v]:fo[v + 1]]
        assert frow[:, 0].tolist() == sorted(frow[:, 0].tolist()) and all(F[t, k] == v for t, k in frow.tolist())
    assert c["report"]["max_degree"] == (int(np.diff(vo).max()) if len(c["V"]) else 0)


# ---- the host entries -------------------------------------------------------------------------------------------------------------

def _host_normals(hip_lib, V, F, offsets, faces, weighting):
    V, F = np.ascontiguousarray(V, F32), np.ascontiguousarray(F, np.int32)
    offsets, faces = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(faces, np.int32)
    out, count = np.full((len(V), 3), 7.0, F32), np.full(1, -1, np.int64)
    assert hip_lib.lara_meshtopo_normals_host(len(V), V.ctypes.data, F.ctypes.data if len(F) else None, offsets.ctypes.data,
                                              faces.ctypes.data if len(faces) else None, weighting, out.ctypes.data, count.ctypes.data) == 0
    return out, int(count[0])


def _host_smooth(hip_lib, X, offsets, neighbors, steps, fixed=None):
    offsets, neighbors = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(neighbors, np.int32)
    fixed = None if fixed is None else np.ascontiguousarray(fixed, np.int32)
    X = np.ascontiguousarray(X, F32)
    for s in steps:
        out = np.full_like(X, 7.0)
        assert hip_lib.lara_meshtopo_smooth_host(len(X), X.ctypes.data, out.ctypes.data, offsets.ctypes.data,
                                                 neighbors.ctypes.data if len(neighbors) else None, float(s),
                                                 None if fixed is None else fixed.ctypes.data) == 0
        X = out
    return X


@pytest.mark.parametrize("key", C.CASES)
def test_host_entries_equal_the_restatement_as_bits(hip_lib, key):
    c = C.case(key)
    for w in (S.AREA, S.UNIFORM):
        got, zero = _host_normals(hip_lib, c["V"], c["F"], c["vf"][0], c["vf"][1], w)
        want, want_zero = c["normals"][w]
        assert np.array_equal(bits(got), bits(want)) and zero == want_zero, (key, w)
        unit = np.linalg.norm(got.astype(np.float64), axis=1)
        assert np.all((np.abs(unit - 1) < 1e-6) | (unit == 0) | np.isnan(unit))
    for (name, fix), want in c["smooth"].items():
        fixed = c["topo"].boundary_vertices() if fix else None
        got = _host_smooth(hip_lib, c["V"], c["vv"][0], c["vv"][1], C.STEPS[name], fixed)
        assert np.array_equal(bits(got), bits(want)), (key, name, fix)
    name = key.partition("/")[0]
    if name in ("face_removed", "fan_300", "one_triangle"):          # fix_boundary holds the boundary, and moves the rest
        b = c["topo"].boundary_vertices() == 1
        moved = (bits(c["smooth"][("taubin_10", True)]) != bits(c["V"])).any(1)
        assert b.sum() == c["report"]["n_boundary_vertices"] > 0 and not moved[b].any()
        assert (name != "face_removed" or moved[~b].mean() > 0.9) and (bits(c["smooth"][("pass", False)]) != bits(c["V"])).any(1)[b].any()
    if name in ("unreferenced", "no_triangle"):                      # a vertex without a neighbour keeps its bits, and has no normal
        lone = np.diff(c["vv"][0]) == 0
        assert lone.sum() == (5 if name == "unreferenced" else 3)
        assert np.array_equal(bits(c["smooth"][("taubin_10", False)])[lone], bits(c["V"])[lone])
        assert c["normals"][S.AREA][1] == lone.sum() and not c["normals"][S.AREA][0][lone].any()
    if name == "degenerate":                                         # collinear triangles with distinct indices: valid, without area
        assert c["normals"][S.AREA][1] > 0 and c["normals"][S.UNIFORM][1] == c["normals"][S.AREA][1]


def test_uniform_and_area_weights_differ_where_they_should():
    """On the UV sphere the pole's faces are equal, so both weightings give the axis; on a ring vertex, whose faces have unequal
    areas, the two differ."""
    c = C.case("uv_sphere")
    a, u = c["normals"][S.AREA][0], c["normals"][S.UNIFORM][0]
    assert np.allclose(a[0], [0, 0, 1], atol=1e-6) and np.allclose(u[0], [0, 0, 1], atol=1e-6)
    assert (bits(a) != bits(u)).any() and np.abs(a - u).max() < 0.05
    assert np.all(np.sum(a.astype(np.float64) * c["V"], 1) > 0.99)         # outward, along the position on a unit sphere


# ---- smoothing teeth -----------------------------------------------------------------------------------------------------------------

def test_taubin_keeps_the_volume_and_laplacian_loses_it(hip_lib):
    V, F = C.noisy_icosphere()
    topo = S.Topology(len(V), F)
    offsets, neighbors = topo.vertex_neighbors()
    taubin = _host_smooth(hip_lib, V, offsets, neighbors, [0.5, -0.53] * 10)
    laplacian = _host_smooth(hip_lib, V, offsets, neighbors, [0.5] * 10)
    assert np.array_equal(bits(taubin), bits(S.smooth_taubin(V, topo, 10))) and np.array_equal(bits(laplacian), bits(S.smooth_laplacian(V, topo, 10)))
    v0, vt, vl = S.volume(V, F), S.volume(taubin, F), S.volume(laplacian, F)
    spread = lambda X: float(np.linalg.norm(X.astype(np.float64), axis=1).std())
    s0, st = spread(V), spread(taubin)
    print(f"meshtopo smoothing: volume {v0:.4f} -> {vt:.4f} Taubin ({100 * (vt / v0 - 1):+.1f} %), {vl:.4f} Laplacian "
          f"({100 * (vl / v0 - 1):+.1f} %); radii spread {s0:.5f} -> {st:.5f} Taubin ({st / s0:.2f} of the start)")
    assert abs(vt / v0 - 1) < 0.02
    assert st < 0.5 * s0
    assert vl < 0.9 * v0


# ---- invariance ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(C.BASE))
def test_a_permutation_of_the_triangles_changes_nothing_it_should_not(name):
    a, b = C.case(name), C.case(name + "/permuted")
    if len(a["F"]) > 1 and name != "copies_4096":
        assert not np.array_equal(a["F"], b["F"])
    for field in ("edges", "edge_n", "edge_fwd"):
        assert np.array_equal(getattr(a["topo"], field), getattr(b["topo"], field)), field
    assert a["report"] == b["report"]
    assert np.array_equal(a["vv"][0], b["vv"][0]) and np.array_equal(a["vv"][1], b["vv"][1])
    for k in a["smooth"]:
        assert np.array_equal(bits(a["smooth"][k]), bits(b["smooth"][k])), k
    for w in (S.AREA, S.UNIFORM):                                      # another order of the faces: the last bit may differ
        assert a["normals"][w][1] == b["normals"][w][1]
        assert np.allclose(a["normals"][w][0], b["normals"][w][0], atol=1e-6, equal_nan=True)


# ---- hooks --------------------------------------------------------------------------------------------------------------------------

def test_add_topology_writes_its_keys_and_nothing_without_it(tmp_path):
    def make(topology):
        e = evaluate.Evaluator(4)
        e.add_scores("a", 30.0, 0.9, None, 0.1, 0.2)
        e.add_scores("b", 20.0, 0.8, None, 0.3, 0.4)
        e.add_volume("a", {"volume_iou": 0.5})
        for name, key in topology:
            e.add_topology(name, C.case(key)["report"])
        return e
    plain, with_topology = make([]), make([("a", "icosphere"), ("b", "face_removed")])
    assert not any(k.startswith("topology") for k in plain.summary())
    plain.write(str(tmp_path / "plain.json"))
    with_topology.write(str(tmp_path / "topology.json"))
    a, b = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "topology.json"))
    assert list(b)[:len(a)] == list(a) and {k: b[k] for k in a} == a
    assert list(b)[len(a):] == ["topology_name", "topology_closed", "topology_oriented", "topology_boundary_edges",
                                "topology_nonmanifold_edges", "topology_euler"]
    assert b["topology_name"] == ["a", "b"] and b["topology_closed"] == [True, False] and b["topology_oriented"] == [True, False]
    assert b["topology_boundary_edges"] == [0, 3] and b["topology_nonmanifold_edges"] == [0, 0] and b["topology_euler"] == [2, 1]
    assert list(a) == ["name", "psnr", "ssim", "lpips_vgg", "lpips_alex", "depth_acc", "psnr_mean", "ssim_mean", "lpips_vgg_mean",
                       "lpips_alex_mean", "volume_name", "volume_iou", "volume_iou_mean"]
    assert open(tmp_path / "plain.json").read() == json.dumps(plain.summary(), indent=4)
    only = evaluate.Evaluator(4)
    assert only.summary() is None
    only.add_topology("a", C.case("face_flipped")["report"])
    assert only.summary() == {"topology_name": ["a"], "topology_closed": [True], "topology_oriented": [False],
                              "topology_boundary_edges": [0], "topology_nonmanifold_edges": [0], "topology_euler": [2]}


def test_extract_refuses_its_new_keywords_where_stated(tmp_path):
    """The checks run before anything is rendered: an extractor without a scene is enough."""
    import inspect
    from lara_amd import mesh
    saved = sys.modules.pop("lara_amd.meshtopo", None)
    try:
        ex = mesh.MeshExtractor.__new__(mesh.MeshExtractor)
        ply, obj = str(tmp_path / "m.ply"), str(tmp_path / "m.obj")
        with pytest.raises(ValueError, match='normals=True needs writer="device"'):
            ex.extract(ply, "gso", cams=[], normals=True)
        with pytest.raises(ValueError, match='normals=True needs writer="device"'):
            ex.extract(ply, "gso", cams=[], normals=True, writer="host")
        with pytest.raises(ValueError, match="OBJ output takes no normals"):
            ex.extract(obj, "gso", cams=[], normals=True, writer="device")
        with pytest.raises(ValueError, match="smooth_method is"):
            ex.extract(obj, "gso", cams=[], smooth_iterations=3, smooth_method="cotangent")
        with pytest.raises(ValueError, match="smooth_iterations must be"):
            ex.extract(obj, "gso", cams=[], smooth_iterations=-1)
        with pytest.raises(ValueError, match="smooth_iterations must be"):
            ex.extract(obj, "gso", cams=[], smooth_iterations=3, smooth_lambda=float("nan"))
        with pytest.raises(ValueError, match="smooth_iterations must be"):
            ex.extract(obj, "gso", cams=[], smooth_iterations=3, smooth_mu=float("inf"))
        assert "lara_amd.meshtopo" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["lara_amd.meshtopo"] = saved
    p = inspect.signature(mesh.MeshExtractor.extract).parameters
    assert [p[k].default for k in ("smooth_iterations", "smooth_method", "smooth_lambda", "smooth_mu", "normals")] == \
        [None, "taubin", 0.5, -0.53, False]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("smooth_iterations", "smooth_method", "normals"))
