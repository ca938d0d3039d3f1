"""csrc/meshtopo.hip held to the restatement of its header (tests/meshtopo_restate.py) on every case of tests/meshtopo_cases.py, no
case exempt: the edge table, `tri_edge`, the report row, both CSR tables and the zero counts AS INTEGERS; vertex normals for both
weightings and the smoothed positions -- one pass with lam and with mu, 3 Laplacian iterations, 10 Taubin iterations, each with and
without `fix_boundary` -- AS int32 BIT PATTERNS, with no tolerance: the arithmetic is + - * / sqrt in double under -ffp-contract=off
with one final rounding, so a difference is a bug in the order or the build flags, not noise.  Two calls give the same bits, a side
stream gives the default stream's bits, T = 0 and T = 1 give well-formed tables, the mesh with an index out of range raises, a .ply
written by `MeshExtractor.extract(normals=True)` reads back with `vertex_normals`, and both spheres have one component and genus 0."""
import numpy as np
import pytest
import torch

from tests import meshtopo_cases as C
from tests import meshtopo_restate as S

pytestmark = pytest.mark.gpu
F32 = np.float32
WEIGHTS = {"area": S.AREA, "uniform": S.UNIFORM}


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a, order="C")).to(_dev(), dtype)          # (a copy: the cases are read-only)


def _np(x):
    return x.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.int32)


_built = {}


def _topo(key):
    """One device build per case, shared by the tests."""
    from lara_amd import meshtopo
    if key not in _built:
        c = C.case(key)
        _built[key] = meshtopo.MeshTopology(_t(c["V"]), _t(c["F"]))
    return _built[key]


def _smoothed(topo, name, fix):
    steps = C.STEPS[name]
    if name.startswith("taubin"):
        return topo.smooth_taubin(len(steps) // 2, steps[0], steps[1], fix_boundary=fix)
    if name == "pass_mu":
        return topo.smooth_laplacian(1, steps[0], fix_boundary=fix)
    return topo.smooth_laplacian(len(steps), steps[0], fix_boundary=fix)


@pytest.mark.parametrize("key", [k for k in C.CASES if k not in C.RAISES])
def test_every_output_equals_the_restatement(hip_lib, key):
    c, topo = C.case(key), _topo(key)
    want = c["topo"]
    i32 = torch.int32
    # the edge table
    assert (topo.n_edges, topo.n_valid, topo.n_vertices, topo.n_triangles) == (want.E, want.n_valid, len(c["V"]), len(c["F"]))
    for name in ("edges", "edge_n", "edge_fwd", "edge_face", "tri_edge"):
        got = getattr(topo, name)
        assert got.dtype == i32 and tuple(got.shape) == getattr(want, name).shape, name
        assert np.array_equal(_np(got), getattr(want, name)), (key, name)
    # the report
    assert topo.report_row().dtype == torch.int64 and topo.report_row().tolist() == want.report_row()
    assert topo.report() == c["report"]
    assert np.array_equal(_np(topo.boundary_vertices()), want.boundary_vertices())
    # the CSR tables
    (vo, vn), (fo, ff) = topo.vertex_neighbors(), topo.vertex_faces()
    assert vo.dtype == fo.dtype == torch.int64 and vn.dtype == ff.dtype == i32
    assert tuple(vn.shape) == (2 * want.E,) and tuple(ff.shape) == (3 * want.n_valid, 2)
    assert np.array_equal(_np(vo), c["vv"][0]) and np.array_equal(_np(vn), c["vv"][1]), key
    assert np.array_equal(_np(fo), c["vf"][0]) and np.array_equal(_np(ff), c["vf"][1]), key
    # the normals
    for name, w in WEIGHTS.items():
        n, zero = topo.vertex_normals(name, return_zero_count=True)
        assert n.dtype == torch.float32 and zero.dtype == torch.int64 and tuple(n.shape) == c["V"].shape
        assert np.array_equal(bits(_np(n)), bits(c["normals"][w][0])), (key, name, int((bits(_np(n)) != bits(c["normals"][w][0])).sum()))
        assert int(zero) == c["normals"][w][1], (key, name)
        again = topo.vertex_normals(name)
        assert torch.equal(again.view(i32), n.view(i32))
    # the smoothing
    before = topo.vertices.clone()
    for (name, fix), ref in c["smooth"].items():
        got = _smoothed(topo, name, fix)
        assert got.dtype == torch.float32 and got.data_ptr() != topo.vertices.data_ptr()
        assert np.array_equal(bits(_np(got)), bits(ref)), (key, name, fix, int((bits(_np(got)) != bits(ref)).sum()))
    assert torch.equal(before.view(i32), topo.vertices.view(i32))
    again = _smoothed(topo, "taubin_10", False)
    assert np.array_equal(bits(_np(again)), bits(c["smooth"][("taubin_10", False)]))
    assert torch.equal(topo.smooth_laplacian(0).view(i32), before.view(i32)) and torch.equal(topo.smooth_taubin(0).view(i32), before.view(i32))
    print(f"meshtopo {key}: {want.T} triangles, {want.n_valid} valid, {want.E} edges, max degree {c['report']['max_degree']}, "
          f"{c['normals'][S.AREA][1]} vertices without a normal")


def test_the_holed_icosphere_keeps_its_boundary(hip_lib):
    c, topo = C.case("face_removed"), _topo("face_removed")
    b = _np(topo.boundary_vertices()) == 1
    assert b.sum() == 3 and sorted(np.nonzero(b)[0].tolist()) == sorted(C.icosphere()[1][0].tolist())
    for name in C.STEPS:
        got = bits(_np(_smoothed(topo, name, True)))
        assert np.array_equal(got[b], bits(c["V"])[b]) and (got[~b] != bits(c["V"])[~b]).any(1).mean() > 0.9
        assert (bits(_np(_smoothed(topo, name, False)))[b] != bits(c["V"])[b]).any()


def test_an_index_out_of_range_raises(hip_lib):
    from lara_amd import meshtopo
    for key in C.RAISES:
        V, F = C.mesh(key)
        assert C.case(key)["topo"].bad
        with pytest.raises(RuntimeError, match=r"outside \[0, Nv\)"):
            meshtopo.MeshTopology(_t(V), _t(F))
        with pytest.raises(RuntimeError, match=r"outside \[0, Nv\)"):
            meshtopo.smooth_taubin(_t(V), _t(F), 1)


def test_wrong_shapes_are_refused_on_the_device(hip_lib):
    from lara_amd import meshtopo
    with pytest.raises(RuntimeError, match=r"expected vertices \[Nv,3\] and triangles \[T,3\]"):
        meshtopo.MeshTopology(torch.zeros(4, 2, device=_dev()), torch.zeros(2, 3, dtype=torch.int64, device=_dev()))
    topo = _topo("icosphere")
    with pytest.raises(RuntimeError, match="as many vertices"):
        topo.vertex_normals(vertices=torch.zeros(5, 3, device=_dev()))
    with pytest.raises(ValueError, match="weighting must be"):
        topo.vertex_normals("angle")
    with pytest.raises(ValueError, match="iterations must be"):
        topo.smooth_taubin(-1)


def test_empty_and_single_triangle_tables_are_well_formed(hip_lib):
    topo = _topo("no_triangle")
    assert tuple(topo.edges.shape) == (0, 2) and tuple(topo.edge_face.shape) == (0, 2) and tuple(topo.tri_edge.shape) == (0, 3)
    assert topo.edge_n.numel() == topo.edge_fwd.numel() == 0
    (vo, vn), (fo, ff) = topo.vertex_neighbors(), topo.vertex_faces()
    assert vo.tolist() == [0, 0, 0, 0] and fo.tolist() == [0, 0, 0, 0] and tuple(vn.shape) == (0,) and tuple(ff.shape) == (0, 2)
    n, zero = topo.vertex_normals(return_zero_count=True)
    assert not n.any() and int(zero) == 3
    assert topo.report(components=True)["n_components"] == 0 and "genus" not in topo.report(components=True)
    assert torch.equal(topo.smooth_taubin(3).view(torch.int32), topo.vertices.view(torch.int32))
    one = _topo("one_triangle")
    assert one.edges.tolist() == [[0, 1], [0, 2], [1, 2]] and one.edge_n.tolist() == [1, 1, 1] and one.edge_fwd.tolist() == [1, 0, 1]
    assert one.edge_face.tolist() == [[0, -1]] * 3 and one.tri_edge.tolist() == [[0, 2, 1]]
    assert one.vertex_neighbors()[1].tolist() == [1, 2, 0, 2, 0, 1] and one.vertex_faces()[1].tolist() == [[0, 0], [0, 1], [0, 2]]
    assert one.vertex_normals().tolist() == [[0.0, 0.0, 1.0]] * 3
    from lara_amd import meshtopo
    empty = meshtopo.MeshTopology(torch.zeros(0, 3, device=_dev()), torch.zeros(0, 3, dtype=torch.int64, device=_dev()))
    assert empty.report()["n_vertices"] == 0 and empty.vertex_neighbors()[0].tolist() == [0] and tuple(empty.vertex_normals().shape) == (0, 3)
    assert tuple(empty.smooth_laplacian(2).shape) == (0, 3)


def test_a_side_stream_gives_the_default_streams_bits(hip_lib):
    from lara_amd import meshtopo
    c = C.case("uv_sphere")
    V, F = _t(c["V"]), _t(c["F"])
    torch.cuda.synchronize()
    # (a high-priority stream: it is not drawn from the round of default-priority streams, and tests/test_stream_safety_gpu.py's
    # outcome depends on which of those it is handed -- with 4 hardware queues every fourth one runs behind the default stream)
    side = torch.cuda.Stream(_dev(), priority=-1)
    with torch.cuda.stream(side):
        topo = meshtopo.MeshTopology(V, F)
        normals = topo.vertex_normals("uniform")
        smooth = topo.smooth_taubin(10)
        row = topo.report_row()
    side.synchronize()
    ref = _topo("uv_sphere")
    assert torch.equal(topo.edges, ref.edges) and torch.equal(topo.edge_face, ref.edge_face) and torch.equal(topo.tri_edge, ref.tri_edge)
    assert row.tolist() == c["topo"].report_row()
    assert np.array_equal(bits(_np(normals)), bits(c["normals"][S.UNIFORM][0]))
    assert np.array_equal(bits(_np(smooth)), bits(c["smooth"][("taubin_10", False)]))


def test_the_one_shot_forms(hip_lib):
    from lara_amd import meshtopo
    c = C.case("icosphere")
    V, F = _t(c["V"]), _t(c["F"], torch.int32)
    assert meshtopo.topology_report(V, F) == c["report"]
    assert np.array_equal(bits(_np(meshtopo.vertex_normals(V, F, "uniform"))), bits(c["normals"][S.UNIFORM][0]))
    n, zero = meshtopo.vertex_normals(V, F, return_zero_count=True)
    assert np.array_equal(bits(_np(n)), bits(c["normals"][S.AREA][0])) and int(zero) == 0
    assert np.array_equal(bits(_np(meshtopo.smooth_laplacian(V, F, 3))), bits(c["smooth"][("laplacian_3", False)]))
    assert np.array_equal(bits(_np(meshtopo.smooth_taubin(V, F, 10))), bits(c["smooth"][("taubin_10", False)]))
    # the normals of other positions for the same triangles
    X = c["smooth"][("taubin_10", False)]
    want = S.vertex_normals(X, c["F"], c["vf"][0], c["vf"][1], S.AREA)[0]
    assert np.array_equal(bits(_np(_topo("icosphere").vertex_normals(vertices=_t(X)))), bits(want))


def test_smoothing_teeth_on_the_device(hip_lib):
    from lara_amd import meshtopo
    V, F = C.noisy_icosphere()
    topo = meshtopo.MeshTopology(_t(V), _t(F))
    taubin, laplacian = _np(topo.smooth_taubin(10)), _np(topo.smooth_laplacian(10, 0.5))
    rt = S.Topology(len(V), F)
    assert np.array_equal(bits(taubin), bits(S.smooth_taubin(V, rt, 10))) and np.array_equal(bits(laplacian), bits(S.smooth_laplacian(V, rt, 10)))
    v0, vt, vl = S.volume(V, F), S.volume(taubin, F), S.volume(laplacian, F)
    spread = lambda X: float(np.linalg.norm(X.astype(np.float64), axis=1).std())
    print(f"meshtopo smoothing on the device: volume {v0:.4f} -> {vt:.4f} Taubin, {vl:.4f} Laplacian; radii spread {spread(V):.5f} -> "
          f"{spread(taubin):.5f}")
    assert abs(vt / v0 - 1) < 0.02 and spread(taubin) < 0.5 * spread(V) and vl < 0.9 * v0


@pytest.mark.parametrize("key", ["icosphere", "uv_sphere"])
def test_components_and_genus_of_the_spheres(hip_lib, key):
    r = _topo(key).report(components=True)
    assert r["n_components"] == 1 and r["genus"] == 0 and r["is_oriented"] and r["euler"] == 2
    assert "n_components" not in _topo(key).report()


def test_components_of_other_meshes(hip_lib):
    for key in ("soup_257", "extra_triangles", "degenerate", "face_flipped"):
        r = _topo(key).report(components=True)
        assert r["n_components"] == C.case(key)["topo"].n_components(), key
        assert "genus" not in r


def test_extract_smooths_and_writes_normals(hip_lib, tmp_path):
    """On the scene and cameras of tests/test_meshclean_gpu.py's own extractor test: the smoothing runs between `clean_mesh` and the
    writer and is `smooth_taubin` of the cleaned mesh; the .ply carries `vertex_normals` of the written mesh."""
    from lara_amd import meshio, meshtopo
    from lara_amd.mesh import MeshExtractor, clean_mesh
    from lara_amd.renderer import Renderer
    from tests.test_meshclean_gpu import AABB, _scene_params, _turntable
    ex = MeshExtractor(_scene_params(), Renderer(sh_degree=1, white_background=True), AABB)
    ply = str(tmp_path / "mesh.ply")
    ex.timings = []
    v, t, c = ex.extract(ply, None, cams=_turntable(), writer="device", smooth_iterations=2, normals=True)
    marks = [name for name, _ in ex.timings]
    assert marks[-3:] == ["clean_mesh", "smooth", "write_obj"] and t.shape[0] > 5000
    assert ex.last_smooth_info["method"] == "taubin" and ex.last_smooth_info["iterations"] == 2 and ex.last_smooth_info["mu"] == -0.53
    v0, t0, c0, _ = clean_mesh(*ex.raw_mesh, aabb=ex.aabb_cfg, keep=10)
    assert torch.equal(t0, t) and torch.equal(c0, c)
    assert torch.equal(meshtopo.smooth_taubin(v0, t0, 2).view(torch.int32), v.view(torch.int32)) and not torch.equal(v0, v)
    rv, rt, rc, rn = meshio.read_ply(ply, return_normals=True)
    assert rv.tobytes() == _np(v).tobytes() and np.array_equal(rt, _np(t)) and rn is not None
    normals, zero = meshtopo.vertex_normals(v, t, return_zero_count=True)
    assert np.array_equal(bits(rn), bits(_np(normals)))
    unit = np.linalg.norm(rn.astype(np.float64), axis=1)
    assert int(zero) == int((unit == 0).sum()) < 0.01 * len(unit) and np.abs(unit[unit > 0] - 1).max() < 1e-6
    with pytest.raises(ValueError, match="OBJ output takes no normals"):
        ex.extract(str(tmp_path / "mesh.obj"), None, cams=_turntable(), writer="device", normals=True)
