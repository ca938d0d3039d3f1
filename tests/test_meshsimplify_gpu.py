"""lara_amd.meshsimplify on the device against the numpy restatement tests/meshsimplify_restate.py: integer outputs exactly,
"average" positions and colours bit for bit where the restatement's fp64 member sums are exact, "quadric" positions per coordinate
within one fp32 spacing, |out - ref64| <= spacing32(max(|ref64|, h)) (the fp64 solve at condition <= 1025 carries ~1e-12 relative
error: the bar is the one rounding to fp32), and the invariants of the contract on every case.

The tests print the worst |out - ref64| / bar and write it to test_out/meshsimplify_parity.txt (kept as
profiles/meshsimplify_parity.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import meshsimplify_restate as R
from tests.meshrender_cases import icosphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))
    out = os.path.join(ROOT, "test_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "meshsimplify_parity.txt"), "w") as f:
        f.write("worst observed |out - ref64| / bar of tests/test_meshsimplify_gpu.py (bar = 1 fails)\n")
        for k in sorted(_worst):
            f.write(f"{k}: {_worst[k]:.4f}\n")
    print(f"meshsimplify parity {key}: {ratio:.4f} of the bar")


def _colors(V):
    return np.random.default_rng(len(V)).random((len(V), 3)).astype(np.float32)


def _hip(V, F, C, h, mode="quadric", origin=None, remove_unreferenced=True):
    from lara_amd.meshsimplify import simplify_vertex_clustering
    v, f, c, info = simplify_vertex_clustering(torch.as_tensor(np.asarray(V, np.float32)).cuda(),
                                               torch.as_tensor(np.asarray(F, np.int64).reshape(-1, 3)).cuda(),
                                               None if C is None else torch.as_tensor(C).cuda(), h, mode, origin, remove_unreferenced)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and f.dtype == torch.int64 and info["vertex_cluster"].dtype == torch.int32
    return dict(V=v.cpu().numpy(), F=f.cpu().numpy(), C=None if c is None else c.cpu().numpy(),
                vertex_cluster=info["vertex_cluster"].cpu().numpy(), **{k: info[k] for k in COUNTERS})


COUNTERS = ("n_cells", "n_degenerate", "n_duplicate", "n_clamped", "n_zero_area")


def _invariants(V, d, ref, h):
    """6. every output vertex inside its cell box within one spacing32; every input vertex within sqrt(3) h (1 + 2^-20) of its
    cluster's vertex; no output triangle with a repeated index; no two equal oriented triples; every output vertex referenced."""
    out, F = d["V"].astype(np.float64), d["F"]
    slack = R.spacing32(np.maximum(np.abs(out), h))
    assert np.all(out >= ref["lo"] - slack) and np.all(out <= ref["hi"] + slack)
    vc = d["vertex_cluster"]
    used = vc >= 0
    dist = np.linalg.norm(np.asarray(V, np.float32).astype(np.float64)[used] - out[vc[used]], axis=1)
    assert np.all(dist <= np.sqrt(3.0) * h * (1 + 2.0 ** -20))
    assert np.all((F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2]))
    assert np.all(F[:, 0] < np.minimum(F[:, 1], F[:, 2])) if len(F) else True
    assert len(np.unique(F, axis=0)) == len(F)
    assert np.array_equal(np.unique(F), np.arange(len(out))) if len(F) else len(out) == 0


def _same(V, F, C, h, mode, origin=None, remove_unreferenced=True, name=None):
    """Integer outputs exactly, positions and colours to their bars, the invariants; returns (device, restatement)."""
    d = _hip(V, F, C, h, mode, origin, remove_unreferenced)
    ref = R.simplify(V, F, C, h, mode, origin, remove_unreferenced)
    np.testing.assert_array_equal(d["F"], ref["F"])
    np.testing.assert_array_equal(d["vertex_cluster"], ref["vertex_cluster"])
    for k in ("n_cells", "n_degenerate", "n_duplicate", "n_zero_area"):
        assert d[k] == ref[k], k
    h32 = float(np.float32(h))
    assert R.outside_count(ref, 1e-9 * h32) <= d["n_clamped"] <= R.outside_count(ref, -1e-9 * h32)
    assert d["V"].shape == ref["V"].shape
    bar = R.spacing32(np.maximum(np.abs(ref["x64"]), h32))
    diff = np.abs(d["V"].astype(np.float64) - ref["x64"])
    if mode == "average" and ref["sums_exact"]:
        np.testing.assert_array_equal(d["V"], ref["V"])
    else:
        if name is not None and diff.size:
            _note(f"{mode} {name}", (diff / bar).max())
        assert np.all(diff <= bar), (diff / bar).max()
    if C is not None and ref["colors_exact"]:
        np.testing.assert_array_equal(d["C"], ref["C"])
    elif C is not None:                                          # (an inexact fp64 sum: the order may show, far below the bar)
        assert np.all(np.abs(d["C"].astype(np.float64) - ref["c64"]) <= R.spacing32(ref["c64"]))
    if remove_unreferenced:
        _invariants(V, d, ref, h32)
    return d, ref


# ---- the meshes ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere(level):
    V, F = icosphere(level)
    return np.asarray(V, np.float32), np.asarray(F, np.int64)


def crowded(h=0.25, n=4097):
    """A hub and n rim vertices at radius 0.4 h in one cell (n + 1 members, 6 n corners), a second ring at 1.6 h across the
    neighbouring cells; origin (0, 0, 0), the hub at the centre of cell (4, 4, 4)."""
    c = np.array([4.5 * h] * 3)
    th = np.arange(n) * (2 * np.pi / n)
    rim = c + np.stack([0.4 * h * np.cos(th), 0.4 * h * np.sin(th), 0.05 * h * np.sin(3 * th)], 1)
    out = c + np.stack([1.6 * h * np.cos(th), 1.6 * h * np.sin(th), 0.2 * h * np.cos(2 * th)], 1)
    V = np.concatenate([c[None], rim, out]).astype(np.float32)
    i = np.arange(n)
    j = (i + 1) % n
    fan = np.stack([np.zeros(n, int), 1 + i, 1 + j], 1)
    return V, np.concatenate([fan, np.stack([1 + i, 1 + n + i, 1 + j], 1), np.stack([1 + j, 1 + n + i, 1 + n + j], 1)]).astype(np.int64)


def roof(n=48, step=0.0213, slope=0.35, ridge=0.4171):
    """Two slopes meeting in a ridge: in the cells beside the ridge's the minimiser of the quadric lies outside the cell."""
    V, F = R.flat_grid(n, step, 0.0)
    V = V.copy()
    V[:, 2] = (0.3 - slope * np.abs(V[:, 0].astype(np.float64) - ridge)).astype(np.float32)
    return V, F


# ---- 1. hand-built integer cases ----------------------------------------------------------------------------------------------
TRI = np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [0.1, 0.6, 0.1]], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["quadric", "average"])
def test_hand_built_cases(hip_lib, mode):
    o = [0.0, 0.0, 0.0]
    # an empty mesh; vertices without triangles
    d = _hip(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), None, 0.25, mode)
    assert d["V"].shape == (0, 3) and d["F"].shape == (0, 3) and d["n_cells"] == 0
    d, _ = _same(TRI, np.zeros((0, 3), np.int64), TRI, 0.25, mode, o)
    assert d["V"].shape == (0, 3) and d["vertex_cluster"].tolist() == [-1, -1, -1] and d["n_cells"] == 3
    # one triangle at a small h: unchanged (a lone vertex is its own mean; the quadric of one plane leaves it there too)
    d, _ = _same(TRI, [[0, 1, 2]], TRI, 0.25, mode, o)
    assert d["F"].tolist() == [[0, 1, 2]] and d["vertex_cluster"].tolist() == [0, 1, 2] and np.array_equal(d["C"], TRI)
    assert np.all(np.abs(d["V"] - TRI) <= np.spacing(np.float32(0.6)))
    # ... and at a large h: nothing left
    d, _ = _same(TRI, [[0, 1, 2]], TRI, 1.0, mode, o)
    assert d["F"].shape == (0, 3) and d["V"].shape == (0, 3) and d["n_degenerate"] == 1 and d["vertex_cluster"].tolist() == [-1] * 3
    # vertices exactly on cell faces (h = 0.25, origin 0): a vertex on a face belongs to the upper cell
    onface = np.array([[0.25, 0.1, 0.1], [0.2499999, 0.1, 0.1], [0.5, 0.25, 0.0], [0.3, 0.1, 0.1], [0.1, 0.2, 0.2], [0.6, 0.3, 0.1]], np.float32)
    d, _ = _same(onface, [[0, 1, 2], [3, 4, 5], [1, 2, 0]], None, 0.25, mode, o)
    assert d["vertex_cluster"].tolist() == [0, 1, 2, 0, 1, 2] and d["F"].tolist() == [[0, 1, 2]] and d["n_duplicate"] == 2
    # two vertex-disjoint triangles on one oriented triple (the lower index stays), a rotated duplicate (dropped), a reversed
    # one (kept), a vertex in no triangle (-1), a triangle inside one cluster, a zero-area triangle
    P = np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [0.1, 0.6, 0.1], [0.12, 0.1, 0.1], [0.62, 0.1, 0.1], [0.12, 0.6, 0.1], [0.9, 0.9, 0.9]],
                 np.float32)
    F = [[3, 4, 5], [0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 3, 2], [0, 0, 1]]
    d, _ = _same(P, F, _colors(P), 0.25, mode, o)
    assert d["F"].tolist() == [[0, 1, 2], [0, 2, 1]] and d["vertex_cluster"].tolist() == [0, 1, 2, 0, 1, 2, -1]
    assert (d["n_cells"], d["n_degenerate"], d["n_duplicate"], d["n_zero_area"]) == (4, 2, 2, 1)
    d, _ = _same(P, F, _colors(P), 0.25, mode, o, remove_unreferenced=False)
    assert d["vertex_cluster"].tolist() == [0, 1, 2, 0, 1, 2, 3] and d["V"].shape == (4, 3)
    # a zero-area triangle adds nothing to A: with it or without it, the same positions
    a = _hip(P, F, None, 0.25, mode, o)
    b = _hip(P, F[:-1], None, 0.25, mode, o)
    assert a["V"].tobytes() == b["V"].tobytes() and (a["n_zero_area"], b["n_zero_area"]) == (1, 0)


# ---- 2., 5., 6. icosphere(3) ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["quadric", "average"])
@pytest.mark.parametrize("h,cells,verts,tris", [(0.1, 338, 338, 672), (0.2, 104, 104, 204), (0.4, 28, 25, 46)])
def test_icosphere3(hip_lib, mode, h, cells, verts, tris):
    V, F = _sphere(3)
    assert V.shape == (642, 3) and F.shape == (1280, 3)
    d, ref = _same(V, F, _colors(V), h, mode, name=f"icosphere(3) h={h}")
    assert (d["n_cells"], len(d["V"]), len(d["F"])) == (cells, verts, tris)
    assert R.outside_count(ref, 1e-9 * h) == R.outside_count(ref, -1e-9 * h) == d["n_clamped"]


# ---- 3. one crowded cell -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["quadric", "average"])
def test_one_crowded_cell(hip_lib, mode):
    h = 0.25
    V, F = crowded(h)
    d, ref = _same(V, F, _colors(V), h, mode, origin=[0.0, 0.0, 0.0], name="crowded cell")
    members = np.bincount(ref["vertex_cluster"][ref["vertex_cluster"] >= 0])
    assert members.max() == 4098 and 3 * 4097 * 2 > 8192 and len(d["F"]) > 0 and d["n_degenerate"] > 4097
    assert R.outside_count(ref, 1e-9 * h) == R.outside_count(ref, -1e-9 * h) == d["n_clamped"]
    assert d["n_clamped"] == (4 if mode == "quadric" else 0)


@pytest.mark.gpu
def test_roof_clamps(hip_lib):
    """Clusters whose quadric minimiser leaves the cell: clamped to the box, counted."""
    h = 0.137
    V, F = roof()
    d, ref = _same(V, F, None, h, "quadric", name="roof")
    assert R.outside_count(ref, 1e-9 * h) == R.outside_count(ref, -1e-9 * h) == d["n_clamped"] == 8
    _same(V, F, None, h, "average")


# ---- 4. icosphere(5): reproducibility ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["quadric", "average"])
def test_icosphere5_matches_and_is_bitwise_reproducible(hip_lib, mode):
    V, F = _sphere(5)
    assert V.shape == (10242, 3) and F.shape == (20480, 3) and len(V) % 256 != 0      # (several blocks; a ragged last one)
    h, C = 0.05, _colors(V)
    a, ref = _same(V, F, C, h, mode, name="icosphere(5) h=0.05")
    b = _hip(V, F, C, h, mode)
    c = _hip(V, F, C, h, mode, origin=[float(x) for x in R.default_origin(V, h)])
    for other in (b, c):
        for k in ("V", "F", "C", "vertex_cluster"):
            assert a[k].tobytes() == other[k].tobytes(), k
        assert all(a[k] == other[k] for k in COUNTERS)
    assert R.outside_count(ref, 1e-9 * h) == R.outside_count(ref, -1e-9 * h) == a["n_clamped"]


# ---- 7. the cube ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cube_corners_on_the_device(hip_lib):
    """The closed form of tests/test_meshsimplify.py on the device: the quadric vertex within 0.0026 h of the corner, the mean
    farther than 0.1 h."""
    h = 0.25
    V, F = R.cube(32)
    o = [-0.5 - h / 2] * 3
    corners = np.array([[sx, sy, sz] for sx in (-0.5, 0.5) for sy in (-0.5, 0.5) for sz in (-0.5, 0.5)])
    cid = [int(np.nonzero(np.all(V == c.astype(np.float32), axis=1))[0][0]) for c in corners]
    q, _ = _same(V, F, None, h, "quadric", o, name="cube")
    a, _ = _same(V, F, None, h, "average", o)
    dq = np.linalg.norm(q["V"][q["vertex_cluster"][cid]].astype(np.float64) - corners, axis=1)
    da = np.linalg.norm(a["V"][a["vertex_cluster"][cid]].astype(np.float64) - corners, axis=1)
    assert dq.max() <= 0.0026 * h, dq.max() / h
    assert da.min() > 0.1 * h, da.min() / h


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_stream_usable(hip_lib):
    V, F = _sphere(3)
    good = _hip(V, F, None, 0.2)
    nan = V.copy()
    nan[17, 1] = np.nan
    inf = V.copy()
    inf[5, 0] = np.inf
    bad_f = F.copy()
    bad_f[100, 2] = len(V)
    neg_f = F.copy()
    neg_f[7, 0] = -1
    above = [float(x) for x in V.min(0) + np.float32(0.01)]
    for args, match in (((nan, F, None, 0.2), "not finite"), ((inf, F, None, 0.2), "not finite"),
                        ((V, bad_f, None, 0.2), r"outside \[0, Nv\)"), ((V, neg_f, None, 0.2), r"outside \[0, Nv\)"),
                        ((V, F, None, 2.0 ** -22), "voxel_size too small"), ((V, F, None, 0.2, "quadric", above), "negative cell")):
        with pytest.raises(RuntimeError, match=match):
            _hip(*args)
        again = _hip(V, F, None, 0.2)                      # the next valid call on the same stream
        assert again["V"].tobytes() == good["V"].tobytes() and np.array_equal(again["F"], good["F"])


# ---- 9. simplify_to ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("target", [1000, 200, 6000])
def test_simplify_to(hip_lib, target):
    from lara_amd.meshsimplify import simplify_to, simplify_vertex_clustering
    V, F = _sphere(4)
    assert F.shape == (5120, 3)
    v, f = torch.as_tensor(V).cuda(), torch.as_tensor(F).cuda()
    c = torch.as_tensor(_colors(V)).cuda()
    v2, f2, c2, info = simplify_to(v, f, c, target)
    if target >= 5120:
        assert torch.equal(v2, v) and torch.equal(f2, f) and torch.equal(c2, c) and info["probes"] == []
        assert v2.data_ptr() != v.data_ptr()
        return
    probes = info["probes"]
    assert f2.shape[0] <= target and 1 < len(probes) <= 12 and all(n == R.count_triangles(V, F, h) for h, n in probes)
    fits = [h for h, n in probes if n <= target]
    assert info["voxel_size"] == min(fits)
    finer = [(h, n) for h, n in probes if h < min(fits)]
    assert all(n > target for h, n in finer)
    if finer:
        assert max(finer)[1] > target          # the next finer probe
    w = simplify_vertex_clustering(v, f, c, min(fits))
    assert torch.equal(w[0], v2) and torch.equal(w[1], f2) and torch.equal(w[2], c2)
    assert f2.shape[0] == dict(probes)[min(fits)]


# ---- 10. MeshExtractor ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mesh_extractor_simplifies_between_clean_mesh_and_write_obj(hip_lib, tmp_path):
    from lara_amd.mesh import MeshExtractor, clean_mesh, read_obj, write_obj
    from lara_amd.meshsimplify import simplify_vertex_clustering
    from lara_amd.renderer import Renderer
    from tests.test_meshclean_gpu import _scene_params, _turntable
    params, cams = _scene_params(), _turntable()
    render = Renderer(sh_degree=1, white_background=True)
    ex = MeshExtractor(params, render, None)
    plain = str(tmp_path / "plain.obj")
    v, t, c = ex.extract(plain, None, cams=cams)
    assert ex.last_simplify_info is None
    cv, ct, cc, _ = clean_mesh(*ex.raw_mesh, aabb=None, keep=10)
    assert torch.equal(v, cv) and torch.equal(t, ct) and torch.equal(c, cc)
    write_obj(str(tmp_path / "by_hand.obj"), cv, ct, cc)
    assert (tmp_path / "plain.obj").read_bytes() == (tmp_path / "by_hand.obj").read_bytes()
    voxel = ex.last_grid[1]
    ex.timings = []
    small = str(tmp_path / "small.obj")
    sv, st, sc = ex.extract(small, None, cams=cams, simplify_voxel=4 * voxel)
    torch.cuda.synchronize()
    assert "simplify" in [name for name, _ in ex.timings]
    wv, wt, wc, winfo = simplify_vertex_clustering(cv, ct, cc, 4 * voxel)
    assert torch.equal(sv, wv) and torch.equal(st, wt) and torch.equal(sc, wc)
    assert torch.equal(ex.last_simplify_info["vertex_cluster"], winfo["vertex_cluster"])
    rv, rt, rc = read_obj(small)
    assert rv.tobytes() == wv.cpu().numpy().tobytes() and np.array_equal(rt, wt.cpu().numpy()) and rc.tobytes() == wc.cpu().numpy().tobytes()
    assert 0 < st.shape[0] < t.shape[0] / 4
    tv, tt, tc = ex.extract(str(tmp_path / "budget.obj"), None, cams=cams, simplify_target=2000)
    assert 0 < tt.shape[0] <= 2000 and len(ex.last_simplify_info["probes"]) > 1
    with pytest.raises(ValueError):
        ex.extract(small, None, cams=cams, simplify_voxel=voxel, simplify_target=10)
