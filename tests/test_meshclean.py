"""The restatement of the reference's mesh post-processing (tests/meshclean_restate.py; Open3D's semantics [RECALLED],
Open3D absent) on known answers, against scipy's connected components, and the OBJ writer of lara_amd.mesh."""
import numpy as np
import pytest

from tests import meshclean_restate as R


def _v(n):
    return np.random.default_rng(0).random((n, 3)).astype(np.float32)


def test_a_shared_edge_joins_a_shared_vertex_does_not_and_a_fan_is_one_cluster():
    v = _v(8)
    lab, cnt, _ = R.cluster_bfs(v, [[0, 1, 2], [2, 1, 3]])                 # edge (1, 2)
    assert lab.tolist() == [0, 0] and cnt.tolist() == [2]
    lab, cnt, _ = R.cluster_bfs(v, [[0, 1, 2], [2, 3, 4]])                 # vertex 2 only
    assert lab.tolist() == [0, 1] and cnt.tolist() == [1, 1]
    lab, cnt, _ = R.cluster_bfs(v, [[0, 1, 2], [1, 0, 3], [4, 5, 6], [0, 1, 7]])   # three triangles on edge (0, 1)
    assert lab.tolist() == [0, 0, 1, 0] and cnt.tolist() == [3, 1]


def test_clusters_are_numbered_by_their_smallest_triangle():
    v = _v(12)
    tris = [[6, 7, 8], [0, 1, 2], [7, 8, 9], [3, 4, 5], [1, 2, 10]]
    lab, cnt, area = R.cluster_bfs(v, tris)
    assert lab.tolist() == [0, 1, 0, 2, 1] and cnt.tolist() == [2, 2, 1]
    a = R.triangle_areas(v, tris)
    np.testing.assert_allclose(area, [a[0] + a[2], a[1] + a[4], a[3]], rtol=1e-15)
    v64 = v.astype(np.float64)
    assert a[0] == 0.5 * np.linalg.norm(np.cross(v64[7] - v64[6], v64[8] - v64[6]))


def _strip_clusters(sizes):
    """One triangle strip (edge-connected) per size, in order, with disjoint vertices."""
    tris, base = [], 0
    for n in sizes:
        tris += [[base + i, base + i + 1, base + i + 2] for i in range(n)]
        base += n + 2
    return np.array(tris), base


def test_keep_rule_keeps_ties_at_the_threshold():
    sizes = [12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 3, 2]            # 12 clusters, the 10th and 11th largest tie at 3
    tris, nv = _strip_clusters(sizes)
    v = _v(nv)
    lab, cnt, _ = R.cluster_bfs(v, tris)
    assert cnt.tolist() == sizes
    keep = R.keep_mask(lab, cnt, 10)
    assert len(np.unique(lab[keep])) == 11 and keep.sum() == sum(sizes) - 2
    tris, nv = _strip_clusters([5, 1, 3, 2])
    lab, cnt, _ = R.cluster_bfs(_v(nv), tris)
    assert R.keep_mask(lab, cnt, 10).all()


def test_crop_keeps_a_vertex_exactly_on_the_scaled_bound():
    aabb = [-5.0, -5.0, -5.0, 5.0, 5.0, 5.0]          # x 1.1 = +-5.5 exactly, in double and in fp32
    assert 5.0 * 1.1 == 5.5
    out = np.nextafter(np.float32(5.5), np.float32(6))
    v = np.array([[0, 0, 0], [5.5, 0, 0], [0, -5.5, 0], [0, 0, out], [-5.5, 5.5, 5.5]], np.float32)
    tris = [[0, 1, 2], [0, 1, 3], [1, 2, 4]]
    t, keep = R.crop(v, tris, np.array(aabb).reshape(2, 3) * 1.1)
    assert keep.tolist() == [True, False, True]
    ov, ot, _, info = R.clean_mesh(v, tris, aabb=aabb)
    assert info["cluster_n_triangles"].tolist() == [2] and ot.tolist() == [[0, 1, 2], [1, 2, 3]]
    np.testing.assert_array_equal(ov, v[[0, 1, 2, 4]])


def test_clean_mesh_preserves_vertex_order_and_remaps():
    v = _v(10)
    col = np.arange(30, dtype=np.float32).reshape(10, 3)
    tris = [[7, 8, 9], [1, 3, 5], [3, 5, 6]]
    ov, ot, oc, info = R.clean_mesh(v, tris, col, keep=1)
    np.testing.assert_array_equal(ov, v[[1, 3, 5, 6]])
    np.testing.assert_array_equal(oc, col[[1, 3, 5, 6]])
    assert ot.tolist() == [[0, 1, 2], [1, 2, 3]]
    assert info["cluster_n_triangles"].tolist() == [1, 2]


def random_mesh(T, seed, nv=None):
    """Triangles in random order mixing edge-connected patches, vertex-only contacts and non-manifold fans."""
    rng = np.random.default_rng(seed)
    nv = nv or max(8, T // 2)
    tris = []
    while len(tris) < T:
        kind = rng.integers(3)
        a, b = rng.integers(nv, size=2)
        if a == b:
            continue
        if kind == 0:        # a fan of 3..6 triangles on edge (a, b)
            for c in rng.integers(nv, size=rng.integers(3, 7)):
                tris.append([a, b, c])
        elif kind == 1:      # a strip
            c = rng.integers(nv)
            for _ in range(rng.integers(1, 8)):
                d = rng.integers(nv)
                tris.append([a, b, c]); a, b, c = b, c, d
        else:                # a lone triangle touching others at most through vertices
            tris.append([a, rng.integers(nv), rng.integers(nv)])
    tris = np.array(tris[:T], np.int64)
    tris = tris[(tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])]
    return rng.random((nv, 3)).astype(np.float32), tris[rng.permutation(len(tris))]


@pytest.mark.parametrize("T,seed", [(50, 0), (400, 1), (3000, 2)])
def test_bfs_agrees_with_scipy_on_random_meshes(T, seed):
    v, t = random_mesh(T, seed, nv=T)          # sparse: many clusters
    a = R.cluster_bfs(v, t)
    b = R.cluster_scipy(v, t)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_allclose(a[2], b[2], rtol=1e-12)
    assert len(a[1]) > 3


def test_empty_mesh_and_fully_cropped_mesh():
    ov, ot, oc, info = R.clean_mesh(_v(4), np.zeros((0, 3), np.int64))
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and len(info["cluster_n_triangles"]) == 0
    ov, ot, oc, info = R.clean_mesh(_v(4) + 5, [[0, 1, 2]], aabb=[-0.5] * 3 + [0.5] * 3)
    assert ov.shape == (0, 3) and ot.shape == (0, 3)


def test_write_obj_round_trips_exactly(tmp_path):
    torch = pytest.importorskip("torch")
    from lara_amd.mesh import read_obj, write_obj
    rng = np.random.default_rng(5)
    v = (rng.standard_normal((257, 3)) * 10.0 ** rng.integers(-8, 8, size=(257, 1))).astype(np.float32)
    v[0] = [np.float32(0.1), np.float32(1) / 3, -0.0]
    c = rng.random((257, 3)).astype(np.float32)
    t = rng.integers(257, size=(300, 3))
    p = tmp_path / "sub" / "m.obj"
    write_obj(str(p), torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(c))
    rv, rt, rc = read_obj(str(p))
    assert rv.tobytes() == v.tobytes()          # (-0.0 included)
    np.testing.assert_array_equal(rv, v)
    np.testing.assert_array_equal(rc, c)
    np.testing.assert_array_equal(rt, t)
    lines = p.read_text().splitlines()
    assert len(lines) == 557 and lines[257].startswith("f ") and lines[257].split()[1:] == [str(x + 1) for x in t[0]]
    write_obj(str(p), torch.from_numpy(v[:3]), torch.zeros(0, 3, dtype=torch.int64))
    rv, rt, rc = read_obj(str(p))
    assert rv.tobytes() == v[:3].tobytes() and rc is None and rt.shape == (0, 3)
