"""The numpy restatement of include/lara_meshsimplify.h (tests/meshsimplify_restate.py) held to closed forms, the
header's constants held to the module's, the library's refusals -- no GPU.  tests/test_meshsimplify_gpu.py holds the
kernels to this restatement."""
import numpy as np
import pytest
import torch

from lara_amd import meshsimplify
from tests import meshsimplify_restate as R


def test_header_constants_equal_the_modules():
    """The error bits, the cell limit and the counter slots of include/lara_meshsimplify.h, as the header defines them and as
    the module and the restatement repeat them."""
    from tests import test_abi_cpu as abi
    assert (meshsimplify.ERR_INDEX, meshsimplify.ERR_PROBE, meshsimplify.ERR_NONFINITE, meshsimplify.ERR_NEGATIVE,
            meshsimplify.ERR_EXTENT, meshsimplify.MAX_CELL, meshsimplify.COUNTERS) == (1, 2, 4, 8, 16, 1 << 21, 4)
    text = abi.header_texts()["lara_meshsimplify.h"]
    for macro, value in (("ERR_INDEX", "1"), ("ERR_PROBE", "2"), ("ERR_NONFINITE", "4"), ("ERR_NEGATIVE", "8"), ("ERR_EXTENT", "16"),
                         ("MAX_CELL", "(1 << 21)"), ("N_DEGENERATE", "0"), ("N_DUPLICATE", "1"), ("N_ZERO_AREA", "2"),
                         ("N_CLAMPED", "3"), ("COUNTERS", "4")):
        assert f"#define LARA_MESHSIMPLIFY_{macro} {value}\n" in text
    assert R.MAX_CELL == meshsimplify.MAX_CELL


def test_size_queries_and_entry_points_refuse_bad_sizes(hip_lib):
    """Negative sizes (and sizes of 2^31 rows and more) come back as LARA2DGS_E_INVALID (-1) from host code, before any
    pointer is used; the python layer refuses CPU tensors and bad arguments."""
    L = hip_lib
    assert L.lara_meshsimplify_cells_workspace_bytes(-1) == -1 and L.lara_meshsimplify_cells_workspace_bytes(1 << 31) == -1
    assert L.lara_meshsimplify_cells_workspace_bytes(0) == 64 * 12 and L.lara_meshsimplify_cells_workspace_bytes(1000) == 2048 * 12
    assert L.lara_meshsimplify_triangles_workspace_bytes(-1) == -1 and L.lara_meshsimplify_triangles_workspace_bytes((1 << 31) // 3 + 1) == -1
    assert L.lara_meshsimplify_triangles_workspace_bytes(100) == 256 * 8 + 512
    assert L.lara_meshsimplify_bucket_workspace_bytes(-1, 4) == -1 and L.lara_meshsimplify_bucket_workspace_bytes(4, -1) == -1
    assert L.lara_meshsimplify_bucket_workspace_bytes(100, 10) == 256 + 512
    assert L.lara_meshsimplify_cells(-1, None, 0.1, None, None, None, None, None, None) == -1
    assert L.lara_meshsimplify_cells(4, None, 0.0, None, None, None, None, None, None) == -1            # h must be positive
    assert L.lara_meshsimplify_cells(4, None, float("nan"), None, None, None, None, None, None) == -1
    assert L.lara_meshsimplify_cells(4, None, 0.1, None, None, None, None, None, None) == -1            # null pointers
    assert L.lara_meshsimplify_cells(0, None, 0.1, None, None, None, None, None, None) == 0
    assert L.lara_meshsimplify_triangles(4, -1, 1, None, None, None, None, None, None, None, None, None) == -1
    assert L.lara_meshsimplify_triangles(4, 2, 5, None, None, None, None, None, None, None, None, None) == -1  # n_cells > Nv
    assert L.lara_meshsimplify_triangles(4, 0, 1, None, None, None, None, None, None, None, None, None) == 0
    assert L.lara_meshsimplify_bucket_fill(-1, 1, None, None, None, None, None) == -1
    assert L.lara_meshsimplify_sums(4, 2, 5, None, None, None, None, None, None, None, 1, None, None, None, None) == -1
    assert L.lara_meshsimplify_solve(4, 2, 1, None, None, None, None, -1.0, None, None, None, None, None) == -1
    assert L.lara_meshsimplify_vertex_map(-1, 0, None, None, None, None, None) == -1
    V, F = R.cube(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshsimplify.simplify_vertex_clustering(torch.from_numpy(V), torch.from_numpy(F), None, 0.25)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshsimplify.simplify_to(torch.from_numpy(V), torch.from_numpy(F), None, 4)
    with pytest.raises(ValueError):
        meshsimplify.simplify_vertex_clustering(torch.from_numpy(V), torch.from_numpy(F), None, 0.25, contraction="median")
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            meshsimplify._pitch(bad)


def test_restatement_refuses_what_the_library_refuses():
    V, F = R.cube(2)
    bad = V.copy()
    bad[3, 1] = np.nan
    for fn in (lambda: R.simplify(bad, F, None, 0.25), lambda: R.simplify(V, F, None, 0.25, origin=[0.0, -1.0, -1.0]),
               lambda: R.simplify(V, F, None, 2.0 ** -22), lambda: R.simplify(V, np.array([[0, 1, len(V)]]), None, 0.25)):
        with pytest.raises(ValueError):
            fn()


def test_integer_rules_by_hand():
    """Faces belong to the upper cell; duplicates keep the lower index, a rotation is a duplicate, a reversal is not; an unused
    vertex maps to -1; a zero-area triangle is counted and dropped."""
    h, o = 0.25, [0.0, 0.0, 0.0]
    V = np.array([[0.25, 0.1, 0.1], [0.2499999, 0.1, 0.1], [0.5, 0.25, 0.0]], np.float32)
    assert R.cells(V, h, o)[0].tolist() == [[1, 0, 0], [0, 0, 0], [2, 1, 0]]
    # three clusters A, B, C (two vertices each), one spare vertex in a fourth cell
    P = np.array([[0.1, 0.1, 0.1], [0.6, 0.1, 0.1], [0.1, 0.6, 0.1], [0.12, 0.1, 0.1], [0.62, 0.1, 0.1], [0.12, 0.6, 0.1], [0.9, 0.9, 0.9]],
                 np.float32)
    F = np.array([[3, 4, 5], [0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 3, 2], [0, 0, 1]])
    s = R.simplify(P, F, None, h, "quadric", origin=o)
    assert s["n_cells"] == 4 and s["F"].tolist() == [[0, 1, 2], [0, 2, 1]]
    assert (s["n_degenerate"], s["n_duplicate"], s["n_zero_area"]) == (2, 2, 1)
    assert s["vertex_cluster"].tolist() == [0, 1, 2, 0, 1, 2, -1] and len(s["V"]) == 3
    keep_all = R.simplify(P, F, None, h, "average", origin=o, remove_unreferenced=False)
    assert keep_all["vertex_cluster"].tolist() == [0, 1, 2, 0, 1, 2, 3] and len(keep_all["V"]) == 4
    np.testing.assert_array_equal(keep_all["V"][0], ((P[0].astype(np.float64) + P[3]) / 2).astype(np.float32))


@pytest.mark.parametrize("mode", ["quadric", "average"])
def test_flat_grid_stays_on_its_plane(mode):
    """(a) A flat triangulated grid: every output vertex lies on the plane to within one fp32 spacing (A has rank 1 there and
    b = 0: the regulariser leaves the mean, which is on the plane)."""
    z = 0.3
    V, F = R.flat_grid(40, 0.01, z)
    s = R.simplify(V, F, None, 0.037, mode)
    assert 0 < len(s["F"]) < len(F) and s["n_zero_area"] == 0
    z32 = float(np.float32(z))
    assert np.all(np.abs(s["V"][:, 2].astype(np.float64) - z32) <= R.spacing32(z32))
    assert np.all(np.abs(s["x64"][:, 2] - z32) <= R.spacing32(z32))
    # orientation survives: every output normal points up
    p0, c = R.face_cross(s["V"], s["F"])
    assert np.all(c[:, 2] > 0)


def test_cube_corners_quadric_against_average():
    """(b) The unit cube, 32 x 32 quads per face, h = 0.25, origin = -0.5 - h / 2: a corner sits at the centre of its cell and
    sees three equal face areas, A = w I, so the quadric vertex lies within 3 lambda / (1 + 3 lambda) |m - corner| <= 0.0026 h
    of the corner (lambda = 2^-10, |m - corner| <= the half diagonal); the mean lies farther than 0.1 h."""
    h = 0.25
    V, F = R.cube(32)
    assert V.shape == (6 * 32 * 32 + 2, 3) and F.shape == (12 * 32 * 32, 3)
    corners = np.array([[sx, sy, sz] for sx in (-0.5, 0.5) for sy in (-0.5, 0.5) for sz in (-0.5, 0.5)])
    cid = [int(np.nonzero(np.all(V == c.astype(np.float32), axis=1))[0][0]) for c in corners]
    q = R.simplify(V, F, None, h, "quadric", origin=[-0.5 - h / 2] * 3)
    a = R.simplify(V, F, None, h, "average", origin=[-0.5 - h / 2] * 3)
    assert q["n_cells"] == 5 ** 3 - 3 ** 3 and np.array_equal(q["F"], a["F"])
    dq = np.linalg.norm(q["V"][q["vertex_cluster"][cid]].astype(np.float64) - corners, axis=1)
    da = np.linalg.norm(a["V"][a["vertex_cluster"][cid]].astype(np.float64) - corners, axis=1)
    assert dq.max() <= 0.0026 * h, dq.max() / h
    assert da.min() > 0.1 * h, da.min() / h


def test_count_is_the_full_result_s_count_and_falls_with_h():
    from tests.meshrender_cases import icosphere
    V, F = icosphere(3)
    counts = [R.count_triangles(V, F, h) for h in (0.1, 0.2, 0.4)]
    assert counts == [len(R.simplify(V, F, None, h, "average")["F"]) for h in (0.1, 0.2, 0.4)] == [672, 204, 46]
