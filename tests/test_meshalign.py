"""`lara_amd.meshalign` without a GPU: the header's row length held to the module's, the library's refusals, the two host solves held to
known motions through the float64 restatement of the reduction row (tests/meshalign_restate.py), and the restated ICP loop on the
level-2 warped icosphere of the issue.  tests/test_meshalign_gpu.py holds the kernels and the device loop to the same restatement.

Bars.  Exact pairs (float64 inputs): 1e-12 relative, the issue's figure -- a few hundred float64 roundings of sums of O(N) terms.
The restated loop rounds to fp32 what the device stores as fp32 (source, transformed points, closest points, normals), so it can
reach the truth only to those roundings: each point is off by at most about 2 u S (u = 2^-24, S = 1.3 the largest coordinate), and
the least-squares motion over hundreds of points is held to 16 u S = 1.2e-6 (a factor 8 for the conditioning of the 6x6 system);
the restated loop lands at 8e-9 .. 1.1e-8 (level 2), three to thirty times below u itself."""
import numpy as np
import pytest
import torch

from lara_amd import _native, evaluate
from tests import meshalign_cases as C
from tests import meshalign_restate as R

TRUTH_BAR = 16 * R.U * 1.3


def test_header_constants_equal_the_modules():
    """The row length of include/lara_meshalign.h in the header, the module and the restatement; the scale goes in as a double,
    the gate as a float."""
    from lara_amd import meshalign
    from tests import test_abi_cpu as abi
    declared = abi.header_functions()
    assert declared["lara_meshalign_transform"][1][4] == "d" and declared["lara_meshalign_accumulate"][1][9] == "f"
    assert meshalign.ROW == R.ROW == 48
    assert "#define LARA_MESHALIGN_ROW 48\n" in abi.header_texts()["lara_meshalign.h"]


def test_refusals(hip_lib):
    """Null pointers, N < 0, N >= 2^30 and `index == NULL` with M != N come back as LARA2DGS_E_INVALID (-1) from host code, before
    any pointer is used (the non-null ones here are the address 1); a transform of no points is a no-op; python refuses CPU tensors
    and what the solves cannot do."""
    from lara_amd import meshalign
    A = (_native.ctypes.c_double * 12)(*np.eye(4)[:3].ravel())
    O = (_native.ctypes.c_double * 3)()
    tr, acc, wsb = hip_lib.lara_meshalign_transform, hip_lib.lara_meshalign_accumulate, hip_lib.lara_meshalign_accumulate_workspace_bytes
    assert tr(0, None, None, A, 1.0, None, None, None) == 0
    for N in (-1, 1 << 30):
        assert tr(N, 1, None, A, 1.0, 1, None, None) == -1
        assert wsb(N) == -1
        assert acc(N, N, 0, 1, 1, None, None, None, 1, 1.0, O, 1, 1, None) == -1
    assert tr(5, 1, None, None, 1.0, 1, None, None) == -1                     # no matrix
    assert tr(5, None, None, A, 1.0, 1, None, None) == -1                     # no points
    assert tr(5, 1, None, A, 1.0, None, None, None) == -1                     # no output
    assert tr(5, 1, 1, A, 1.0, 1, None, None) == -1                           # normals without an output for them
    assert wsb(0) > 0 and wsb(257) >= 2 * (46 * 8 + 2 * 4) and wsb((1 << 30) - 1) > 0
    assert acc(5, 4, 0, 1, 1, None, None, None, 1, 1.0, O, 1, 1, None) == -1    # no index and M != N
    assert acc(5, 5, 3, 1, 1, None, 1, None, 1, 1.0, O, 1, 1, None) == -1       # normals without their index
    assert acc(5, 5, 3, 1, 1, None, None, 1, 1, 1.0, O, 1, 1, None) == -1       # ... and the other way round
    assert acc(5, 5, 0, 1, 1, None, None, None, 1, 1.0, None, 1, 1, None) == -1   # no origin
    assert acc(5, 5, 0, 1, 1, None, None, None, 1, 1.0, O, None, 1, None) == -1   # no row
    assert acc(5, 5, 0, None, 1, None, None, None, 1, 1.0, O, 1, 1, None) == -1   # no source
    assert acc(5, 5, 0, 1, None, None, None, None, 1, 1.0, O, 1, 1, None) == -1   # no target
    assert acc(5, 5, 0, 1, 1, None, None, None, None, 1.0, O, 1, 1, None) == -1   # no distances
    assert acc(5, 5, 0, 1, 1, None, None, None, 1, 1.0, O, 1, None, None) == -1   # no workspace
    assert acc(5, -1, 0, 1, 1, 1, None, None, 1, 1.0, O, 1, 1, None) == -1 and acc(5, 5, 1 << 30, 1, 1, 1, None, None, 1, 1.0, O, 1, 1, None) == -1
    P = torch.zeros(4, 3)
    for fn in (lambda: meshalign.transform_points(P, np.eye(4)), lambda: meshalign.moments(P),
               lambda: meshalign.accumulate(P, P, None, torch.zeros(4), 1.0),
               lambda: meshalign.icp(P, P, max_dist=1.0, estimation="point", device="cpu"),
               lambda: meshalign.aligned_scores((P, torch.zeros(1, 3, dtype=torch.int64)), P, max_dist=1.0, device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
    with pytest.raises(ValueError, match="with_scale needs"):
        meshalign.icp(P, P, max_dist=1.0, with_scale=True, device="cpu")
    with pytest.raises(ValueError, match="'plane' or 'point'"):
        meshalign.icp(P, P, max_dist=1.0, estimation="surface", device="cpu")
    with pytest.raises(ValueError, match="init must be"):
        meshalign.icp(P, P, max_dist=1.0, init="fpfh", device="cpu")
    with pytest.raises(ValueError, match="positive determinant"):
        meshalign._similarity(np.diag([1.0, 1.0, -1.0, 1.0]))
    with pytest.raises(ValueError, match="moves a mesh"):
        meshalign.align_mesh(P, P, max_dist=1.0)


# ---- the host solves through the restated row -----------------------------------------------------------------------------------

def _exact_row(P, Q, normals=None, origin=(0.0, 0.0, 0.0)):
    n = len(P)
    return R.row(P, Q, None, normals, None if normals is None else np.arange(n), np.zeros(n), 1.0, origin, dtype=np.float64)[0]


@pytest.mark.parametrize("scale, angle, axis", [(0.5, 20.0, (1, 2, 3)), (1.0, 170.0, (0, 0, 1)), (2.0, 95.0, (-3, 1, 0.5)), (1.08, 15.0, (1, 2, 3))])
def test_solve_point_recovers_a_known_similarity(scale, angle, axis):
    """Exact pairs 100 units from the origin, the row taken about ORIGIN: scale, rotation and translation to 1e-12 relative.
    Without `with_scale` the same pairs at scale 1 give the rigid motion."""
    from lara_amd import meshalign
    g = np.random.default_rng(5)
    o = np.array(C.ORIGIN)
    P = o + g.normal(size=(200, 3))
    for s, ws in ((scale, True), (1.0, False)):
        T = R.rigid(angle, axis, t=(3.0, -2.0, 1.0), scale=s)
        Q = P @ T[:3, :3].T + T[:3, 3]
        got = meshalign.solve_point(_exact_row(P, Q, origin=o), ws, origin=o)
        assert np.abs(got[:3, :3] - T[:3, :3]).max() <= 1e-12 * s, (s, np.abs(got[:3, :3] - T[:3, :3]).max())
        assert np.abs(got[:3, 3] - T[:3, 3]).max() <= 1e-12 * np.abs(Q).max()      # (t = mean q - sR mean p: a difference at |q|)
        assert abs(np.linalg.det(got[:3, :3]) ** (1 / 3) - s) <= 1e-12 * s and np.array_equal(got[3], [0, 0, 0, 1])


def test_solve_point_keeps_the_rotation_proper_on_a_planar_set():
    """All points in one plane: the smallest singular value is 0 and its vectors' signs are the SVD's choice; the determinant fix
    must give the rotation, never the reflection through the plane."""
    from lara_amd import meshalign
    g = np.random.default_rng(6)
    P = np.concatenate([g.normal(size=(50, 2)), np.zeros((50, 1))], 1)
    for angle, axis in ((40.0, (1, 2, 3)), (180.0, (1, 0, 0)), (120.0, (1, 1, 1)), (90.0, (0, 1, 0))):
        T = R.rigid(angle, axis, t=(0.5, 0.25, -1.0))
        got = meshalign.solve_point(_exact_row(P, P @ T[:3, :3].T + T[:3, 3]))
        assert np.linalg.det(got[:3, :3]) > 0.999 and np.abs(got - T).max() <= 1e-12, (angle, np.abs(got - T).max())
    with pytest.raises(ValueError, match="at least 3 pairs"):
        meshalign.solve_point(_exact_row(P[:2], P[:2]))
    line = np.outer(np.arange(10.0), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="singular"):
        meshalign.solve_point(_exact_row(line, line))
    with pytest.raises(ValueError, match="singular"):
        meshalign.solve_point(_exact_row(np.ones((5, 3)), np.ones((5, 3))))


def test_solve_plane_recovers_a_small_motion():
    """A motion of 1e-3 rad and 1e-3 units between exact pairs with the normals at the targets: one step is right to second order
    (the step drops the terms of order theta^2 |p| / 2 and theta |t|, bounded here by 4 theta^2 with |p| <= 1.3), and three steps,
    each re-linearised about the accumulated motion, reach 1e-12."""
    from lara_amd import meshalign
    V, F = R.warped_icosphere(1)
    P = V.astype(np.float64)
    Nn = np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]])
    Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    S = P[F].mean(1)                                       # the face centroids, their faces' normals
    theta = 1e-3
    T = R.rigid(np.rad2deg(theta), (2, -1, 2), t=(6e-4, -5e-4, 6e-4))
    Q, Nq = S @ T[:3, :3].T + T[:3, 3], Nn @ T[:3, :3].T
    acc = np.eye(4)
    errs = []
    for _ in range(3):
        X = S @ acc[:3, :3].T + acc[:3, 3]
        acc = meshalign.solve_plane(_exact_row(X, Q, Nq)) @ acc
        errs.append(float(np.abs(acc - T).max()))
        assert abs(np.linalg.det(acc[:3, :3]) - 1.0) <= 1e-14
    print(f"meshalign solve_plane: |T - truth| after 1, 2, 3 steps {errs}")
    assert errs[0] <= 4 * theta ** 2 and errs[2] <= 1e-12
    with pytest.raises(ValueError, match="at least 6 pairs"):
        meshalign.solve_plane(_exact_row(S[:5], Q[:5], Nq[:5]))
    with pytest.raises(ValueError, match="at least 6 pairs"):
        meshalign.solve_plane(_exact_row(S, Q))                                              # no normals at all
    flat = np.concatenate([np.random.default_rng(7).normal(size=(30, 2)), np.zeros((30, 1))], 1)
    with pytest.raises(ValueError, match="singular"):
        meshalign.solve_plane(_exact_row(flat, flat, np.tile([0.0, 0.0, 1.0], (30, 1))))     # a plane pins three motions only


def test_the_origin_keeps_the_digits():
    """Pairs 10^4 units away, exact to the spacing of float64 there (3.6e-12): about their offset the row gives the rotation to
    1e-11, about 0 the centred sums cancel eight digits and the result is visibly worse -- what the parameter is for."""
    from lara_amd import meshalign
    g = np.random.default_rng(8)
    o = np.array([1e4, -2e4, 3e4])
    P = o + g.normal(size=(300, 3))
    T = R.rigid(33.0, t=(1.0, 2.0, 3.0))
    Q = P @ T[:3, :3].T + T[:3, 3]
    good = np.abs(meshalign.solve_point(_exact_row(P, Q, origin=o), origin=o)[:3, :3] - T[:3, :3]).max()
    bad = np.abs(meshalign.solve_point(_exact_row(P, Q))[:3, :3] - T[:3, :3]).max()
    print(f"meshalign origin: rotation error {good:.2e} about the points' offset, {bad:.2e} about 0")
    assert good <= 1e-11 and bad > 100 * good


# ---- the restated loop ----------------------------------------------------------------------------------------------------------

_loops = {}


def _loop(angle, estimation):
    if (angle, estimation) not in _loops:
        S, V, F, T = C.registration_case(2, angle)
        _loops[angle, estimation] = (R.icp(S, V, F, max_dist=C.MAX_DIST, estimation=estimation, max_iter=50 if estimation == "plane" else 10), T)
    return _loops[angle, estimation]


@pytest.mark.parametrize("angle", sorted(C.STARTS))
def test_restated_icp_in_plane_mode_reaches_the_truth(angle):
    out, T = _loop(angle, "plane")
    err = float(np.abs(out["transformation"][:3] - T[:3]).max())
    print(f"meshalign restated plane mode from {angle} degrees: {out['iterations']} iterations, |T - truth| {err:.2e}, "
          f"inlier rmse {out['inlier_rmse']:.2e}, rotation error {R.rotation_error(out['transformation'], T):.2e}")
    assert out["converged"] and out["iterations"] == C.RESTATED_ITERATIONS[angle]
    assert out["fitness"] == 1.0 and err <= TRUTH_BAR and out["inlier_rmse"] <= TRUTH_BAR


@pytest.mark.parametrize("angle", sorted(C.STARTS))
def test_restated_icp_in_point_mode_never_raises_its_rmse(angle):
    """Point mode slides along the surface: after 10 iterations it is nowhere near the truth (which is why nothing here asks for
    that), but every iteration lowers the inlier RMSE: the solve is the least-squares optimum for the pairs it was given, and the
    next search can only shorten each pair (all pairs are inliers here: fitness 1 throughout)."""
    out, T = _loop(angle, "point")
    rmse = [h["inlier_rmse"] for h in out["history"]]
    print(f"meshalign restated point mode from {angle} degrees: rmse {rmse[0]:.4f} -> {rmse[-1]:.4f} in {out['iterations']} iterations, "
          f"rotation error {R.rotation_error(out['transformation'], T):.3f}")
    assert all(h["fitness"] == 1.0 for h in out["history"])
    assert all(b <= a for a, b in zip(rmse, rmse[1:])) and rmse[-1] < 0.5 * rmse[0]


def test_pca_candidates_are_the_four_proper_rotations():
    """Each candidate maps the source's centroid and principal frame onto the target's; for a rigidly moved copy one of them is the
    motion itself."""
    from lara_amd import meshalign
    V, F = R.warped_icosphere(2)
    T = R.rigid(C.PCA_START[0], t=C.PCA_START[1])
    P = np.concatenate([V.astype(np.float64), V.astype(np.float64)[F].mean(1)])
    Sm = P @ np.linalg.inv(T)[:3, :3].T + np.linalg.inv(T)[:3, 3]
    cands = meshalign.pca_candidates(Sm.mean(0), np.cov(Sm.T, bias=True), P.mean(0), np.cov(P.T, bias=True))
    assert len(cands) == 4 and all(abs(np.linalg.det(c[:3, :3]) - 1.0) <= 1e-12 for c in cands)
    assert all(np.abs(c[:3, :3] @ Sm.mean(0) + c[:3, 3] - P.mean(0)).max() <= 1e-12 for c in cands)
    assert min(np.abs(c - T).max() for c in cands) <= 1e-9
    assert len({tuple(np.round(c[:3, :3].ravel(), 6)) for c in cands}) == 4


# ---- hooks ----------------------------------------------------------------------------------------------------------------------

def test_aligned_scores_dict_reaches_the_evaluator():
    s = {"accuracy": 0.01, "completeness": 0.03, "chamfer": 0.04, "chamfer_sq": 0.0016, "normal_consistency": 0.9,
         "thresholds": [0.01, 0.02], "precision": [0.5, 1.0], "recall": [0.25, 0.5], "fscore": [1.0 / 3.0, 2.0 / 3.0], "n_pred": 10,
         "n_gt": 10, "fallbacks": 0}
    reg = {"transformation": np.eye(4), "scale": 1.0, "fitness": 1.0, "inlier_rmse": 0.0, "iterations": 3, "converged": True,
           "history": [], "fallbacks": 0}
    plain, aligned = evaluate.Evaluator(4), evaluate.Evaluator(4)
    plain.add_geometry("a", s)
    aligned.add_geometry("a", dict(s, distance="triangle", alignment=reg))
    assert plain.summary() == aligned.summary() and "alignment" not in aligned.summary() and aligned.summary()["chamfer_mean"] == 0.04
