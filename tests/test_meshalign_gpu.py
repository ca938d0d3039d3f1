"""csrc/meshalign.hip and the loop of lara_amd/meshalign.py held to the float64 restatement (tests/meshalign_restate.py): the
reduction row against the restated sums, masking, reproducibility, the transform bit for bit, the registration of the level-3 warped
icosphere in plane and point mode, the PCA start, `aligned_scores`, and the bench tool at its --quick size.

Bars (u = 2^-24).
  sums       the kernel and the restatement add the same float64 terms in different orders: |difference| <= (2 N + 16) 2^-53 times
             the sum of the terms' magnitudes, per entry; the two counts are exact.
  transform  the float64 sequence of the header rounded once: equal bits.  Unit normals come back unit to 8 u.
  motion     tests/meshalign_cases.py: max |T - truth| of the restated loop at level 3 (2.98e-8 from 10 degrees, 7.81e-9 from 25),
             which rounds to fp32 what the device stores as fp32; the device gets 4 x that.
  truth      where the device's path has no restated twin (the PCA start samples the target): 16 u S, as tests/test_meshalign.py.
  rmse       against the restated row at the device's final motion: closest points are stored as fp32, so a pair's residual may
             move by sqrt(3) u S (S = 1.3).
The tests print what they measure and write test_out/meshalign_parity.txt, kept as profiles/meshalign_parity.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import meshalign_cases as C
from tests import meshalign_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_MAX = 1.3
TRUTH_BAR = 16 * R.U * S_MAX
_notes = {}


def _note(key, text):
    _notes[key] = text
    out = os.path.join(ROOT, "test_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "meshalign_parity.txt"), "w") as f:
        f.write("what tests/test_meshalign_gpu.py measured (a ratio: of its bar, 1 fails)\n")
        for k in sorted(_notes):
            f.write(f"{k}: {_notes[k]}\n")
    print(f"meshalign parity {key}: {text}")


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), dtype)


def _row(src, tgt, index, normals, nindex, dist, max_dist, origin=(0.0, 0.0, 0.0)):
    from lara_amd import meshalign
    return meshalign.accumulate(_t(src), _t(tgt), _t(index), _t(dist), max_dist, _t(normals), _t(nindex), origin)


def _bits(row):
    return row.cpu().numpy().view(np.int64)


# ---- 1. the row against the restatement -----------------------------------------------------------------------------------------

_worst_sum = [0.0]


@pytest.mark.parametrize("N", C.SIZES)
def test_accumulate_equals_the_restated_sums(hip_lib, N):
    for with_index in (False, True):
        for with_normals in (False, True):
            for origin in ((0.0, 0.0, 0.0), C.ORIGIN):
                args = C.pairs(N, 1000 + N, with_index, with_normals, origin)
                got = _row(*args, origin).cpu().numpy()
                ref, mag = R.row(*args, origin)
                assert got[0] == ref[0] and got[47] == ref[47], (N, with_index, with_normals, origin, got[0], ref[0], got[47], ref[47])
                bar = (2 * N + 16) * 2.0 ** -53 * mag
                diff = np.abs(got - ref)
                assert np.all(diff[bar == 0] == 0), (N, with_index, with_normals, origin)
                ratio = float((diff[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0
                _worst_sum[0] = max(_worst_sum[0], ratio)
                assert ratio <= 1.0, (N, with_index, with_normals, origin, ratio)
                if not with_normals:
                    assert np.all(got[19:] == 0)
    _note("1 sums, worst |device - restated| / ((2N + 16) 2^-53 sum|term|)", f"{_worst_sum[0]:.4f}")


def test_accumulate_of_nothing_is_a_row_of_zeros(hip_lib):
    z = np.zeros((0, 3), np.float32)
    got = _row(z, z, None, None, None, np.zeros(0, np.float32), 1.0).cpu().numpy()
    assert got.shape == (48,) and np.all(got == 0) and not np.signbit(got).any()


# ---- 2. masking -----------------------------------------------------------------------------------------------------------------

def test_excluded_pairs_change_no_bit(hip_lib):
    """(a) appended: 260 pairs that are not kept, behind 300 that are (one more workgroup, one more partial), leave the row's bits
    alone, whatever sits in their coordinates; (b) in place: the same positions excluded in eight different ways give eight equal
    rows, with the count the restatement gives; (c) dist == max_dist is kept, the next float above it is not; (d) a zero normal and
    a NaN normal drop a pair out of entries 19 .. 47 only."""
    src, tgt, index, normals, nindex, dist, _ = C.pairs(300, 77, True, True)
    M = len(tgt)
    index = np.clip(index, 0, M - 1)
    max_dist = float(np.float32(dist.max()))
    base = _bits(_row(src, tgt, index, normals, nindex, dist, max_dist))
    assert base.view(np.float64)[0] == 300 and base.view(np.float64)[47] == 300
    above = np.nextafter(np.float32(max_dist), np.float32(np.inf))
    kinds = [(-1, 0.1), (M, 0.1), (0, np.inf), (0, np.nan), (0, above), (-2 ** 31, 0.1), (2 ** 31 - 1, 0.1), (0, -np.inf)]
    # (a)
    k = 260
    g = np.random.default_rng(78)
    src2 = np.concatenate([src, np.where(g.random((k, 3)) < 0.3, np.nan, 1e30).astype(np.float32)])
    index2 = np.concatenate([index, np.array([kinds[i % len(kinds)][0] for i in range(k)], np.int32)])
    dist2 = np.concatenate([dist, np.array([kinds[i % len(kinds)][1] for i in range(k)], np.float32)])
    nindex2 = np.concatenate([nindex, g.integers(-5, len(normals) + 5, k).astype(np.int32)])
    assert np.array_equal(_bits(_row(src2, tgt, index2, normals, nindex2, dist2, max_dist)), base)
    # (b)
    where = np.arange(3, 300, 7)
    rows = []
    for bad_index, bad_dist in kinds:
        i2, d2 = index.copy(), dist.copy()
        if bad_dist == 0.1:
            i2[where] = bad_index
        else:
            d2[where] = bad_dist
        rows.append(_bits(_row(src, tgt, i2, normals, nindex, d2, max_dist)))
        ref = R.row(src, tgt, i2, normals, nindex, d2, max_dist)[0]
        assert rows[-1].view(np.float64)[0] == ref[0] == 300 - len(where) and rows[-1].view(np.float64)[47] == ref[47]
    assert all(np.array_equal(r, rows[0]) for r in rows) and not np.array_equal(rows[0], base)
    # (c)
    d3 = dist.copy()
    d3[5] = np.float32(max_dist)
    assert _row(src, tgt, index, normals, nindex, d3, max_dist).cpu().numpy()[0] == 300
    d3[5] = above
    assert _row(src, tgt, index, normals, nindex, d3, max_dist).cpu().numpy()[0] == 299
    # (d)
    n2 = np.concatenate([normals, [[0, 0, 0], [np.nan, 1, 0], [0, np.inf, 0]]]).astype(np.float32)
    K = len(normals)
    ni_bad, ni_out = nindex.copy(), nindex.copy()
    ni_bad[where] = K + np.arange(len(where)) % 3
    ni_out[where] = -1
    a = _bits(_row(src, tgt, index, n2, ni_bad, dist, max_dist))
    b = _bits(_row(src, tgt, index, n2, ni_out, dist, max_dist))
    assert np.array_equal(a, b)
    assert np.array_equal(a[:19], base[:19]) and a.view(np.float64)[47] == 300 - len(where)
    assert not np.array_equal(a[19:47], base[19:47]) and np.isfinite(a.view(np.float64)).all()


# ---- 3. reproducible ------------------------------------------------------------------------------------------------------------

def test_two_calls_and_two_streams_give_the_same_bits(hip_lib):
    args = C.pairs(70001, 5, True, True, C.ORIGIN)
    dev_args = [_t(x) if isinstance(x, np.ndarray) else x for x in args]
    from lara_amd import meshalign

    def run():
        src, tgt, index, normals, nindex, dist, max_dist = dev_args
        return meshalign.accumulate(src, tgt, index, dist, max_dist, normals, nindex, C.ORIGIN)
    a, b = _bits(run()), _bits(run())
    torch.cuda.synchronize()
    # torch hands streams out of a pool of 32 in turn, and which of them a LATER test gets decides which hardware queue its work
    # shares (tests/test_stream_safety_gpu.py needs a side stream that does not queue behind the caller's): a whole turn of the pool
    # is taken here, as tests/test_meshdist_gpu.py does, so that every test after this one is handed the stream it would be without it
    side = [torch.cuda.Stream(_dev()) for _ in range(32)][0]
    with torch.cuda.stream(side):          # (its own workspace: `meshmetrics._workspace` is keyed by the stream)
        c = run()
    side.synchronize()
    assert np.array_equal(a, b) and np.array_equal(a, _bits(c))


# ---- 4. transform ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", (0, 1, 257))
def test_transform_equals_the_float64_sequence_bit_for_bit(hip_lib, N):
    from lara_amd import meshalign
    g = np.random.default_rng(40 + N)
    P = (g.normal(size=(N, 3)) * 3).astype(np.float32)
    Nn = g.normal(size=(N, 3))
    Nn = (Nn / np.linalg.norm(Nn, axis=1, keepdims=True)).astype(np.float32)
    T = R.rigid(73.0, (0.3, -1.0, 2.0), t=(0.5, -100.0, 7.0), scale=2.0)
    ref_p, ref_n = R.transform(P, T, Nn)
    got = meshalign.transform_points(_t(P), T).cpu().numpy()
    assert got.shape == (N, 3) and np.array_equal(got.view(np.int32), ref_p.view(np.int32))
    gp, gn = meshalign.transform_points(_t(P), T, _t(Nn))
    assert np.array_equal(gp.cpu().numpy().view(np.int32), ref_p.view(np.int32))
    assert np.array_equal(gn.cpu().numpy().view(np.int32), ref_n.view(np.int32))
    if N:
        off = float(np.abs(np.linalg.norm(gn.cpu().numpy().astype(np.float64), axis=1) - 1.0).max())
        _note(f"4 transform, N = {N}: | |n'| - 1 | / 8 u at scale 2", f"{off / (8 * R.U):.4f}")
        assert off <= 8 * R.U
    dp, dn = _t(P), _t(Nn)                  # in place
    rp, rn = meshalign.transform_points(dp, T, dn, out=(dp, dn))
    assert rp.data_ptr() == dp.data_ptr() and rn.data_ptr() == dn.data_ptr()
    assert np.array_equal(dp.cpu().numpy().view(np.int32), ref_p.view(np.int32))
    assert np.array_equal(dn.cpu().numpy().view(np.int32), ref_n.view(np.int32))


def test_moments_are_the_float64_moments(hip_lib):
    from lara_amd import meshalign
    P = (np.array(C.ORIGIN) + np.random.default_rng(9).normal(size=(1000, 3)) * [1.0, 2.0, 0.5]).astype(np.float32)
    n, mean, cov = meshalign.moments(_t(P), origin=C.ORIGIN)
    P64 = P.astype(np.float64)
    assert n == 1000 and np.abs(mean - P64.mean(0)).max() <= 1e-12 * 100 and np.abs(cov - np.cov(P64.T, bias=True)).max() <= 1e-12 * 4


# ---- 5. plane mode --------------------------------------------------------------------------------------------------------------

_cases = {}


def _case(angle):
    if angle not in _cases:
        S, V, F, T = C.registration_case(3, angle)
        _cases[angle] = (S, V, F, T, _t(S), (_t(V), _t(F)))
    return _cases[angle]


@pytest.mark.parametrize("angle", sorted(C.STARTS))
def test_icp_in_plane_mode_recovers_the_motion(hip_lib, angle):
    from lara_amd import meshalign
    S, V, F, T, dS, dmesh = _case(angle)
    reg = meshalign.icp(dS, dmesh, max_dist=C.MAX_DIST)
    err = float(np.abs(reg["transformation"][:3] - T[:3]).max())
    queries = len(S) * (reg["iterations"] + 1)
    # the restated row at the device's final motion: brute force once
    Q = R.transform(S, reg["transformation"])
    d, face, c = R.closest_on_mesh(Q, V, F)
    r = R.row(Q, c.astype(np.float32), None, None, None, d, C.MAX_DIST)[0]
    rmse_ref = float(np.sqrt(r[1] / r[0]))
    _note(f"5 plane mode from {angle} degrees", f"{reg['iterations']} iterations (restated: {C.RESTATED_ITERATIONS[angle]}), max |T - truth| "
          f"{err:.3e} = {err / C.DEVICE_BAR[angle]:.3f} of the bar {C.DEVICE_BAR[angle]:.3e} (restated loop: {C.RESTATED_ERROR_L3[angle]:.3e}), "
          f"fitness {reg['fitness']}, inlier rmse {reg['inlier_rmse']:.3e} (restated at this motion: {rmse_ref:.3e}), "
          f"fallbacks {reg['fallbacks']} of {queries} queries")
    assert reg["converged"] and abs(reg["iterations"] - C.RESTATED_ITERATIONS[angle]) <= 1
    assert reg["fitness"] == 1.0 == r[0] / len(S) and reg["fallbacks"] <= C.FALLBACK_CAP * queries
    assert len(reg["history"]) == reg["iterations"] + 1 and abs(reg["scale"] - 1.0) <= 1e-12
    assert abs(reg["inlier_rmse"] - rmse_ref) <= np.sqrt(3.0) * R.U * S_MAX
    assert err <= C.DEVICE_BAR[angle]


# ---- 6. point mode --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("angle", sorted(C.STARTS))
def test_icp_in_point_mode_lowers_its_rmse_step_by_step(hip_lib, angle):
    from lara_amd import meshalign
    S, V, F, T, dS, dmesh = _case(angle)
    reg = meshalign.icp(dS, dmesh, max_dist=C.MAX_DIST, estimation="point", max_iter=10)
    rmse = [h["inlier_rmse"] for h in reg["history"]]
    assert reg["iterations"] == 10 and len(rmse) == 11 and all(b <= a for a, b in zip(rmse, rmse[1:])), rmse
    one = meshalign.icp(dS, dmesh, max_dist=C.MAX_DIST, estimation="point", max_iter=1)
    # restated iteration 1: one brute-force search at the start, the restated row, the module's solve
    origin = V.astype(np.float64).mean(0)
    d, face, c = R.closest_on_mesh(S, V, F)
    ref = meshalign.solve_point(R.row(S, c.astype(np.float32), None, None, None, d, C.MAX_DIST, origin)[0], False, origin)
    diff = float(np.abs(one["transformation"][:3] - ref[:3]).max())
    _note(f"6 point mode from {angle} degrees", f"rmse {rmse[0]:.5f} -> {rmse[-1]:.5f} in 10 iterations, never rising; iteration 1 against its "
          f"restatement {diff:.3e} = {diff / C.DEVICE_BAR[angle]:.2e} of the bar")
    assert one["iterations"] == 1 and not one["converged"] and diff <= C.DEVICE_BAR[angle]
    assert one["history"][1]["inlier_rmse"] == rmse[1]


def test_the_scale_is_recovered_from_exact_pairs(hip_lib):
    """Index-paired rows (index NULL, as `moments` calls the kernel): the source against its own image under a similarity of scale
    1.08, which the device rounds to fp32 -- u / 2 relative a coordinate, so the scale is held to 4 u relative.  The loop with
    `with_scale` on the same motion lowers its RMSE step by step."""
    from lara_amd import meshalign
    angle, t, scale = C.SCALE_START
    V, F = R.warped_icosphere(3)
    T = R.rigid(angle, t=t, scale=scale)
    S = R.moved_source(V, F, T)
    dS = _t(S)
    image = meshalign.transform_points(dS, T)
    row = meshalign.accumulate(dS, image, None, torch.zeros(len(S), device=_dev()), 1.0).cpu().numpy()
    got = meshalign.solve_point(row, True)
    s = np.linalg.det(got[:3, :3]) ** (1.0 / 3.0)
    _note("6 scale 1.08 from exact pairs", f"|s - 1.08| / (4 u 1.08) = {abs(s - scale) / (4 * R.U * scale):.4f}, max |T - truth| {np.abs(got - T).max():.3e}")
    assert row[0] == len(S) and abs(s - scale) <= 4 * R.U * scale and np.abs(got - T).max() <= TRUTH_BAR
    reg = meshalign.icp(dS, (_t(V), _t(F)), max_dist=C.MAX_DIST, estimation="point", with_scale=True, max_iter=10)
    rmse = [h["inlier_rmse"] for h in reg["history"]]
    assert all(b <= a for a, b in zip(rmse, rmse[1:])), rmse
    assert 1.0 < reg["scale"] < scale * 1.01 and reg["fitness"] == 1.0


# ---- 7. the PCA start -----------------------------------------------------------------------------------------------------------

def test_the_pca_start_reaches_what_the_identity_start_cannot(hip_lib):
    """The source turned by 150 degrees: from the identity the loop settles in a local minimum (restated: inlier RMSE 0.013), from
    the best of the four PCA candidates it reaches the truth."""
    from lara_amd import meshalign
    angle, t = C.PCA_START
    V, F = R.warped_icosphere(3)
    T = R.rigid(angle, t=t)
    dS, dmesh = _t(R.moved_source(V, F, T)), (_t(V), _t(F))
    plain = meshalign.icp(dS, dmesh, max_dist=C.MAX_DIST)
    pca = meshalign.icp(dS, dmesh, max_dist=C.MAX_DIST, init="pca", n=20000)
    err = float(np.abs(pca["transformation"][:3] - T[:3]).max())
    _note("7 pca start at 150 degrees", f"init=None ends at inlier rmse {plain['inlier_rmse']:.4e} after {plain['iterations']} iterations, "
          f"init='pca' at {pca['inlier_rmse']:.3e} after {pca['iterations']}, max |T - truth| {err:.3e} = {err / TRUTH_BAR:.3f} of 16 u S")
    assert plain["inlier_rmse"] > pca["inlier_rmse"] and pca["converged"] and pca["fitness"] == 1.0
    assert err <= TRUTH_BAR
    centroid = meshalign.icp(dS, dmesh, max_dist=C.MAX_DIST, init="centroid", n=20000, max_iter=1)
    assert centroid["iterations"] == 1 and np.isfinite(centroid["inlier_rmse"])


# ---- 8. aligned_scores ----------------------------------------------------------------------------------------------------------

def test_aligned_scores_of_a_moved_copy(hip_lib):
    from lara_amd import evaluate, meshalign, meshdist
    V, F = R.warped_icosphere(3)
    T = R.rigid(10, t=C.STARTS[10])
    inv = np.linalg.inv(T)
    moved = (V.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    mesh, pred = (_t(V), _t(F)), (_t(moved), _t(F))
    n = 20000
    before = meshdist.mesh_scores(pred, mesh, n=n)
    itself = meshdist.mesh_scores(mesh, mesh, n=n)
    after = meshalign.aligned_scores(pred, mesh, n=n, distance="triangle", max_dist=C.MAX_DIST)
    same = meshalign.aligned_scores(mesh, mesh, n=n, distance="triangle", max_dist=C.MAX_DIST)
    off = float(np.abs(same["alignment"]["transformation"] - np.eye(4)).max())
    bar = min(C.DEVICE_BAR.values())
    _note("8 aligned_scores, triangle distances", f"chamfer before {before['chamfer']:.4e}, after {after['chamfer']:.4e}, the mesh against "
          f"itself {itself['chamfer']:.4e}: after / itself = {after['chamfer'] / itself['chamfer']:.3f} (bar 4), before / after = "
          f"{before['chamfer'] / after['chamfer']:.3e} (bar 100); identity move: max |T - I| {off:.3e} = {off / bar:.3f} of the bar")
    assert after["distance"] == "triangle" and after["alignment"]["converged"]
    ev = evaluate.Evaluator(4)
    ev.add_geometry("a", after)
    assert ev.summary()["chamfer_mean"] == after["chamfer"]
    assert before["chamfer"] > 100 * after["chamfer"]
    assert after["chamfer"] <= 4 * itself["chamfer"]
    assert off <= bar


# ---- 9. the bench tool ----------------------------------------------------------------------------------------------------------

def test_bench_tool_runs_at_its_quick_size(hip_lib, tmp_path):
    out = tmp_path / "bench.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "meshalign_bench.py"), "--quick", "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(run.stdout.strip().splitlines()[-1]) == res
    assert res["n"] == 20000 and res["T"] <= 20000 and res["fallback_share"] <= 0.01
    for key in ("transform_ms", "query_ms", "accumulate_ms", "solve_plane_host_ms", "solve_point_host_ms"):
        assert res[key] > 0
    assert res["binding_stage"] in ("transform_ms", "query_ms", "accumulate_ms", "solve_plane_host_ms")
    assert res["icp"]["converged"] and res["icp"]["fitness"] == 1.0 and res["icp"]["max_abs_error_against_the_known_motion"] <= TRUTH_BAR
    assert res["torch_operators"]["kept_pairs_equal"] and res["torch_operators"]["transform_and_sums_ms"] > 0
