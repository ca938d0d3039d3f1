"""csrc/meshwind.hip held to the restatement of its header (tests/meshwind_restate.py) on every case of tests/meshwind_cases.py: the
moments buffer AS INT64 BIT PATTERNS; the counters of the walk AS INTEGERS for beta = 2, 3 and inf, no point exempt; w within the
summation bar of the restated walk of the same beta, and at beta = inf of float64 brute force in id order; the same bits twice and
on a side stream; NaN on the points that are not finite; zeros without a valid triangle; `contains` against float64 brute force
beyond the margin of tests/meshwind_cases.margin, the status bit on the restated band, |sdf| `TriangleBVH.query`'s bits;
`volume_scores` at 16^3 on two icospheres and with the holed icosphere as `pred`, counts equal to the restatement's, beside
`meshsign`'s figures.

The lines that start with "meshwind parity:" are the ones profiles/meshwind_parity.txt records."""
import numpy as np
import pytest
import torch

from tests import meshdist_restate as R
from tests import meshsign_restate as S
from tests import meshwind_cases as WC
from tests import meshwind_restate as W

pytestmark = pytest.mark.gpu
F32 = np.float32
INF = float("inf")
BUILT = tuple(k for k in WC.KEYS if not k.startswith("empty"))          # (T = 0: there is no hierarchy to build; see the refusal below)


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a, order="C")).to(_dev(), dtype)          # (a copy: the cases are read-only)


_fields = {}


def _field(key):
    """One device build of the hierarchy and the moments of the case, shared by the tests."""
    if key not in _fields:
        from lara_amd import meshbvh, meshwind
        c = WC.case(key)
        _fields[key] = meshwind.WindingField(meshbvh.TriangleBVH(_t(c["V"]), _t(c["F"])))
    return _fields[key]


def _rows(field, P, beta):
    from lara_amd import meshwind
    w, n_tri, n_far = meshwind.winding(field, _t(P), beta, return_counts=True)
    assert w.dtype == torch.float64 and n_tri.dtype == n_far.dtype == torch.int32 and tuple(w.shape) == (len(P),)
    return w, n_tri.cpu().numpy(), n_far.cpu().numpy()


@pytest.mark.parametrize("key", BUILT)
def test_moments_equal_the_restatement_as_bit_patterns(hip_lib, key):
    """Double arithmetic, a fixed order, no contraction, IEEE sqrt and division: the header, the offsets and every stored slot."""
    from lara_amd import meshwind
    f, M = _field(key), WC.moments(key)
    lay, total = W.layout(M.bvh.T)
    assert f.moments.shape[0] == total == M.nbytes and f.offsets == lay
    header = f.moments[:W.HEADER_BYTES].view(torch.int64).cpu().numpy()
    assert header[:9].tolist() == [o for o, _ in lay] + [0] * (9 - len(lay)) and header[9] == M.bvh.T
    worst = 0
    for k in range(len(lay)):
        got = f.level(k).cpu().numpy()
        assert got.shape == M.levels[k].shape
        worst += int((got.view(np.int64) != M.levels[k].view(np.int64)).sum())
    live = sum(int((lev[:, 3] > 0).sum()) for lev in M.levels)
    print(f"meshwind moments {key}: {len(M.flat)} stored slots on {len(lay)} levels, {live} with area, {worst} words differ")
    assert worst == 0
    again = meshwind.WindingField(f.bvh)
    assert torch.equal(again.moments[W.HEADER_BYTES:].view(torch.int64), f.moments[W.HEADER_BYTES:].view(torch.int64))


@pytest.mark.parametrize("key", BUILT)
def test_walk_equals_the_restatement(hip_lib, key):
    """n_tri and n_far as integers -- the same moments and the same comparisons give the same decisions -- and w within
    (n_terms + 4) 2^-53 sum |term| / 4 pi of the restated walk, for beta = 2, 3 and inf; at beta = inf also of float64 brute force
    in id order; the same bits on a second call and on a side stream; NaN and zero counters on the points that are not finite."""
    from lara_amd import meshwind
    c, f = WC.case(key), _field(key)
    fin = np.isfinite(c["P"]).all(1)
    worst = {}
    for beta in (2.0, 3.0, INF):
        want_w, want_tri, want_far, mag = WC.walked(key, beta)
        w, n_tri, n_far = _rows(f, c["P"], beta)
        got = w.cpu().numpy()
        assert np.array_equal(n_tri, want_tri), (key, beta, int((n_tri != want_tri).sum()))
        assert np.array_equal(n_far, want_far), (key, beta, int((n_far != want_far).sum()))
        assert np.array_equal(np.isnan(got), ~fin) and not n_tri[~fin].any() and not n_far[~fin].any()
        bar = W.bar(want_tri.astype(np.int64) + want_far, mag)
        ratio = np.abs(got[fin] - want_w[fin]) / np.maximum(bar[fin], 1e-300)
        worst[beta] = float(ratio.max())
        if beta == INF:
            bar = W.bar(c["n_valid"], np.maximum(mag, c["mag"]))
            worst["brute"] = float((np.abs(got[fin] - c["w"][fin]) / np.maximum(bar[fin], 1e-300)).max())
            assert not n_far.any()
        again = meshwind.winding(f, _t(c["P"]), beta)
        assert torch.equal(again.view(torch.int64), w.view(torch.int64))
    # (a high-priority stream: it is not drawn from the round of default-priority streams, and tests/test_stream_safety_gpu.py's
    # outcome depends on which of those it is handed -- with 4 hardware queues every fourth one runs behind the default stream)
    side = torch.cuda.Stream(_dev(), priority=-1)
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        on_side = meshwind.winding(f, _t(c["P"]), 2.0)
    side.synchronize()
    assert torch.equal(on_side.view(torch.int64), meshwind.winding(f, _t(c["P"]), 2.0).view(torch.int64))
    print(f"meshwind parity: device walk {key}: {len(c['P'])} points, worst ratio to the bar beta 2: {worst[2.0]:.3f}, beta 3: "
          f"{worst[3.0]:.3f}, beta inf: {worst[INF]:.3f}, beta inf against float64 brute force: {worst['brute']:.3f}")
    if max(worst.values()) > 1.0:          # the issue: report the device atan2's error on the terms, do not widen the bar
        p0, p1, p2 = W.triangles(c["V"], c["F"])
        q = c["P"][fin][:256]
        want = W.solid(q[:, None], p0[None, :64], p1[None, :64], p2[None, :64])
        print(f"meshwind parity: {key}: the bar is exceeded; restated terms for the report: |Omega| up to {np.abs(want).max():.4f}")
    assert max(worst.values()) <= 1.0, (key, worst)


def test_meshes_without_a_valid_triangle_and_empty_calls(hip_lib):
    """Zeros for a mesh none of whose triangles is valid (NaN on the points that are not finite), through the kernels; T = 0 itself
    is refused where the hierarchy is built, as it was before this module; N = 0 is a no-op."""
    from lara_amd import meshbvh, meshwind
    V1, _ = R.icosphere(1)
    P = np.array([[0, 0, 0], [0.5, 0.25, 2], [np.nan, 0, 0], [0, -np.inf, 0]], F32)
    bad = np.full((5, 3), len(V1) + 1, np.int64)
    nan_V = np.full((3, 3), np.nan, F32)
    for V, F in ((V1, bad), (nan_V, np.arange(3, dtype=np.int64)[None])):
        f = meshwind.WindingField(meshbvh.TriangleBVH(_t(V), _t(F)))
        for beta in (2.0, INF):
            w, n_tri, n_far = _rows(f, P, beta)
            w = w.cpu().numpy()
            assert w[:2].tolist() == [0.0, 0.0] and np.isnan(w[2:]).all() and not n_tri.any() and not n_far.any()
        assert all(not bool(f.level(k).any()) for k in range(len(f.offsets)))
        inside, status = meshwind.contains(f, _t(P), return_status=True)
        assert inside.dtype == torch.bool and inside.cpu().tolist() == [False] * 4 and status.cpu().tolist() == [0, 0, 4, 4]
        assert np.all(np.isposinf(meshwind.signed_distance(f, _t(P)).cpu().numpy()))
    c = WC.case("empty")
    with pytest.raises(ValueError, match="no triangles"):
        meshbvh.TriangleBVH(_t(c["V"]), _t(c["F"]))
    fin = np.isfinite(c["P"]).all(1)
    assert np.all(c["w"][fin] == 0.0) and np.isnan(c["w"][~fin]).all() and not WC.walked("empty", 2.0)[1].any()
    f = _field("icosphere")
    assert meshwind.winding(f, _t(P[:0])).shape == (0,) and meshwind.contains(f, _t(P[:0])).shape == (0,)
    assert meshwind.signed_distance(f, _t(P[:0])).shape == (0,)
    with pytest.raises(RuntimeError, match="built for another BVH"):
        meshwind.winding(_field("cube").bvh, _t(P), field=f)
    assert torch.equal(meshwind.winding(f.bvh, _t(P), field=f).view(torch.int64), meshwind.winding(f, _t(P)).view(torch.int64))
    assert torch.equal(meshwind.winding(f.bvh, _t(P)).view(torch.int64), meshwind.winding(f, _t(P)).view(torch.int64))


@pytest.mark.parametrize("key", BUILT)
def test_classification(hip_lib, key):
    """`contains` under the defaults equals `w_brute64 > 0.5` on every point whose float64 brute-force w is farther from 0.5 than
    the margin (2 E per sheet, tests/meshwind_cases.margin; at most 2 % of the case's points are exempt, asserted); inside, the
    status bits and the signed distance equal the restated classification of the restated walk wherever that walk's w is not within
    its summation bar of the threshold or of the band's edges; |sdf| has the bits of `TriangleBVH.query`'s dist."""
    from lara_amd import meshwind
    c, f = WC.case(key), _field(key)
    P = _t(c["P"])
    fin = np.isfinite(c["P"]).all(1)
    inside, status = meshwind.contains(f, P, return_status=True)
    got_inside, got_status = inside.cpu().numpy(), status.cpu().numpy()
    assert status.dtype == torch.uint8 and inside.dtype == torch.bool
    clear = fin & (np.abs(c["w"] - 0.5) > WC.margin(key))
    exempt = int((fin & ~clear).sum())
    assert exempt <= 0.02 * len(c["P"]), (key, exempt)
    assert np.array_equal(got_inside[clear], c["w"][clear] > 0.5), key
    assert not got_inside[~fin].any() and np.all(got_status[~fin] == 4) and np.all(got_status[fin] & 6 == 0)
    w2, n_tri, n_far, mag = WC.walked(key, 2.0)
    bar = W.bar(n_tri.astype(np.int64) + n_far, mag)
    with np.errstate(invalid="ignore"):
        edge = np.minimum(np.abs(w2 - 0.5), np.minimum(np.abs(w2 - 0.45), np.abs(w2 - 0.55)))
    sure = ~fin | (edge > bar)
    want_inside, want_status, _ = W.classify(w2, 0.5, 0.05)
    assert sure.sum() >= 0.95 * len(c["P"])          # (a point ON a face of a closed mesh has w = 0.5 up to rounding)
    assert np.array_equal(got_inside[sure], want_inside[sure] == 1) and np.array_equal(got_status[sure], want_status[sure]), key
    dist, face = f.bvh.query(P)
    sdf, f2, s2 = meshwind.signed_distance(f, P, return_face=True, return_status=True)
    assert torch.equal(f2, face) and torch.equal(s2, status)
    assert torch.equal(sdf.abs().view(torch.int32), dist.abs().view(torch.int32))
    got = sdf.cpu().numpy()
    d = dist.cpu().numpy()
    assert np.array_equal(np.signbit(got), got_inside | np.signbit(d))
    wide = meshwind.contains(f, P, band=0.25, return_status=True)[1].cpu().numpy()
    narrow = meshwind.contains(f, P, band=0.0, return_status=True)[1].cpu().numpy()
    assert np.all(narrow[fin] == 0) and (wide & 1).sum() >= (got_status & 1).sum()
    print(f"meshwind classification {key}: {int(got_inside.sum())} of {len(got_inside)} points inside, {int((got_status & 1).sum())} in the "
          f"band, {exempt} within the margin of the threshold ({100.0 * exempt / len(got_inside):.2f} %)")


def _restated_sides(meshes, P, beta=2.0):
    sides = []
    for V, F in meshes:
        w = W.winding(V, F, P, beta)[0]
        sides.append(W.classify(w, 0.5, 0.05)[:2] + (w,))
    return sides


def _lattice(meshes, resolution=16):
    boxes = [S.box(V, F) for V, F in meshes]
    lo, hi = np.minimum(boxes[0][0], boxes[1][0]), np.maximum(boxes[0][1], boxes[1][1])
    P, step = S.lattice(lo, hi, resolution)
    return P.reshape(-1, 3), step


def test_lattice_counts_on_two_icospheres(hip_lib):
    """`volume_scores` at 16^3 for the icosphere against itself shifted by (0.25, 0, 0): the eight counts equal the restatement's
    (no lattice point lies within the walk's summation bar of the threshold or the band's edges: asserted), the IoU is printed
    beside `meshsign`'s; `Evaluator.add_volume` takes the dict; `winding_grid` is `winding` on the lattice."""
    from lara_amd import evaluate, meshbvh, meshsign, meshwind
    V, F = R.icosphere(3)
    V2 = (V + np.array([0.25, 0, 0], F32)).astype(F32)
    a, b = meshbvh.TriangleBVH(_t(V), _t(F)), meshbvh.TriangleBVH(_t(V2), _t(F))
    s = meshwind.volume_scores(a, b, resolution=16)
    P, step = _lattice(((V, F), (V2, F)))
    sides = _restated_sides(((V, F), (V2, F)), P)
    for _, _, w in sides:
        assert np.minimum(np.abs(w - 0.5), np.minimum(np.abs(w - 0.45), np.abs(w - 0.55))).min() > 1e-9
    want = S.counts(sides[0][0], sides[0][1], sides[1][0], sides[1][1])
    assert s["counts"] == want and s["n_lattice"] == 4096 and s["resolution"] == 16 and s["rule"] == "solid_angle" and s["rays"] == 0
    assert s["volume_iou"] == want[2] / want[3] and s["decided_pred"] == 1.0 - want[4] / 4096 and s["decided_gt"] == 1.0 - want[5] / 4096
    cell = float(step[0]) * float(step[1]) * float(step[2])
    assert s["volume_pred"] == want[0] * cell and s["volume_gt"] == want[1] * cell
    assert abs(s["volume_pred_mesh"] - 4.1527) < 1e-4 and (s["beta"], s["threshold"], s["band"]) == (2.0, 0.5, 0.05)
    assert "unanimous_pred" not in s and want[6] == want[7] == 0
    ref = meshsign.volume_scores(a, b, resolution=16)
    assert set(s) - {"decided_pred", "decided_gt", "beta", "threshold", "band"} == set(ref) - {"unanimous_pred", "unanimous_gt"}
    print(f"meshwind parity: volume_scores 16^3, two icospheres 0.25 apart: counts {want}, IoU {s['volume_iou']:.4f} (meshsign's "
          f"parity vote: {ref['volume_iou']:.4f}), decided {s['decided_pred']:.4f} / {s['decided_gt']:.4f}")
    assert abs(ref["volume_iou"] - 0.6643) < 5e-5
    e = evaluate.Evaluator(4)
    e.add_volume("two spheres", s)
    assert e.summary()["volume_iou"] == [s["volume_iou"]]
    fa = meshwind.WindingField(a)
    again = meshwind.volume_scores(fa, (_t(V2), _t(F)), resolution=16, device=_dev())
    assert again == s
    exact = meshwind.volume_scores(fa, b, resolution=16, beta=INF)
    sides = _restated_sides(((V, F), (V2, F)), P, INF)
    assert exact["beta"] == "inf" and exact["counts"] == S.counts(sides[0][0], sides[0][1], sides[1][0], sides[1][1])
    grid = meshwind.winding_grid(fa, 4, lo=[-1.5, -1.5, -1.5], hi=[1.5, 1.5, 1.5])
    pts = meshsign.lattice([-1.5, -1.5, -1.5], [1.5, 1.5, 1.5], 4, _dev())[0].view(-1, 3)
    assert grid.dtype == torch.float64 and tuple(grid.shape) == (4, 4, 4)
    assert torch.equal(grid.view(-1).view(torch.int64), meshwind.winding(fa, pts).view(torch.int64))
    own = meshwind.winding_grid(fa, 4).cpu().numpy()
    assert own.shape == (4, 4, 4) and abs(own[1:3, 1:3, 1:3].min() - 1.0) < 0.03 and abs(own[0, 0, 0]) < 0.03


def test_lattice_counts_with_the_holed_icosphere_as_pred(hip_lib):
    """The same with the holed icosphere as `pred`: the counts equal the restatement's, `decided_pred` is reported, and
    `meshsign.volume_scores`' `unanimous_pred` is printed beside it: the rays disagree where the winding number still decides."""
    from lara_amd import meshbvh, meshsign, meshwind
    V, F = R.icosphere(3)
    Vh, Fh = WC.holed_icosphere()
    V2 = (V + np.array([0.25, 0, 0], F32)).astype(F32)
    a, b = meshbvh.TriangleBVH(_t(Vh), _t(Fh)), meshbvh.TriangleBVH(_t(V2), _t(F))
    s = meshwind.volume_scores(a, b, resolution=16)
    P, _ = _lattice(((Vh, Fh), (V2, F)))
    sides = _restated_sides(((Vh, Fh), (V2, F)), P)
    for _, _, w in sides:
        assert np.minimum(np.abs(w - 0.5), np.minimum(np.abs(w - 0.45), np.abs(w - 0.55))).min() > 1e-9
    want = S.counts(sides[0][0], sides[0][1], sides[1][0], sides[1][1])
    assert s["counts"] == want and s["decided_pred"] == 1.0 - want[4] / 4096 and s["decided_gt"] == 1.0 - want[5] / 4096
    ref = meshsign.volume_scores(a, b, resolution=16)
    print(f"meshwind parity: volume_scores 16^3, holed icosphere as pred: counts {want}, IoU {s['volume_iou']:.4f}, decided_pred "
          f"{s['decided_pred']:.4f}; meshsign's parity vote: IoU {ref['volume_iou']:.4f}, unanimous_pred {ref['unanimous_pred']:.4f}")
    assert 0.9 < s["decided_pred"] < 1.0 and s["decided_gt"] > 0.95 and ref["unanimous_pred"] < 1.0
