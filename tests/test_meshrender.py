"""The float64 / integer restatement of include/lara_meshrender.h (tests/meshrender_restate.py) held to closed forms, and the
cases of tests/meshrender_cases.py held to what they are built to show -- no GPU.  tests/test_meshrender_gpu.py holds the
kernels to this restatement."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from lara_amd import meshrender
from tests import meshrender_cases as C
from tests import meshrender_restate as R

NEAR_TIE_CAP = 0.005        # the restatement alone, per case; the GPU test allows the kernels 1 %


def restate(case, view=0, mutate=None, triangles=None):
    vm, pm = C.matrices(case)
    t = case["triangles"] if triangles is None else np.asarray(triangles, np.int64)
    return R.render_view(case["vertices"], t, vm[view], pm[view], case["eyes"][view], case["H"], case["W"], case["znear"],
                         colors=case["colors"], mutate=mutate)


@pytest.fixture(scope="module")
def results():
    """Every view of every case, once."""
    out = {}
    for key, make in C.CASES.items():
        case = make()
        out[key] = (case, [restate(case, v) for v in range(len(case["cams"]))])
    return out


def test_fronto_parallel_quad_lands_on_its_pixels():
    """A quad on the plane z = 2 from pixel (4, 4) to (12, 12) of a 16 x 16 image: under pixel = ((ndc + 1) W - 1) / 2 its
    corners snap to 256 x those pixels exactly; it covers the samples 4..11 (the right and bottom edges own nothing), at depth
    2, with the normal (0, 0, -1) towards the camera at the origin, lit head-on."""
    W = H = 16
    cams, eyes = C.flat_camera(W, H)
    v = np.array([C.flat_vertex(4, 4, W, H), C.flat_vertex(12, 4, W, H), C.flat_vertex(12, 12, W, H), C.flat_vertex(4, 12, W, H)], np.float32)
    case = {"cams": cams, "eyes": eyes, "vertices": v, "triangles": np.array([[0, 1, 2], [0, 2, 3]]), "colors": None, "H": H,
            "W": W, "znear": 0.5}
    for tris in (case["triangles"], case["triangles"][:, ::-1]):          # either winding: the triangles are two-sided
        res, (sx, sy, z, zb) = restate(case, triangles=tris)
        assert sx.tolist() == [1024, 3072, 3072, 1024] and sy.tolist() == [1024, 1024, 3072, 3072] and z.tolist() == [2.0] * 4
        inside = np.zeros((H, W), bool)
        inside[4:12, 4:12] = True
        assert np.array_equal(res["face"] >= 0, inside) and np.array_equal(res["count"], inside.astype(int))
        assert np.all(res["depth"][inside] == 2.0) and np.all(res["depth"][~inside] == 0.0)
        assert np.allclose(res["normal"][inside], [0.0, 0.0, -1.0], atol=1e-15) and np.all(res["normal"][~inside] == 0.0)
        assert res["faces_eye"].all()
        # the diagonal's samples belong to exactly one of the two triangles
        assert sorted(set(res["face"][inside].tolist())) == [0, 1]
        # head light: pixel (8, 8) is the point (1/16, 1/16, 2), so n . l = 2 / sqrt(4 + 2 / 256)
        assert abs(res["colour"][8, 8, 2] - np.float32(0.8) * (0.25 + 0.75 * 2.0 / np.sqrt(4.0 + 2.0 / 256.0))) < 1e-12
        assert np.array_equal(R.quantize(res["colour"][0, 0]), np.round(np.float32([0.722, 0.376, 0.161]).astype(np.float64) * 255))


def test_fill_rule_enumerated_by_hand(results):
    case, views = results["a"]
    res, _ = views[0]
    got = sorted((int(x), int(y)) for y, x in zip(*np.nonzero(res["face"] >= 0)))
    assert got == case["expect"]["covered"] and len(got) == 10
    for x, y in ((6, 2), (2, 6), (4, 4), (5, 3), (3, 5)):                  # the hypotenuse's sample points and its two ends
        assert res["face"][y, x] == -1


def test_quantiser_rounds_ties_to_even_and_clamps():
    """The quantiser is np.round(255 x) clamped: exact ties go to the even code."""
    ties = (np.arange(0, 255) + 0.5) / 255.0 * 255.0 / 255.0
    x = np.concatenate([ties, [0.0, 0.2, 0.999, 1.0, 1.7, -0.3], np.linspace(0, 1, 1001)])
    assert np.array_equal(R.quantize(x), np.clip(np.round(x * 255.0), 0, 255).astype(np.uint8))
    assert R.quantize(np.array([0.5, 1.5, 2.5, 3.5]) / 255.0).tolist() == [int(np.round(v * 255.0)) for v in np.array([0.5, 1.5, 2.5, 3.5]) / 255.0]
    assert R.quantize([1.7, -0.3]).tolist() == [255, 0]
    assert np.round(0.5) == 0 and np.round(1.5) == 2 and np.round(2.5) == 2      # what "as np.round" means


def test_near_ties_stay_rare_in_every_case(results):
    """The share of covered pixels whose winner and runner-up lie closer than their fp32 depth bounds: at most 0.5 % in every
    case for the restatement alone, none at all where the case says so."""
    for key, (case, views) in results.items():
        for res, _ in views:
            covered = int((res["face"] >= 0).sum())
            excluded = int(R.near_tie(res).sum())
            assert excluded <= NEAR_TIE_CAP * covered, (key, excluded, covered)
            if case["zero_excluded"]:
                assert excluded == 0, key


def test_cases_show_what_they_are_built_for(results):
    for key, (case, views) in results.items():
        exp = case["expect"]
        for res, _ in views:
            if "faces" in exp:
                assert set(res["face"][res["face"] >= 0].tolist()) == exp["faces"], key
            if "outer_only" in exp:
                assert res["face"].max() < exp["outer_only"] and (res["face"] >= 0).sum() > 500
            if "info" in exp:
                assert res["info"].tolist() == exp["info"]
                alone, _ = restate(case, triangles=exp["same_as"])
                assert np.array_equal(alone["face"] >= 0, res["face"] >= 0) and np.array_equal(alone["depth"], res["depth"])
                assert np.array_equal(alone["colour"], res["colour"])
            assert res["faces_eye"].all(), key
            assert res["info"].sum() == len(case["triangles"])
    assert (results["j"][1][0][0]["face"] == -1).all() and results["j"][1][0][0]["info"].tolist() == [0, 0, 0, 0]
    for key in ("c", "d", "i", "k"):                                       # front and back faces: two-sided coverage
        assert max(int(res["count"].max()) for res, _ in results[key][1]) >= 2


def test_fan_and_strip_cover_each_sample_exactly_once(results):
    """Case (b) against an independent statement of the rule in exact rationals: a sample is covered by a triangle when the
    sample moved by (e, e^2), e = 2^-40 pixel units, lies strictly inside it."""
    case, ((res, (sx, sy, _, _)),) = results["b"]
    e = Fraction(1, 2 ** 40)
    union = np.zeros((case["H"], case["W"]), int)
    for tri in case["triangles"]:
        x, y = [Fraction(int(sx[i])) for i in tri], [Fraction(int(sy[i])) for i in tri]
        for py in range(case["H"]):
            for px in range(case["W"]):
                qx, qy = px * 256 + e, py * 256 + e * e
                s = [(x[b] - x[a]) * (qy - y[a]) - (y[b] - y[a]) * (qx - x[a]) for a, b in ((0, 1), (1, 2), (2, 0))]
                union[py, px] += all(v > 0 for v in s) or all(v < 0 for v in s)
    assert union.max() == 1 and union.sum() > 200
    assert np.array_equal(res["count"], union)
    assert res["face"][16, 16] >= 0 and union[16, 16] == 1                 # the fan's hub is a sample point: one owner


def test_each_mutation_fails_exactly_what_it_touches(results):
    (case_a, ((a, _),)), (case_b, ((b, _),)) = results["a"], results["b"]
    (case_e, ((e, _),)), (case_c, c_views) = results["e"], results["c"]
    c = c_views[0][0]
    # every edge inclusive: more samples in (a), double coverage in (b); depths of the samples covered before and ties untouched
    ma, mb, me = restate(case_a, mutate="inclusive")[0], restate(case_b, mutate="inclusive")[0], restate(case_e, mutate="inclusive")[0]
    assert (ma["face"] >= 0).sum() == 15 and mb["count"].max() >= 2
    assert np.array_equal(ma["depth"][a["face"] >= 0], a["depth"][a["face"] >= 0])
    assert set(me["face"][me["face"] >= 0].tolist()) == {0, 1}
    # z linear on the screen: coverage as before, the depths of the sphere move by far more than their bound; flat cases keep theirs
    mc = restate(case_c, mutate="screen_linear")[0]
    assert np.array_equal(mc["count"], c["count"])
    hit = c["face"] >= 0
    moved = np.abs(mc["depth"] - c["depth"])[hit] > 100 * c["depth_bound"][hit]
    assert moved.mean() > 0.5            # (the two agree at the vertices and differ most at a triangle's centre)
    assert np.array_equal(restate(case_a, mutate="screen_linear")[0]["depth"], a["depth"])
    # ties to the higher id: only the coincident quads change
    assert set(restate(case_e, mutate="tie_high")[0]["face"][e["face"] >= 0].tolist()) == {2, 3}
    mt = restate(case_c, mutate="tie_high")[0]
    assert np.array_equal(mt["face"], c["face"]) and np.array_equal(mt["depth"], c["depth"])
    assert np.array_equal(restate(case_b, mutate="tie_high")[0]["face"], b["face"])


def test_workspace_layout_and_refused_sizes(hip_lib):
    """Host code of the library: the four sections follow one another, 256-byte aligned, inside the workspace."""
    n, H, W, Nv, T = 3, 37, 29, 1001, 1999
    offs = (ctypes.c_int64 * 4)()
    assert hip_lib.lara_meshrender_section_offsets(n, H, W, Nv, T, offs) == 0
    o = list(offs)
    total = hip_lib.lara_meshrender_workspace_bytes(n, H, W, Nv, T)
    assert o[0] == 0 and all(v % 256 == 0 for v in o)
    assert all(b - a >= need for a, b, need in zip(o, o[1:] + [total], (n * Nv * 16, n * H * W * 8, n * T * 4, n * 8)))
    assert hip_lib.lara_meshrender_workspace_bytes(1, 16, 16, 0, 0) > 0
    for bad in ((-1, 16, 16, 4, 4), (1, 0, 16, 4, 4), (65536, 1, 1, 4, 4), (8, 16384, 16384, 4, 4), (1, 16, 16, 1 << 30, 4)):
        assert hip_lib.lara_meshrender_workspace_bytes(*bad) == -1
    assert hip_lib.lara_meshrender_section_offsets(1, 16, 16, 4, 4, None) == -1
    shading = (ctypes.c_float * 8)()
    assert hip_lib.lara_meshrender_views(1, 16, 16, 4, 4, *([None] * 6), 0.5, shading, 0, *([None] * 6), None, None) == -1


def test_there_is_no_cpu_path():
    case = C.case_a()
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshrender.render_mesh_views(case["cams"], torch.from_numpy(case["vertices"]), torch.from_numpy(case["triangles"]))
    assert meshrender.ALBEDO == (0.25, 0.5, 0.8) and meshrender.BACKGROUND == (0.722, 0.376, 0.161)
