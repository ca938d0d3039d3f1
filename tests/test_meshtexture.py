"""include/lara_meshtexture.h without a GPU, through the library's host twins (which run csrc/texatlas.h, the functions the
kernels run): the header's constants held to the module's; the layout's owner and (a, b) tables against a plain double loop; the
footprint property of the atlas -- a bilinear read inside a triangle touches only texels the triangle owns -- over a dense barycentric
sample of every triangle for S = 3, 4, 7, 8; `corner_uvs`, points and anchors equal to the restatement (tests/meshtexture_restate.py)
AS BIT PATTERNS; the bake's texture, view and alpha equal exactly and its weight as bits, on every case of tests/meshtexture_cases.py,
in both blend modes, with and without a mask, with fallback colours and with `fill`; `sample` as bits; the PNG and the OBJ / MTL
round trips; the refusals; the extractor's new keywords; and the tooth: on the icosphere under a colour field of wave number 20 the
baked atlas, read back at the hit points of a held-out view, misses the field by at most 0.25 of what barycentric vertex colours do.

There is no tolerance in this file except the tooth's cap, which is the issue's.  The lines that start with "meshtexture parity:"
are the ones profiles/meshtexture_parity.txt records."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from lara_amd import _native
from tests import meshtexture_cases as TC
from tests import meshtexture_restate as X

F32 = np.float32
PATCHES = (3, 4, 7, 8)


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a, order="C")).to(dtype=dtype)          # (a copy: the cases are read-only)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _host_bake(c, kw, **more):
    from lara_amd import meshtexture as MT
    kw = TC.bake_arguments(c, kw)
    m, vc = kw.pop("mask"), kw.pop("vertex_colors")
    L = c["layout"]
    return MT.bake(_t(c["V"]), _t(c["F"]), _t(c["images"]), np.array(c["ixt"]), np.array(c["c2w"]), patch=L[0], width=L[2],
                   occlusion=False, host=True, mask=None if m is None else _t(m), vertex_colors=None if vc is None else _t(vc), **kw, **more)


def test_header_constants_equal_the_modules():
    """The limits and blend modes of include/lara_meshtexture.h equal the module's; every entry but the size query either takes
    the stream or is a host twin."""
    from lara_amd import meshray, meshtexture as MT
    from tests import test_abi_cpu as abi
    own = {name: sig for name, sig in _native._SIGS.items() if name.startswith("lara_meshtexture_")}
    assert len(own) == 7
    for name, (_, _, has_stream) in own.items():
        assert has_stream or name.endswith("_host") or name == "lara_meshtexture_atlas_size", name
    text = open(os.path.join(abi.ROOT, "include", "lara_meshtexture.h")).read()
    for macro, value in (("MIN_PATCH", MT.MIN_PATCH), ("MAX_PATCH", MT.MAX_PATCH), ("MAX_VIEWS", MT.MAX_VIEWS), ("MAX_POWER", MT.MAX_POWER),
                         ("WEIGHTED", MT.BLENDS["weighted"]), ("BEST", MT.BLENDS["best"])):
        assert f"#define LARA_MESHTEXTURE_{macro} {value}\n" in text
    assert MT.MAX_VIEWS == meshray.MAX_EYES == X.MAX_VIEWS == 64


def test_the_unit_is_built_without_contraction():
    text = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "Makefile")).read()
    assert "FLAGS_meshtexture := -ffp-contract=off\n" in text and " meshtexture " in text.split("OBJS")[1].splitlines()[0]


def test_the_module_is_opt_in():
    """Importing the package, the extractor's module and the ray module does not import this one."""
    import subprocess
    code = "import sys, lara_amd, lara_amd.mesh, lara_amd.meshray; sys.exit(1 if 'lara_amd.meshtexture' in sys.modules else 0)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


# ---- the layout -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,T", [(3, 3, 11), (4, 3, 11), (7, 3, 11), (8, 3, 11), (8, 1, 5), (3, 4, 1), (5, 2, 0), (4, 5, 64)])
def test_owner_and_local_coordinates_equal_a_plain_double_loop(hip_lib, S, C, T):
    """Triangle f of a probe mesh has the vertices (0, 0, f), (S - 2, 0, f), (0, S - 2, f): a texel's point is then (a, b, f), and the
    host entry's face, a and b are compared with the double loop's as integers."""
    from lara_amd import meshtexture as MT
    L = MT.atlas(T, S, C * (S + 1))
    face, a, b = X.owner_tables(S, C, T)
    assert L == X.atlas(T, S, C * (S + 1)) == (S, C, face.shape[1], face.shape[0])
    V = np.array([[[0, 0, f], [S - 2, 0, f], [0, S - 2, f]] for f in range(max(T, 1))], F32).reshape(-1, 3)
    F = np.arange(3 * T, dtype=np.int64).reshape(T, 3)
    got, point, anchor = (x.numpy() for x in MT.texels(L, _t(V), _t(F), host=True))
    assert np.array_equal(got, face)
    own = face >= 0
    assert np.array_equal(point[own], np.stack([a[own], b[own], face[own]], 1).astype(F32))
    assert np.isnan(point[~own]).all() and np.isnan(anchor[~own]).all()
    # every triangle owns S (S + 1) / 2 texels, and the gutter row a + b = S - 1 is S of them
    assert all(int((face == f).sum()) == S * (S + 1) // 2 and int(((face == f) & (a + b == S - 1)).sum()) == S for f in range(T))
    if T % 2:
        assert int((face == -1).sum()) >= S * (S + 1) // 2


def test_atlas_sizes_and_refusals(hip_lib):
    from lara_amd import meshtexture as MT
    for T in (0, 1, 2, 11, 1280, 9328):
        for kw in (dict(), dict(patch=3), dict(patch=7, width=100), dict(max_texels=1 << 20), dict(max_texels=1 << 16, width=256)):
            want = X.atlas(T, kw.get("patch"), kw.get("width"), kw.get("max_texels"))
            if want is None:
                with pytest.raises(ValueError, match="no patch"):
                    MT.atlas(T, **kw)
                continue
            L = MT.atlas(T, **kw)
            assert L == want
            size = _native.host_array("l", 2)
            _native.call("lara_meshtexture_atlas_size", None, L[0], L[1], T, size)
            assert (size[0], size[1]) == L[2:]
            if "max_texels" in kw:
                assert L[2] * L[3] <= kw["max_texels"]
                bigger = X.atlas(T, L[0] + 1, kw.get("width"))
                assert bigger[2] * bigger[3] > kw["max_texels"] or L[0] == MT.MAX_PATCH
    assert MT.atlas(0, 5)[2:] == (6, 5)
    with pytest.raises(ValueError, match="no patch"):
        MT.atlas(9328, max_texels=1 << 14)
    for bad in (2, 0, -1, 4097):
        with pytest.raises(ValueError, match="patch size"):
            MT.atlas(10, bad)
    with pytest.raises(ValueError, match="not both"):
        MT.atlas(10, 4, max_texels=1000)
    with pytest.raises(ValueError, match="2\\^30 texels"):
        MT.atlas(1 << 25, 8)
    with pytest.raises(ValueError, match="T must be"):
        MT.atlas(-1)
    size = _native.host_array("l", 2)
    for S, C, T in ((2, 1, 1), (4097, 1, 1), (4, 0, 1), (4, 1, -1), (8, 4096, 1 << 26)):
        assert hip_lib.lara_meshtexture_atlas_size(S, C, T, size) == -1
    assert hip_lib.lara_meshtexture_atlas_size(4, 1, 1, None) == -1


@pytest.mark.parametrize("S", PATCHES)
def test_a_bilinear_read_inside_a_triangle_touches_only_its_own_texels(hip_lib, S):
    """T = 11, C = 3: every tap of weight > 0 of the restated sampler lies on a texel the double loop gives to the face, for every
    face and a dense barycentric sample (the lattice of step 1 / 24, corners and edges included, and 400 points off it); and the
    host sampler, reading an atlas that is 0 on the face's texels and 255 everywhere else, returns exactly 0."""
    from lara_amd import meshtexture as MT
    T, C = 11, 3
    L = X.atlas(T, S, C * (S + 1))
    owner, _, _ = X.owner_tables(S, C, T)
    bary = TC.dense_bary()
    for f in range(T):
        face = np.full(len(bary), f, np.int64)
        x, y, wt = X.taps(L, face, bary)
        assert (x >= 0).all() and (x < L[2]).all() and (y >= 0).all() and (y < L[3]).all()
        foreign = (owner[y, x] != f) & (wt > 0)
        assert not foreign.any(), (S, f, int(foreign.sum()))
        assert np.abs(wt.sum(1) - 1).max() < 1e-15
        tex = np.where((owner == f)[:, :, None], 0, 255).astype(np.uint8).repeat(4, 2)
        got = MT.sample(L, T, _t(tex), _t(face.astype(np.int32)), _t(bary), alpha=True, host=True).numpy()
        assert not got.any()
    # the corners read their own texel alone: the atlas position of `corner_uvs`
    uv = X.corner_uvs(L, T).astype(np.float64)
    corners = np.eye(3, dtype=F32)
    for f in range(T):
        x, y, wt = X.taps(L, np.full(3, f), corners)
        assert np.array_equal(wt[:, 0], np.ones(3)) and np.abs((x[:, 0] + 0.5) / L[2] - uv[f, :, 0]).max() < 1e-7
        assert np.abs((1 - (y[:, 0] + 0.5) / L[3]) - uv[f, :, 1]).max() < 1e-7


@pytest.mark.parametrize("key", TC.KEYS)
def test_corner_uvs_points_and_anchors_equal_the_restatement_as_bit_patterns(hip_lib, key):
    from lara_amd import meshtexture as MT
    c = TC.case(key)
    L, T = c["layout"], len(c["F"])
    assert np.array_equal(bits(MT.corner_uvs(L, T).numpy()), bits(X.corner_uvs(L, T)))
    face, point, anchor = X.texels(L, c["V"], c["F"])
    got = [x.numpy() for x in MT.texels(L, _t(c["V"]), _t(c["F"]), host=True)]
    assert got[0].dtype == np.int32 and np.array_equal(got[0], face)
    assert np.array_equal(bits(got[1]), bits(point)) and np.array_equal(bits(got[2]), bits(anchor))
    own = face >= 0
    assert np.isfinite(point[own]).all() and np.isfinite(anchor[own]).all() and np.isnan(point[~own]).all()
    if key.startswith("bad_triangles"):
        from tests.meshdist_cases import BAD
        assert not np.isin(face, BAD).any() and (face == 4).any()


@pytest.mark.parametrize("key", TC.KEYS)
def test_bake_equals_the_restatement(hip_lib, key):
    """texture (alpha with it) and view as integers, weight as bits, under every variant of tests/meshtexture_cases.VARIANTS."""
    c = TC.case(key)
    for name, kw in TC.VARIANTS:
        want = TC.restated(key, name)
        tex = _host_bake(c, kw)
        assert np.array_equal(tex.texture.numpy(), want[0]), (key, name, int((tex.texture.numpy() != want[0]).sum()))
        assert np.array_equal(bits(tex.weight.numpy()), bits(want[1])), (key, name)
        assert tex.view.dtype == torch.int32 and np.array_equal(tex.view.numpy(), want[2]), (key, name)
        own, alpha = tex.face.numpy() >= 0, want[0][..., 3]
        assert set(np.unique(alpha)) <= {0, 255} and not alpha[~own].any() and not want[1][alpha == 0].any()
        assert tex.coverage == (float((alpha[own] == 255).mean()) if own.any() else 0.0)
    if key in ("odd S4 V0", "empty S4 C2"):
        assert not TC.restated(key, "weighted")[0][..., 3].any() and tex.coverage == 0.0


def test_what_the_views_do(hip_lib):
    """On the icosphere: the view inside the sphere colours nothing unless `two_sided`; the view whose border cuts the sphere
    colours some; `best` names the view of largest weight; fallback texels
    carry the vertex colours' blend or `fill`."""
    c = TC.case("icosphere S8")
    only = lambda e: np.full(c["mask"].shape, np.int64(1) << np.int64(e))
    k = dict(c)
    for e, two_sided, some in ((4, False, False), (4, True, True), (5, False, True)):
        k["mask"] = only(e)
        t = _host_bake(k, dict(blend="best", mask=True, two_sided=two_sided))
        view = t.view.numpy()
        assert set(np.unique(view)) <= {-1, e} and bool((view == e).any()) == some
    best, weighted = TC.restated("icosphere S8", "best"), TC.restated("icosphere S8", "weighted")
    assert np.array_equal(best[2] >= 0, weighted[2] > 0) and weighted[2].max() >= 2
    assert (best[1] <= weighted[1]).all()
    filled = TC.restated("icosphere S8", "best masked fill two-sided")
    own = X.texels(c["layout"], c["V"], c["F"])[0] >= 0
    assert np.array_equal(np.unique(filled[0][~own | (filled[0][..., 3] == 0)][:, :3], axis=0), X.quantize(np.array([[0.2, 0.5, 0.9]], F32).astype(np.float64)))


@pytest.mark.parametrize("key", ["icosphere S8", "uv_sphere S4 C50", "bad_triangles S4 C5", "odd S7 C4", "odd S8 C1", "empty S4 C2"])
def test_sample_equals_the_restatement_as_bit_patterns(hip_lib, key):
    from lara_amd import meshtexture as MT
    c = TC.case(key)
    L, T = c["layout"], len(c["F"])
    tex = TC.restated(key, "weighted masked colours")[0]
    g = np.random.default_rng(7)
    bary = np.concatenate([TC.dense_bary(12), (g.random((300, 3)) * 1.4 - 0.2).astype(F32), np.array([[np.nan, np.nan, 0.5], [0, 2, -1]], F32)])
    face = g.integers(-1, T + 2, len(bary)).astype(np.int32)
    for alpha in (False, True):
        want = X.sample(L, T, tex, face, bary, alpha, (0.1, 0.2, 0.3))
        got = MT.sample(L, T, _t(tex), _t(face), _t(bary), alpha, (0.1, 0.2, 0.3), host=True).numpy()
        assert got.shape == (len(bary), 4 if alpha else 3) and np.array_equal(bits(got), bits(want))
        out = (face < 0) | (face >= T)
        assert np.array_equal(got[out][:, :3], np.broadcast_to(np.array([0.1, 0.2, 0.3], F32), (int(out.sum()), 3)))


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def test_png_round_trip(tmp_path):
    from lara_amd import meshtexture as MT
    g = np.random.default_rng(1)
    for shape in ((1, 1), (3, 5), (48, 216)):
        a = g.integers(0, 256, shape + (4,), dtype=np.uint8)
        p = str(tmp_path / "a.png")
        MT.write_png(p, a)
        assert np.array_equal(MT.read_png(p), a)
        data = open(p, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[-8:-4] == b"IEND"
    with pytest.raises(ValueError, match="uint8"):
        MT.write_png(p, np.zeros((4, 4, 3), np.uint8))
    open(p, "wb").write(data[:40] + bytes([data[40] ^ 1]) + data[41:])
    with pytest.raises(ValueError, match="CRC"):
        MT.read_png(p)


@pytest.mark.parametrize("key", ["icosphere S3 C37", "odd S7 C4", "empty S4 C2"])
def test_textured_obj_round_trip(hip_lib, tmp_path, key):
    from lara_amd import meshtexture as MT
    c = TC.case(key)
    tex = _host_bake(c, dict(blend="weighted"))
    obj, mtl, png = MT.write_textured_obj(str(tmp_path / "mesh.obj"), c["V"], c["F"], tex)
    assert (obj, mtl, png) == tuple(str(tmp_path / n) for n in ("mesh.obj", "mesh.mtl", "mesh.png"))
    v, t, uv, rgba = MT.read_textured_obj(obj)
    assert v.tobytes() == np.ascontiguousarray(c["V"]).tobytes() and np.array_equal(t, c["F"])
    assert np.array_equal(bits(uv), bits(X.corner_uvs(c["layout"], len(c["F"])))) and np.array_equal(rgba, tex.texture.numpy())
    text = open(obj).read().splitlines()
    assert text[:2] == ["mtllib mesh.mtl", "usemtl atlas"] and sum(x.startswith("vt ") for x in text) == 3 * len(c["F"])
    assert "map_Kd mesh.png" in open(mtl).read().splitlines()
    if len(c["F"]):
        assert text[-1] == "f %d/%d %d/%d %d/%d" % tuple(x for k in range(3) for x in (c["F"][-1, k] + 1, 3 * len(c["F"]) - 2 + k))
    with pytest.raises(ValueError, match="written as .obj"):
        MT.write_textured_obj(str(tmp_path / "mesh.ply"), c["V"], c["F"], tex)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    from lara_amd import meshtexture as MT
    c = TC.case("odd S7 C4")
    V, F, I = _t(c["V"]), _t(c["F"]), _t(c["images"])
    ixt, c2w = np.array(c["ixt"]), np.array(c["c2w"])
    with pytest.raises(ValueError, match="at most 64 views"):
        MT.bake(V, F, torch.zeros(65, 4, 4, 3), np.zeros((65, 3, 3)), np.zeros((65, 4, 4)), host=True, occlusion=False)
    for bad in (torch.zeros(6, 48, 64), torch.zeros(6, 48, 64, 4), torch.zeros(6, 3, 48, 64)):
        with pytest.raises(ValueError, match=r"images \[V,H,W,3\]"):
            MT.bake(V, F, bad, ixt, c2w, host=True, occlusion=False)
    with pytest.raises(ValueError, match="patch size"):
        MT.bake(V, F, I, ixt, c2w, patch=2, host=True, occlusion=False)
    with pytest.raises(ValueError, match="blend is"):
        MT.bake(V, F, I, ixt, c2w, blend="median", host=True, occlusion=False)
    for power in (-1, 9):
        with pytest.raises(ValueError, match="power must be"):
            MT.bake(V, F, I, ixt, c2w, power=power, host=True, occlusion=False)
    with pytest.raises(RuntimeError, match="no visibility walk"):
        MT.bake(V, F, I, ixt, c2w, host=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        MT.bake(V, F, I, ixt, c2w)
    with pytest.raises(ValueError, match="one camera per image"):
        MT.bake(V, F, I[:3], ixt, c2w, host=True, occlusion=False)
    with pytest.raises(ValueError, match="not the one of"):
        MT.texels((7, 4, 32, 21), V, F, host=True)
    L = hip_lib
    assert L.lara_meshtexture_texels_host(2, 1, 1, 3, 1, 1, 1, 1, 1) == -1 and L.lara_meshtexture_texels_host(4, 1, 1, 3, None, 1, 1, 1, 1) == -1
    assert L.lara_meshtexture_texels(4, 1, 1, 3, 1, 1, None, 1, 1, None) == -1
    ok = dict(S=4, C=1, T=1, Nv=3, V=1, H=4, W=4, power=2, blend=0, near=0.0)

    def bake_rc(**kw):
        a = dict(ok, **kw)
        return L.lara_meshtexture_bake_host(a["S"], a["C"], a["T"], a["Nv"], 1, 1, 1, 1, 1, a["V"], a["H"], a["W"], 1, 1, 1, 1, None, a["near"], 0.1,
                                            a["power"], 0, a["blend"], None, 0.0, 0.0, 0.0, 1, 1, None if kw.get("no_view") else 1)
    for kw in (dict(S=2), dict(C=0), dict(T=-1), dict(V=65), dict(V=-1), dict(power=9), dict(power=-1), dict(blend=2), dict(near=float("nan")),
               dict(H=1 << 16, W=1 << 16), dict(no_view=True)):
        assert bake_rc(**kw) == -1, kw
    s = L.lara_meshtexture_sample_host
    assert s(4, 1, 1, 0, None, None, None, 3, 0.0, 0.0, 0.0, None) == 0
    assert s(4, 1, 1, 5, 1, 1, 1, 2, 0.0, 0.0, 0.0, 1) == -1 and s(4, 1, 1, -1, 1, 1, 1, 3, 0.0, 0.0, 0.0, 1) == -1
    assert s(4, 1, 1, 5, None, 1, 1, 3, 0.0, 0.0, 0.0, 1) == -1 and s(4, 1, 1, 1 << 30, 1, 1, 1, 3, 0.0, 0.0, 0.0, 1) == -1
    assert L.lara_meshtexture_sample(4, 1, 1, 5, 1, 1, 1, 3, 0.0, 0.0, 0.0, None, None) == -1


def test_extractor_keywords_and_refusals(tmp_path):
    from lara_amd import mesh
    saved = sys.modules.pop("lara_amd.meshtexture", None)
    try:
        ex = mesh.MeshExtractor.__new__(mesh.MeshExtractor)
        ply, obj = str(tmp_path / "m.ply"), str(tmp_path / "m.obj")
        for kw in (dict(texture_patch=6), dict(texture_max_texels=1 << 20)):
            with pytest.raises(ValueError, match="needs a .obj path"):
                ex.extract(ply, "gso", cams=[], **kw)
        with pytest.raises(ValueError, match="not both"):
            ex.extract(obj, "gso", cams=[], texture_patch=6, texture_max_texels=1 << 20)
        with pytest.raises(ValueError, match="texture_patch must be >= 3"):
            ex.extract(obj, "gso", cams=[], texture_patch=2)
        with pytest.raises(ValueError, match="texture_blend is"):
            ex.extract(obj, "gso", cams=[], texture_patch=6, texture_blend="median")
        with pytest.raises(ValueError, match="written by the host writer"):
            ex.extract(obj, "gso", cams=[], texture_patch=6, writer="device")
        with pytest.raises(ValueError, match="at most 64 views"):
            ex.extract(obj, "gso", cams=[None] * 65, texture_patch=6)
        assert "lara_amd.meshtexture" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["lara_amd.meshtexture"] = saved
    p = inspect.signature(mesh.MeshExtractor.extract).parameters
    assert [p[k].default for k in ("texture_patch", "texture_max_texels", "texture_blend")] == [None, None, "weighted"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("texture_patch", "texture_max_texels", "texture_blend"))


# ---- the tooth --------------------------------------------------------------------------------------------------------------------------
def test_a_baked_atlas_carries_what_vertex_colours_cannot(hip_lib):
    """The icosphere (1 280 faces) under the colour field of wave number 20, S = 8, 8 orbit views, one held-out view; the rays of
    the held-out view are cast in float64 on the host, and the atlas is read at their (face, barycentrics).  RMSE against the analytic
    colour of the same hit points <= 0.25 x the RMSE of the barycentric blend of exact vertex colours (the issue's cap; a perfect
    bake reaches 0.059).  Source views of 96 x 96: the restatement alone gives 0.128 there (0.200 at 64 x 64, 0.077 at 160 x 160), so
    the cap leaves room for the source images' resolution and no more.  The host bake is the restatement's, bit for bit."""
    from lara_amd import meshtexture as MT
    t = TC.tooth()
    L = X.atlas(len(t["F"]), 8)
    k, w2c, eyes = TC.camera_arrays(t["ixt"], t["c2w"])
    want = X.bake(L, t["V"], t["F"], t["images"], k, w2c, eyes)
    restated = TC.rmse(X.sample(L, len(t["F"]), want[0], t["face"], t["bary"]), t["truth"])
    vertex = TC.rmse(t["vertex_blend"], t["truth"])
    print(f"meshtexture parity: tooth, restatement: vertex colours RMSE {vertex:.4f}, atlas RMSE {restated:.4f}, ratio {restated / vertex:.4f}")
    assert restated <= TC.TOOTH_CAP * vertex
    tex = MT.bake(_t(t["V"]), _t(t["F"]), _t(t["images"]), np.array(t["ixt"]), np.array(t["c2w"]), patch=8, occlusion=False, host=True)
    assert tex.layout == L and np.array_equal(tex.texture.numpy(), want[0])
    got = TC.rmse(tex.sample(_t(t["face"]), _t(t["bary"])).numpy(), t["truth"])
    print(f"meshtexture parity: tooth, host entries: {len(t['face'])} hit points of the held-out view, sources {t['res'][0]}^2, atlas "
          f"{L[2]} x {L[3]}, coverage {tex.coverage:.4f}, atlas RMSE {got:.4f}, ratio {got / vertex:.4f} (cap {TC.TOOTH_CAP}, perfect bake "
          f"{TC.TOOTH_PERFECT})")
    assert got <= TC.TOOTH_CAP * vertex and vertex > 0.1
