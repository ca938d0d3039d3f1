"""csrc/meshtexture.hip held to its host twins and to the restatement of its header (tests/meshtexture_restate.py) on every case of
tests/meshtexture_cases.py: face, view and the texture's bytes AS INTEGERS, points, anchors, weights and samples AS BIT PATTERNS -- the
contract `meshtopo` and `meshalign` hold for double arithmetic with division and square root --, twice and on a side stream; the
visibility mask the bake is fed equal to `meshray`'s own restatement; the two-layer mesh, whose inner layer no view sees; the T = 0
and V = 0 outputs; `render_textured` on the tooth of tests/test_meshtexture.py; and `MeshExtractor.extract(texture_patch=6)` with a
stub renderer on a synthetic sphere.

The lines that start with "meshtexture parity:" are the ones profiles/meshtexture_parity.txt records."""
import numpy as np
import pytest
import torch

from tests import meshray_restate as MR
from tests import meshtexture_cases as TC
from tests import meshtexture_restate as X

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.array(a, order="C")).to(_dev(), dtype)          # (a copy: the cases are read-only)


def _h(a):
    return torch.from_numpy(np.array(a, order="C"))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.int32)


def _same(tex, want):
    return (np.array_equal(tex[0].cpu().numpy(), want[0]) and np.array_equal(bits(tex[1].cpu().numpy()), bits(want[1]))
            and np.array_equal(tex[2].cpu().numpy(), want[2]))


_built = {}


def _visible(key):
    """(bvh, face, point, anchor, mask) of the case on the device, built once: the mask is `meshray.visibility` on the anchors."""
    if key not in _built:
        from lara_amd import meshbvh, meshray, meshtexture as MT
        c = TC.case(key)
        V, F = _t(c["V"]), _t(c["F"])
        face, point, anchor = MT.texels(c["layout"], V, F)
        bvh = mask = None
        if len(c["F"]) and len(c["eyes"]):
            bvh = meshbvh.TriangleBVH(V, F)
            mask = meshray.visibility(bvh, anchor.view(-1, 3), _t(c["eyes"]), faces=face.view(-1)).view(face.shape)
        _built[key] = (bvh, face, point, anchor, mask)
    return _built[key]


@pytest.mark.parametrize("key", TC.KEYS)
def test_texels_equal_the_host_twin_and_the_restatement(hip_lib, key):
    from lara_amd import meshtexture as MT
    c = TC.case(key)
    _, face, point, anchor, _ = _visible(key)
    want = X.texels(c["layout"], c["V"], c["F"])
    host = MT.texels(c["layout"], _h(c["V"]), _h(c["F"]), host=True)
    for got, w, h in zip((face, point, anchor), want, host):
        g = got.cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g.view(np.int32), w.view(np.int32)) and np.array_equal(g.view(np.int32), h.numpy().view(np.int32))
    again = MT.texels(c["layout"], _t(c["V"]), _t(c["F"]))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(again, (face, point, anchor)))


@pytest.mark.parametrize("key", TC.KEYS)
def test_bake_equals_the_host_twin_and_the_restatement(hip_lib, key):
    """Every variant; where a variant asks for a mask it is visibility's, read back for the host twin and the restatement.  The same
    bits on a second call and on a side stream."""
    from lara_amd import meshtexture as MT
    c = TC.case(key)
    L = c["layout"]
    bvh, face, point, anchor, vis = _visible(key)
    vis_host = None if vis is None else vis.cpu().numpy()
    V, F, I, k, w2c, eyes = (_t(c[n]) for n in ("V", "F", "images", "k", "w2c", "eyes"))
    texels_host = [x.cpu() for x in (face, point, anchor)]
    differ = 0
    for name, kw in TC.VARIANTS:
        a = TC.bake_arguments(c, kw, mask=vis_host)
        want = X.bake(L, c["V"], c["F"], c["images"], c["k"], c["w2c"], c["eyes"], **a)
        m, vc = a.pop("mask"), a.pop("vertex_colors")
        dev_kw = dict(a, vertex_colors=None if vc is None else _t(vc))
        got = MT.bake_texels(L, V, F, face, point, anchor, I, k, w2c, eyes, None if m is None else _t(m), **dev_kw)
        host = MT.bake_texels(L, _h(c["V"]), _h(c["F"]), *texels_host, _h(c["images"]), _h(c["k"]), _h(c["w2c"]), _h(c["eyes"]),
                              None if m is None else _h(m), **dict(a, vertex_colors=None if vc is None else _h(vc)), host=True)
        differ += int((got[0].cpu().numpy() != want[0]).sum()) + int((bits(got[1].cpu().numpy()) != bits(want[1])).sum())
        assert _same(got, want), (key, name)
        assert _same(got, [x.numpy() for x in host]), (key, name)
        again = MT.bake_texels(L, V, F, face, point, anchor, I, k, w2c, eyes, None if m is None else _t(m), **dev_kw)
        assert all(torch.equal(x, y) for x, y in zip(again[:1] + again[2:], got[:1] + got[2:])) and torch.equal(again[1].view(torch.int32), got[1].view(torch.int32))
    # the public entry with its own walk (a high-priority stream: see tests/test_meshtopo_gpu.py on the round of default-priority streams)
    main = MT.bake(V, F, I, _h(c["ixt"]), _h(c["c2w"]), patch=L[0], width=L[2], bvh=bvh, vertex_colors=_t(c["colours"]))
    side = torch.cuda.Stream(_dev(), priority=-1)
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        on_side = MT.bake(V, F, I, _h(c["ixt"]), _h(c["c2w"]), patch=L[0], width=L[2], vertex_colors=_t(c["colours"]))
    side.synchronize()
    assert main.layout == on_side.layout == L
    assert torch.equal(main.texture, on_side.texture) and torch.equal(main.view, on_side.view) and torch.equal(main.weight.view(torch.int32), on_side.weight.view(torch.int32))
    want = X.bake(L, c["V"], c["F"], c["images"], c["k"], c["w2c"], c["eyes"], mask=vis_host, vertex_colors=c["colours"])
    assert _same((main.texture, main.weight, main.view), want)
    assert (main.mask is None) == (vis is None) and (vis is None or torch.equal(main.mask, vis))
    print(f"meshtexture parity: device bake {key}: atlas {L[2]} x {L[3]}, {len(c['images'])} views, {len(TC.VARIANTS)} variants, "
          f"{differ} bytes or weight words differ from the restatement, coverage {main.coverage:.4f}")


@pytest.mark.parametrize("key", ["two_layer S3 C40", "odd S7 C4", "bad_triangles S4 C5"])
def test_the_mask_fed_to_the_bake_is_meshrays_restatement(hip_lib, key):
    """Bit e of an owned texel = no other triangle is hit from eye e before the anchor, by tests/meshray_restate.visibility (about
    400 texels, evenly taken, where the atlas is larger); a hit within the restatement's ambiguous band of the cut is exempt, as
    in tests/test_meshray_gpu.py.  Unowned texels (a NaN anchor) have 0."""
    c = TC.case(key)
    _, face, _, anchor, mask = _visible(key)
    f, a, m = face.view(-1).cpu().numpy(), anchor.view(-1, 3).cpu().numpy(), mask.view(-1).cpu().numpy()
    assert not m[f < 0].any()
    pick = np.nonzero(f >= 0)[0]
    pick = pick[::max(1, len(pick) // 400)]
    seen, amb = MR.visibility(a[pick], c["eyes"], c["V"], c["F"], skip=f[pick])
    E = len(c["eyes"])
    got = (m[pick, None] >> np.arange(E)[None]) & 1
    want = (seen[:, None] >> np.arange(E)[None]) & 1
    wrong = (got != want) & ~amb
    print(f"meshtexture parity: visibility {key}: {len(pick)} texels x {E} eyes, {int(amb.sum())} ambiguous, {int(wrong.sum())} differ")
    assert not wrong.any() and not (m[pick] >> E).any()


def test_no_view_sees_the_inner_layer(hip_lib):
    """The icosphere around a copy scaled by 0.5: every texel of the inner layer falls back (alpha 0, the vertex colours' blend), every
    outer texel some view accepts without the walk keeps alpha 255 with it; `occlusion=False` colours the inner layer."""
    from lara_amd import meshtexture as MT
    key = "two_layer S3 C40"
    c = TC.case(key)
    L = c["layout"]
    V, F, I = _t(c["V"]), _t(c["F"]), _t(c["images"])
    tex = MT.bake(V, F, I, _h(c["ixt"]), _h(c["c2w"]), patch=L[0], width=L[2], vertex_colors=_t(c["colours"]))
    free = MT.bake(V, F, I, _h(c["ixt"]), _h(c["c2w"]), patch=L[0], width=L[2], vertex_colors=_t(c["colours"]), occlusion=False)
    face, alpha, alpha_free = tex.face.cpu().numpy(), tex.texture[..., 3].cpu().numpy(), free.texture[..., 3].cpu().numpy()
    inner, outer = face >= len(c["F"]) // 2, (face >= 0) & (face < len(c["F"]) // 2)
    assert inner.sum() == outer.sum() > 0
    assert not alpha[inner].any()
    # the outer layer is convex and nothing lies outside it: a view that faces an outer texel sees it
    assert np.array_equal(alpha[outer], alpha_free[outer]) and (alpha[outer] == 255).mean() > 0.9
    assert (alpha_free[inner] == 255).mean() > 0.9
    want = X.bake(L, c["V"], c["F"], c["images"], c["k"], c["w2c"], c["eyes"], mask=np.zeros(face.shape, np.int64), vertex_colors=c["colours"])
    assert np.array_equal(tex.texture.cpu().numpy()[inner], want[0][inner])
    assert tex.coverage == float((alpha[face >= 0] == 255).mean()) and tex.coverage < 0.55 < free.coverage


@pytest.mark.parametrize("key", ["empty S4 C2", "odd S4 V0"])
def test_without_triangles_or_views_the_outputs_are_well_formed(hip_lib, key):
    from lara_amd import meshtexture as MT
    c = TC.case(key)
    L = c["layout"]
    tex = MT.bake(_t(c["V"]), _t(c["F"]), _t(c["images"]), _h(c["ixt"]), _h(c["c2w"]), patch=L[0], width=L[2], fill=(1.0, 0.5, 0.0))
    assert tex.layout == L and tuple(tex.texture.shape) == (L[3], L[2], 4) and tex.mask is None and tex.coverage == 0.0
    assert tuple(tex.uvs.shape) == (len(c["F"]), 3, 2)
    rgba = tex.texture.cpu().numpy()
    assert np.array_equal(np.unique(rgba.reshape(-1, 4), axis=0), np.array([[255, 128, 0, 0]], np.uint8))
    assert not tex.weight.any() and not tex.view.any()
    out = tex.sample(_t(np.array([-1, 0, 3], np.int32)), _t(np.full((3, 3), 1 / 3, F32)), alpha=True, background=(0.5, 0.25, 1.0))
    if len(c["F"]) == 0:
        assert np.array_equal(out.cpu().numpy(), np.broadcast_to(np.array([0.5, 0.25, 1.0, 0.0], F32), (3, 4)))


@pytest.mark.parametrize("key", ["icosphere S8", "uv_sphere S4 C50", "bad_triangles S4 C5", "odd S8 C1"])
def test_sample_equals_the_host_twin_and_the_restatement(hip_lib, key):
    from lara_amd import meshtexture as MT
    c = TC.case(key)
    L, T = c["layout"], len(c["F"])
    tex = TC.restated(key, "weighted masked colours")[0]
    g = np.random.default_rng(7)
    bary = np.concatenate([TC.dense_bary(12), (g.random((300, 3)) * 1.4 - 0.2).astype(F32), np.array([[np.nan, np.nan, 0.5], [0, 2, -1]], F32)])
    face = g.integers(-1, T + 2, len(bary)).astype(np.int32)
    for alpha in (False, True):
        want = X.sample(L, T, tex, face, bary, alpha, (0.1, 0.2, 0.3))
        got = MT.sample(L, T, _t(tex), _t(face), _t(bary), alpha, (0.1, 0.2, 0.3))
        host = MT.sample(L, T, _h(tex), _h(face), _h(bary), alpha, (0.1, 0.2, 0.3), host=True)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and np.array_equal(bits(host.numpy()), bits(want))
        assert torch.equal(MT.sample(L, T, _t(tex), _t(face), _t(bary), alpha, (0.1, 0.2, 0.3)).view(torch.int32), got.view(torch.int32))
    args = (_t(tex), _t(face), _t(bary))
    side = torch.cuda.Stream(_dev(), priority=-1)          # (high priority: see tests/test_meshtopo_gpu.py)
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        on_side = MT.sample(L, T, *args, True, (0.1, 0.2, 0.3))
    side.synchronize()
    assert torch.equal(on_side.view(torch.int32), got.view(torch.int32))


def test_render_textured_on_the_tooth(hip_lib):
    """tests/test_meshtexture.py's tooth through the kernels, the visibility walk and `render_textured`: the held-out view's pixels that
    hit the mesh, against the analytic colour of the hit points `raycast` reports; the cap is the issue's 0.25."""
    from lara_amd import meshbvh, meshray, meshtexture as MT
    t = TC.tooth()
    V, F = _t(t["V"]), _t(t["F"])
    bvh = meshbvh.TriangleBVH(V, F)
    tex = MT.bake(V, F, _t(t["images"]), _h(t["ixt"]), _h(t["c2w"]), patch=8, bvh=bvh)
    m = t["res"][1]
    frame = MT.render_textured(bvh, tex, _h(t["held_ixt"][None]), _h(t["held_c2w"][None]), m, m, background=(0, 0, 0))[0]
    o, d = meshray.pixel_rays(_h(t["held_ixt"][None]), _h(t["held_c2w"][None]), m, m, _dev())
    _, face, bary = meshray.raycast(bvh, o.view(-1, 3), d.view(-1, 3), return_bary=True)
    face, bary = face.cpu().numpy(), bary.cpu().numpy().astype(np.float64)
    hit = face >= 0
    tri = t["V"].astype(np.float64)[t["F"][face[hit]]]
    truth = TC.field((bary[hit, :, None] * tri).sum(1), TC.TOOTH_WAVE)
    vertex = TC.rmse((bary[hit, :, None] * TC.field(tri, TC.TOOTH_WAVE)).sum(1), truth)
    got = TC.rmse(frame.view(-1, 3).cpu().numpy()[hit], truth)
    host = MT.bake(_h(t["V"]), _h(t["F"]), _h(t["images"]), _h(t["ixt"]), _h(t["c2w"]), patch=8, occlusion=False, host=True)
    print(f"meshtexture parity: tooth on the device: {int(hit.sum())} pixels, vertex colours RMSE {vertex:.4f}, render_textured RMSE {got:.4f}, "
          f"ratio {got / vertex:.4f} (cap {TC.TOOTH_CAP}); coverage {tex.coverage:.4f}")
    assert got <= TC.TOOTH_CAP * vertex and not frame.view(-1, 3).cpu().numpy()[~hit].any()
    # the icosphere is convex: the walk hides nothing a facing view holds, and the device's atlas is the host's
    assert np.array_equal(tex.texture.cpu().numpy(), host.texture.numpy())


class _SphereRenderer:
    """A stand-in for the renderer `MeshExtractor` drives: the views of a sphere of radius 0.35 coloured by the analytic field, by
    ray-sphere intersection in torch (depth along the view axis, acc 1 on the sphere, a white background)."""
    RADIUS, WAVE = 0.35, 9.0

    def render_img(self, cam, rays, centers, shs, opacity, scaling, rotation, device):
        from lara_amd.mesh import _cam_c2w
        o, d = rays[..., :3].double(), rays[..., 3:6].double()
        a, b, c = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - self.RADIUS ** 2
        disc = b * b - a * c
        hit = disc > 0
        t = (-b - disc.clamp_min(0).sqrt()) / a
        p = o + t[..., None] * d
        forward = _cam_c2w(cam)[:3, 2].double().to(rays.device)
        depth = torch.where(hit, ((p - o) * forward).sum(-1), torch.zeros_like(t))
        phase = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=rays.device)
        image = torch.where(hit[..., None], 0.5 + 0.5 * torch.sin(self.WAVE * p + phase), torch.ones_like(p))
        return {"depth": depth.float(), "acc_map": hit.float(), "image": image.float()}


def test_extract_bakes_and_writes_a_textured_obj(hip_lib, tmp_path):
    """`texture_patch=6` after a 4-voxel simplification writes the .obj, the .mtl and the .png, they read back to the returned mesh
    and to `last_texture`, and the texture shows the sphere's colours; with the defaults the bytes are `write_obj`'s, as before."""
    from lara_amd import cameras, meshtexture as MT
    from lara_amd.mesh import MeshExtractor, write_obj
    c2w = torch.cat([cameras.turntable_c2w(8, e) for e in (0.0, -30.0, 30.0)])
    cams = cameras.make_cameras(c2w, 128, 128, 0.75, 0.75, 1.906 - 0.8, 1.906 + 0.8, device="cuda")
    one = torch.zeros(1, 3, device="cuda")
    params = (one, torch.zeros(1, 4, 3, device="cuda"), torch.zeros(1, 1, device="cuda"), one.clone(), torch.zeros(1, 4, device="cuda"),
              torch.ones(1, dtype=torch.bool, device="cuda"))
    ex = MeshExtractor(params, _SphereRenderer(), [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5])
    plain = str(tmp_path / "plain.obj")
    v0, t0, c0 = ex.extract(plain, None, cams=cams)
    assert ex.last_texture is None and t0.shape[0] > 1000
    write_obj(str(tmp_path / "by_hand.obj"), v0, t0, c0)
    assert (tmp_path / "plain.obj").read_bytes() == (tmp_path / "by_hand.obj").read_bytes()
    assert not (tmp_path / "plain.mtl").exists() and not (tmp_path / "plain.png").exists()
    ex.timings = []
    path = str(tmp_path / "textured.obj")
    v, t, c = ex.extract(path, None, cams=cams, simplify_voxel=4 * ex.last_grid[1], texture_patch=6)
    marks = [name for name, _ in ex.timings]
    assert marks[-3:] == ["simplify", "texture", "write_obj"] and 0 < t.shape[0] < t0.shape[0] / 4
    tex = ex.last_texture
    assert isinstance(tex, MT.Texture) and tex.layout == MT.atlas(t.shape[0], 6) and tex.n_triangles == t.shape[0]
    for ext in (".obj", ".mtl", ".png"):
        assert (tmp_path / ("textured" + ext)).exists()
    rv, rt, ruv, rgba = MT.read_textured_obj(path)
    assert rv.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(rt, t.cpu().numpy())
    assert np.array_equal(bits(ruv), bits(tex.uvs.numpy())) and np.array_equal(rgba, tex.texture.cpu().numpy())
    # every view-coloured texel shows the field at its surface point to within the extraction's own error of the surface (a few
    # voxels) times the field's slope (WAVE / 2 per unit length), the source pixel's footprint and the 8-bit steps
    face, point, _ = MT.texels(tex.layout, v, t)
    seen = (tex.texture[..., 3] == 255).cpu().numpy()
    assert 0.5 < tex.coverage == float(seen[face.cpu().numpy() >= 0].mean())
    p = point.cpu().numpy().astype(np.float64)[seen]
    want = TC.field(p * (_SphereRenderer.RADIUS / np.linalg.norm(p, axis=1, keepdims=True)), _SphereRenderer.WAVE)
    err = TC.rmse(rgba[seen][:, :3] / 255.0, want)
    vertex_err = TC.rmse(c.cpu().numpy(), TC.field(v.cpu().numpy().astype(np.float64), _SphereRenderer.WAVE))
    print(f"meshtexture parity: extractor: {t.shape[0]} triangles, atlas {tex.layout[2]} x {tex.layout[3]}, coverage {tex.coverage:.4f}, "
          f"texel RMSE against the field {err:.4f}, vertex colours' RMSE at the vertices {vertex_err:.4f}")
    # 0.1: the simplification moves the surface by at most its cell, 4 voxels = 0.015, which moves the field by at most 0.015 x WAVE / 2
    # = 0.067; the source pixel's footprint and the 8-bit steps add less than 0.01.  Colours unrelated to the field give 0.5.
    assert err < 0.1
    with pytest.raises(ValueError, match="needs a .obj path"):
        ex.extract(str(tmp_path / "textured.ply"), None, cams=cams, texture_patch=6)
