"""Tight tiles (`lara2dgs_view.prefiltered` bit 2, `tight_tiles=True`): a surfel is binned into the tiles its cull box meets
instead of its whole 3-sigma square.  The pairs that go are pairs the composite's staging drops anyway (the one tile test of
`csrc/tilebox.h`, restated as `tile_keep` in tests/test_tilebox_cpu.py), so

  1. the tight lists are the loose lists minus exactly those entries, in order; radii, records and cull boxes are the loose call's;
     no pair with a pixel of alpha >= 1/255 (evaluated here in fp64 from the records) is lost;
  2. the outputs are the loose call's up to what a shifted list position does -- the bars of
     test_raster_parity_gpu.py::test_opt_in_culling_of_transparent_surfels_changes_no_pixel, as they stand: colour <= 2.5e-7,
     maps <= 1e-6, at most 1 % of the pixels differ at all, every gradient within 1e-5 of its tensor's maximum;
  3. what the project promises bit for bit holds with the flag on: views against one-view calls, colour-only against zeros,
     a subset call against re-binning, two runs;
  4. `Renderer` / the pipeline: on and off agree within the bars, the environment variable sets the default.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests.helpers import raster_settings, small_scene
from tests.test_tilebox_cpu import tile_keep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COLOUR_BAR, MAPS_BAR, PIXELS_BAR, GRAD_BAR = 2.5e-7, 1e-6, 1e-2, 1e-5


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def _quat_from_R(R):
    w = math.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = math.copysign(math.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2])
    y = math.copysign(math.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0])
    z = math.copysign(math.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])
    return [w, x, y, z]


HAND = dict(crossing=0, below=1, above=2, border=3, diagonal=4)


def _hand_scene(S=64):
    """Seven hand-placed surfels in front of one 64 x 64 camera: the cases the synthetic scenes never produce."""
    from lara_amd import cameras
    cam = cameras.make_cameras(cameras.turntable_c2w(4), S, S, 0.75, 0.75, 0.5, 2.5)[0]
    c2w = np.linalg.inv(cam.world_view_transform.double().numpy().T)
    thr = np.float32(1.0 / 255.0)
    a = math.radians(45.0)
    rot45 = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.0]])
    along_view = np.array([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])       # the u axis along the viewing direction
    f = 0.5 * S / math.tan(0.375)

    def at(px, py, z=1.9):     # the view-space point that projects to pixel (px, py)
        return [(px - (S - 1) / 2) * z / f, (py - (S - 1) / 2) * z / f, z]
    rows = [  # view-space centre, view-space rotation, scales, opacity
        (at(30, 30, 1.2), along_view, (1.0, 0.05), 0.9),                                   # its disc crosses the camera's w = 0 plane
        # opacity just below 1/255 -- by 2e-4 of it: the list test below asks for every pair with alpha >= 1/255 (1 - 1e-4), and an
        # opacity inside that band has alpha <= opacity < 1/255 on every pixel (never blended, the empty box) yet a pixel the test counts
        (at(20, 40), np.eye(3), (0.15, 0.15), float(thr * np.float32(1.0 - 2e-4))),
        (at(40, 20), np.eye(3), (0.15, 0.15), float(np.nextafter(thr, np.float32(1)))),    # ... and just above
        (at(-3, 33), np.eye(3), (0.12, 0.12), 0.5),                                        # box straddles the left image border
        (at(31.5, 31.5), rot45, (0.45, 0.01), 0.8),                                        # elongated at 45 degrees
        (at(47.3, 48.9), np.eye(3), (0.05, 0.08), 0.3),                                    # two ordinary ones
        (at(10.2, 12.7), rot45, (0.1, 0.03), 0.05),
    ]
    means = [(c2w @ np.array(pv + [1.0]))[:3] for pv, _, _, _ in rows]
    quats = [_quat_from_R(c2w[:3, :3] @ Rv) for _, Rv, _, _ in rows]
    g = torch.Generator().manual_seed(4)
    act = dict(means3D=torch.tensor(np.array(means), dtype=torch.float32), shs=torch.randn(len(rows), 4, 3, generator=g) * 0.5,
               opacities=torch.tensor([[o] for _, _, _, o in rows], dtype=torch.float32),
               scales=torch.tensor([sc for _, _, sc, _ in rows], dtype=torch.float32),
               rotations=torch.tensor(quats, dtype=torch.float32))
    return act, cam


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "init":
        act, cams = small_scene(grid=12, size=96, seed=3)
        return act, cams[1], (1.0, 1.0, 1.0)
    if name == "trained":
        act, cams = small_scene(grid=16, size=128, seed=3, regime="trained")
        return act, cams[1], (0.0, 0.5, 1.0)
    act, cam = _hand_scene()
    return act, cam, (0.2, 0.5, 1.0)


SCENES = ("init", "trained", "hand")


@functools.lru_cache(maxsize=None)
def _states(name):
    """The state of the loose and of the tight forward of a scene, as numpy (computed once per scene)."""
    from lara_amd import rasterizer
    act, cam, bg = _scene(name)
    rs = raster_settings(cam, bg, device=DEV)
    t = {k: v.to(DEV) for k, v in act.items()}
    out = {}
    for tight in (False, True):
        r = rasterizer.forward_with_state(rs, t["means3D"], t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                                          tight_tiles=tight)
        torch.cuda.synchronize()
        v = r["views"]
        hdr = v["header"].cpu().numpy().view(np.uint32)
        assert hdr[1] == 0, "unexpected capacity overflow"
        D = int(hdr[0])
        out[tight] = dict(D=D, ranges=v["ranges"].cpu().numpy().view(np.uint32).astype(np.int64), cullbox=v["cullbox"].cpu().numpy(),
                          point_list=v["point_list"][:D].cpu().numpy().view(np.uint32).astype(np.int64), geom=v["geom"].cpu().numpy(),
                          radii=r["radii"].cpu().numpy(), color=r["color"].cpu().numpy(), allmap=r["allmap"].cpu().numpy())
    return out


def _in_tile_order(st):
    """(surfel id, tile) of every list entry, tile by tile."""
    lens = st["ranges"][:, 1] - st["ranges"][:, 0]
    tiles = np.repeat(np.arange(len(lens)), lens)
    pos = np.concatenate([np.arange(s, e) for s, e in st["ranges"]]) if len(lens) else np.zeros(0, np.int64)
    return st["point_list"][pos.astype(np.int64)], tiles, lens


def _live(geom, ids, tiles, gx, W, H, chunk=4096):
    """Per (surfel, tile) pair: does a pixel of the tile reach alpha >= 1/255 (1 - 1e-4)?  fp64, rho = min(rho3d, rho2d) as in
    oracle/surfel_oracle.c, from the records the forward wrote."""
    thr = (1.0 / 255.0) * (1.0 - 1e-4)
    out = np.zeros(len(ids), bool)
    lx = np.arange(16, dtype=np.float64)
    for c0 in range(0, len(ids), chunk):
        g = geom[ids[c0:c0 + chunk]].astype(np.float64)
        tl = tiles[c0:c0 + chunk]
        Tu, Tv, Tw = (g[:, None, None, 3 * k:3 * k + 3] for k in range(3))
        px = ((tl % gx) * 16)[:, None, None] + lx[None, None, :]
        py = ((tl // gx) * 16)[:, None, None] + lx[None, :, None]
        p = np.cross(px[..., None] * Tw - Tu, py[..., None] * Tw - Tv)
        ok = p[..., 2] != 0
        pz = np.where(ok, p[..., 2], 1.0)
        rho3d = (p[..., 0] / pz) ** 2 + (p[..., 1] / pz) ** 2
        rho2d = 2.0 * ((g[:, None, None, 9] - px) ** 2 + (g[:, None, None, 10] - py) ** 2)
        alpha = np.minimum(0.99, g[:, None, None, 11] * np.exp(-0.5 * np.minimum(rho3d, rho2d)))
        out[c0:c0 + chunk] = (ok & (px < W) & (py < H) & (alpha >= thr)).any((1, 2))
    return out


# ---- 1. lists --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_tight_lists_are_the_loose_lists_minus_the_entries_whose_box_misses_the_tile(hip_lib, name):
    act, cam, _ = _scene(name)
    H, W = int(cam.image_height), int(cam.image_width)
    gx = (W + 15) // 16
    st = _states(name)
    lo, ti = st[False], st[True]
    vis = lo["radii"] > 0
    assert np.array_equal(lo["radii"], ti["radii"]) and vis.any()
    assert np.array_equal(lo["geom"][vis].view(np.uint32), ti["geom"][vis].view(np.uint32))
    assert np.array_equal(lo["cullbox"][vis].view(np.uint32), ti["cullbox"][vis].view(np.uint32))
    ids, tiles, _ = _in_tile_order(lo)
    assert len(ids) == lo["D"] and vis[ids].all()
    keep = tile_keep(lo["cullbox"][ids], tiles % gx, tiles // gx)
    ids_t, tiles_t, lens_t = _in_tile_order(ti)
    # every tile: the loose list without the entries whose cull box fails the tile test, in the same order
    assert np.array_equal(lens_t, np.bincount(tiles[keep], minlength=len(lens_t)))
    assert np.array_equal(ids_t, ids[keep]) and np.array_equal(tiles_t, tiles[keep])
    # ranges and D are consistent with it: lists back to back in tile order, (0, 0) where empty
    starts = np.cumsum(lens_t) - lens_t
    assert np.array_equal(ti["ranges"][lens_t > 0, 0], starts[lens_t > 0]) and not ti["ranges"][lens_t == 0].any()
    assert ti["D"] == int(keep.sum()) == int(lens_t.sum())
    assert ti["D"] < lo["D"], (ti["D"], lo["D"])
    # no pair that can blend a pixel went
    live = _live(lo["geom"], ids, tiles, gx, W, H)
    print(f"{name}: D {lo['D']} -> {ti['D']} ({ti['D'] / lo['D']:.3f}); pairs with a pixel of alpha >= 1/255: {int(live.sum())} "
          f"({live.mean():.3f} of D), of them outside the box: {int((live & ~keep).sum())}")
    assert live.any() and not (live & ~keep).any()


def test_hand_placed_surfels_hit_the_special_boxes(hip_lib):
    st = _states("hand")
    lo, ti = st[False], st[True]
    cb = lo["cullbox"]
    inf = np.inf
    n_lo, n_ti = np.bincount(lo["point_list"], minlength=len(cb)), np.bincount(ti["point_list"], minlength=len(cb))
    assert (lo["radii"] > 0).all() and (n_lo > 0).all()
    # the disc that crosses the w = 0 plane: unbounded box, its 3-sigma rectangle unchanged
    i = HAND["crossing"]
    assert np.array_equal(cb[i], np.array([-inf, inf, -inf, inf], np.float32)) and n_ti[i] == n_lo[i]
    # opacity just below 1/255: the empty box, no tile, radius kept; just above: a box, at least its own tile
    i = HAND["below"]
    assert np.array_equal(cb[i], np.array([inf, -inf, inf, -inf], np.float32)) and n_ti[i] == 0 and ti["radii"][i] == lo["radii"][i] > 0
    i = HAND["above"]
    assert np.isfinite(cb[i]).all() and 1 <= n_ti[i] < n_lo[i]
    # the box over the image border keeps the border tiles it reaches; the 45-degree one keeps every tile of its box
    i = HAND["border"]
    assert cb[i, 0] < 0 < cb[i, 1] and n_ti[i] >= 1
    i = HAND["diagonal"]
    assert np.isfinite(cb[i]).all() and n_ti[i] >= 4


# ---- 2. outputs ------------------------------------------------------------------------------------------------------------
def _run(name, tight, maps_grad="randn"):
    from lara_amd import rasterize_gaussians
    act, cam, bg = _scene(name)
    rs = raster_settings(cam, bg, device=DEV)
    inp = {k: v.to(DEV).clone().requires_grad_(True) for k, v in act.items()}
    m2 = torch.zeros_like(inp["means3D"], requires_grad=True)
    color, radii, allmap = rasterize_gaussians(inp["means3D"], m2, inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"],
                                               None, rs, tight_tiles=tight)
    g = torch.Generator().manual_seed(2)
    dc, da = torch.randn(color.shape, generator=g).to(DEV), (torch.randn(allmap.shape, generator=g) * 0.1).to(DEV)
    loss = (color * dc).sum()
    if maps_grad == "randn":
        loss = loss + (allmap * da).sum()
    elif maps_grad == "zeros":
        loss = loss + (allmap * torch.zeros_like(allmap)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.clone() for k, v in inp.items()}
    grads["means2D"] = m2.grad.clone()
    return color.detach(), allmap.detach(), radii, grads


def _within_the_bars(c0, a0, c1, a1, what):
    dc, da = float((c0 - c1).abs().max()), float((a0 - a1).abs().max())
    moved = float(((c0 != c1).any(-3) | (a0 != a1).any(-3)).float().mean())
    print(f"{what}: colour max diff {dc:.3e}, maps max diff {da:.3e}, pixels that differ {moved:.2e}")
    assert dc <= COLOUR_BAR and da <= MAPS_BAR, (what, dc, da)
    assert moved <= PIXELS_BAR, (what, moved)


@pytest.mark.parametrize("name", SCENES)
def test_tight_outputs_and_gradients_are_the_loose_ones_within_the_bars(hip_lib, name):
    c0, a0, r0, g0 = _run(name, False)
    c1, a1, r1, g1 = _run(name, True)
    assert torch.equal(r0, r1)
    _within_the_bars(c0, a0, c1, a1, name)
    owns_none = torch.from_numpy(np.bincount(_states(name)[True]["point_list"], minlength=r0.numel()) == 0).to(DEV)
    for k in g0:
        err = float((g0[k] - g1[k]).abs().max()) / (float(g0[k].abs().max()) + 1e-30)
        print(f"{name}: grad {k}: max diff / max {err:.3e}")
        assert float((g0[k] - g1[k]).abs().max()) <= GRAD_BAR * float(g0[k].abs().max()) + 1e-12, (k, err)
        assert torch.isfinite(g1[k]).all() and not g1[k][owns_none].any(), k
    if name == "hand":
        assert bool(owns_none[HAND["below"]]) and bool((r1 > 0)[HAND["below"]])


@pytest.mark.parametrize("name", SCENES)
def test_the_oracles_gradient_check_holds_with_tight_tiles(hip_lib, name, monkeypatch):
    from lara_amd import rasterizer
    from tests.test_raster_parity_gpu import _grad_check
    act, cam, bg = _scene(name)
    monkeypatch.setattr(rasterizer, "rasterize_gaussians", functools.partial(rasterizer.rasterize_gaussians, tight_tiles=True))
    _grad_check(act, cam, bg)


# ---- 3. the same bits where the project promises them, with the flag on ------------------------------------------------------
def _leafs(act):
    return {k: v.to(DEV).clone().requires_grad_(True) for k, v in act.items()}


def test_five_views_in_one_call_are_five_one_view_calls_bit_for_bit(hip_lib):
    from lara_amd import rasterize_gaussians, rasterize_gaussians_views
    S, n = 96, 5
    act, cams = small_scene(grid=12, size=S, n_views=n, seed=3)
    settings = [raster_settings(c, bg, device=DEV) for c, bg in zip(cams, ((1, 1, 1), (0, 0, 0), (.5, .5, .5), (1, 1, 1), (0, 0, 0)))]
    g = torch.Generator().manual_seed(5)
    dcs, das = torch.randn(n, 3, S, S, generator=g).to(DEV), (torch.randn(n, 7, S, S, generator=g) * 0.1).to(DEV)
    outs, per_view = [], []
    for i, rs in enumerate(settings):
        t = _leafs(act)
        m2 = torch.zeros_like(t["means3D"], requires_grad=True)
        c, r, a = rasterize_gaussians(t["means3D"], m2, t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, rs,
                                      tight_tiles=True)
        torch.autograd.backward([c, a], [dcs[i], das[i]])
        outs.append((c.detach(), r, a.detach()))
        per_view.append({k: v.grad for k, v in t.items()} | {"means2D": m2.grad})
    t = _leafs(act)
    m2 = torch.zeros_like(t["means3D"], requires_grad=True)
    color, radii, allmap = rasterize_gaussians_views(settings, t["means3D"], m2, t["opacities"], shs=t["shs"], scales=t["scales"],
                                                     rotations=t["rotations"], tight_tiles=True)
    torch.autograd.backward([color, allmap], [dcs, das])
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(color[i].detach(), outs[i][0]) and torch.equal(radii[i], outs[i][1]) and torch.equal(allmap[i].detach(), outs[i][2]), i
    got = {k: v.grad for k, v in t.items()} | {"means2D": m2.grad}
    for k in got:
        want = per_view[0][k].clone()
        for pv in per_view[1:]:
            want = want + pv[k]            # view order, as the library folds the views
        assert torch.equal(got[k], want), k


@pytest.mark.parametrize("name", SCENES)
def test_colour_only_backward_is_the_full_one_fed_zeros_and_two_runs_agree(hip_lib, name):
    full, only, again = _run(name, True, "zeros"), _run(name, True, "none"), _run(name, True, "none")
    for k in full[3]:
        assert torch.equal(full[3][k], only[3][k]), k
        assert torch.equal(only[3][k], again[3][k]), k
    assert torch.equal(only[0], again[0]) and torch.equal(only[1], again[1]) and torch.equal(only[2], again[2])
    a, b = _run(name, True), _run(name, True)
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_subset_call_equals_rebinning_and_needs_the_coarse_calls_flags(hip_lib):
    from lara_amd import rasterize_gaussians_views
    S, n = 96, 4
    act, cams = small_scene(grid=20, size=S, seed=11)
    settings = [raster_settings(c, bg, device=DEV) for c, bg in zip(cams[:n], ((1, 1, 1), (0, 0, 0), (.5, .5, .5), (1, 1, 1)))]
    P = act["means3D"].shape[0]
    g = torch.Generator().manual_seed(3)
    idx = (torch.rand(P, generator=g) < 0.5).nonzero().squeeze(-1).to(DEV)
    dc, da = torch.randn(n, 3, S, S, generator=g).to(DEV), (0.1 * torch.randn(n, 7, S, S, generator=g)).to(DEV)
    coarse = {}
    for tight in (True, False):
        t = _leafs(act)
        coarse[tight] = (rasterize_gaussians_views(settings, t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"],
                                                   rotations=t["rotations"], tight_tiles=tight)[0], t)

    def fine(subset_of, tight=True):
        t = {k: v.detach()[idx].clone().requires_grad_(True) for k, v in coarse[True][1].items()}
        with torch.no_grad():
            t["shs"].add_(0.05)
        color, radii, allmap = rasterize_gaussians_views(settings, t["means3D"], None, t["opacities"], shs=t["shs"], scales=t["scales"],
                                                         rotations=t["rotations"], subset_of=subset_of, tight_tiles=tight)
        D = color.grad_fn.D
        torch.autograd.backward([color, allmap], [dc, da])
        return color.detach(), radii, allmap.detach(), {k: v.grad for k, v in t.items()}, D

    full, filt = fine(None), fine((coarse[True][0], idx))
    assert full[4] == filt[4] > 0
    for a, b in zip(full[:3], filt[:3]):
        assert torch.equal(a, b)
    for k in full[3]:
        assert torch.equal(full[3][k], filt[3][k]), k
    assert fine(None, tight=False)[4] > full[4]      # (the lists that were filtered were the tight ones)
    # a coarse call binned under the other rule: refused, either way round
    with pytest.raises(RuntimeError, match="other flags"):
        fine((coarse[False][0], idx), tight=True)
    with pytest.raises(RuntimeError, match="other flags"):
        fine((coarse[True][0], idx), tight=False)


# ---- 4. Renderer / pipeline --------------------------------------------------------------------------------------------------
def test_renderer_on_and_off_agree_and_the_environment_sets_the_default(hip_lib, monkeypatch):
    from lara_amd import cameras, synthetic
    from lara_amd.renderer import MAP_KEYS, Renderer
    monkeypatch.delenv("LARA2DGS_TIGHT_TILES", raising=False)
    assert Renderer(sh_degree=1).tight_tiles is True
    monkeypatch.setenv("LARA2DGS_TIGHT_TILES", "0")
    assert Renderer(sh_degree=1).tight_tiles is False and Renderer(sh_degree=1, tight_tiles=True).tight_tiles is True
    monkeypatch.setenv("LARA2DGS_TIGHT_TILES", "1")
    assert Renderer(sh_degree=1).tight_tiles is True and Renderer(sh_degree=1, tight_tiles=False).tight_tiles is False
    S, n = 96, 4
    sc = {k: v.to(DEV) for k, v in synthetic.make_scene(grid=12, K=2, regime="init", seed=2).items()}
    cams = cameras.make_cameras(cameras.turntable_c2w(n), S, S, 0.75, 0.75, 0.5, 2.5, device=DEV)
    g = torch.Generator().manual_seed(9)
    rays = [torch.nn.functional.normalize(torch.randn(S, S, 6, generator=g), dim=-1).to(DEV) for _ in cams]
    res, Ds = {}, {}
    for tight in (False, True):
        raster_out = []
        with torch.no_grad():
            res[tight] = Renderer(sh_degree=1, white_background=True, tight_tiles=tight).render_views(
                cams, rays, sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"], DEV, raster_out=raster_out)
        res[tight + 2] = raster_out[0]
    # the rasteriser's own outputs, then the six maps derived from them: the image under the colour bar, the others under the maps'
    _within_the_bars(res[2][0], res[2][2], res[3][0], res[3][2], "render_views (rasteriser)")
    for i, (f0, f1) in enumerate(zip(res[False], res[True])):
        assert set(f0) == set(MAP_KEYS)
        for k in MAP_KEYS:
            d = float((f0[k] - f1[k]).abs().max())
            moved = float((f0[k] != f1[k]).reshape(S * S, -1).any(-1).float().mean())
            print(f"render_views view {i} {k}: max diff {d:.3e}, pixels that differ {moved:.2e}")
            assert d <= (COLOUR_BAR if k == "image" else MAPS_BAR), (k, d)
            assert moved <= PIXELS_BAR, (k, moved)


def test_one_training_step_of_the_pipeline_with_the_flag_on_and_off(hip_lib):
    from lara_amd.pipeline import lara_loss
    from tests.test_pipeline import _small_problem
    dev = torch.device(DEV)
    runs = {}
    for tight in (False, True):
        pipe, batch, feat_vol = _small_problem(dev)
        pipe.fine_mask = "plain"
        pipe.gs_render.tight_tiles = tight
        out = pipe(batch, feat_vol, with_fine=True)
        loss, _ = lara_loss(batch, out, 2000, ms_ssim=False)
        loss.backward()
        pipe.join_streams()
        torch.cuda.synchronize()
        runs[tight] = (float(loss.detach()), {n: p.grad.clone() for n, p in pipe.named_parameters() if p.grad is not None}, feat_vol.grad.clone())
    (l0, g0, f0), (l1, g1, f1) = runs[False], runs[True]
    print(f"pipeline loss loose {l0!r} tight {l1!r}")
    assert abs(l0 - l1) <= 1e-6 * abs(l0)
    assert set(g0) == set(g1) and g0

    def close(a, b, n):     # the bars of tests/test_pipeline.py::test_pipeline_equals_the_operators_called_one_by_one
        fp32_path = n.startswith(("decoder.norm", "decoder.cross_att", "decoder.mlp_fine"))
        assert float((a - b).abs().max()) <= (2e-4 if fp32_path else 1e-2) * float(b.abs().max()) + 1e-12, n
        cos = float((a.double() * b.double()).sum() / (a.double().norm() * b.double().norm() + 1e-300))
        assert cos >= 1 - 1e-5, (n, cos)
    for n in g0:
        close(g1[n], g0[n], n)
    close(f1, f0, "feat_vol")
