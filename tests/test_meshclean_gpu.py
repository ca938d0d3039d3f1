"""lara_amd.mesh on the device against the restatement tests/meshclean_restate.py (Open3D's semantics [RECALLED]):
clean_mesh on hand-built, random, fused and full-size meshes, MeshExtractor against the same steps composed by hand, and
LaRaPipeline(return_buffer=True) feeding it."""
import numpy as np
import pytest
import torch

from tests import meshclean_restate as R
from tests.test_meshclean import _strip_clusters, random_mesh

AABB = [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]


@pytest.fixture(autouse=True)
def _release_cached_blocks():
    """These tests allocate up to ~1 GB (grids, edge tables): hand the caching allocator's blocks back after each one, so
    that the tests after them start from the allocator state they would see without these."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _hip(v, t, c=None, aabb=None, keep=10):
    from lara_amd.mesh import clean_mesh
    out = clean_mesh(torch.as_tensor(v).cuda(), torch.as_tensor(np.asarray(t, np.int64).reshape(-1, 3)).cuda(),
                     None if c is None else torch.as_tensor(c).cuda(), aabb=aabb, keep=keep)
    torch.cuda.synchronize()
    return out


def _same(v, t, c=None, aabb=None, keep=10, clusters=R.cluster_bfs):
    hv, ht, hc, info = _hip(v, t, c, aabb, keep)
    rv, rt, rc, rinfo = R.clean_mesh(v, t, c, aabb, keep, clusters=clusters)
    np.testing.assert_array_equal(info["triangle_clusters"].cpu().numpy(), rinfo["triangle_clusters"])
    np.testing.assert_array_equal(info["cluster_n_triangles"].cpu().numpy(), rinfo["cluster_n_triangles"])
    np.testing.assert_allclose(info["cluster_area"].cpu().numpy(), rinfo["cluster_area"], rtol=1e-9, atol=0)
    assert hv.dtype == torch.float32 and ht.dtype == torch.int64
    np.testing.assert_array_equal(hv.cpu().numpy(), rv)
    np.testing.assert_array_equal(ht.cpu().numpy(), rt)
    if c is not None:
        np.testing.assert_array_equal(hc.cpu().numpy(), rc)
    return hv, ht, hc, info


@pytest.mark.gpu
def test_hand_built_cases(hip_lib):
    rng = np.random.default_rng(0)
    v = rng.random((40, 3)).astype(np.float32)
    c = rng.random((40, 3)).astype(np.float32)
    for tris in ([[0, 1, 2], [2, 1, 3]], [[0, 1, 2], [2, 3, 4]], [[0, 1, 2], [1, 0, 3], [4, 5, 6], [0, 1, 7]],
                 [[6, 7, 8], [0, 1, 2], [7, 8, 9], [3, 4, 5], [1, 2, 10]]):
        _same(v, tris, c)
    tris, nv = _strip_clusters([12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 3, 2])
    _, ht, _, info = _same(rng.random((nv, 3)).astype(np.float32), tris)
    assert info["cluster_n_triangles"].numel() == 12 and ht.shape[0] == sum([12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 3])
    tris, nv = _strip_clusters([5, 1, 3, 2])
    _same(rng.random((nv, 3)).astype(np.float32), tris)
    out = np.nextafter(np.float32(5.5), np.float32(6))
    vb = np.array([[0, 0, 0], [5.5, 0, 0], [0, -5.5, 0], [0, 0, out], [-5.5, 5.5, 5.5]], np.float32)
    _, ht, _, _ = _same(vb, [[0, 1, 2], [0, 1, 3], [1, 2, 4]], aabb=[-5.0] * 3 + [5.0] * 3)
    assert ht.shape[0] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_random_meshes_match_and_are_bitwise_reproducible(hip_lib, seed):
    v, t = random_mesh(100_000, seed, nv=120_000)
    c = np.random.default_rng(seed).random(v.shape).astype(np.float32)
    a = _same(v, t, c, clusters=R.cluster_scipy)
    assert a[3]["cluster_n_triangles"].numel() > 1000
    b = _hip(v, t, c)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for k in ("triangle_clusters", "cluster_n_triangles", "cluster_area"):
        assert torch.equal(a[3][k], b[3][k]), k
    # a dense mesh: few large clusters, long union chains
    v, t = random_mesh(100_000, seed + 7, nv=30_000)
    _same(v, t, clusters=R.cluster_scipy, aabb=[-0.4] * 3 + [0.4] * 3)


@pytest.mark.gpu
def test_fused_spheres_with_a_tie_and_a_cut(hip_lib):
    """Marching cubes of fused analytic spheres (tests/test_tsdf.py:_sphere_views per sphere, one volume): 12 spheres,
    two of the same radius at the keep threshold (a tie), the box cutting through one of them."""
    from lara_amd.tsdf import TSDFVolume
    from tests.test_tsdf import _sphere_views
    radii = [0.22, 0.21, 0.2, 0.19, 0.18, 0.17, 0.16, 0.15, 0.14, 0.12, 0.12, 0.1]
    verts, tris, cols = [], [], []
    base = 0
    for i, r in enumerate(radii):          # separate volumes per sphere, shifted (a union of disjoint meshes)
        vol = TSDFVolume((-0.5, -0.5, -0.5), 1.0 / 48, 3.0 / 48, 48)
        depth, color, K, E = _sphere_views(16, 64, 64, radius=r, poles=True)
        vol.integrate(depth, color, K, E, 10.0)
        v, t, c = vol.extract_triangle_mesh()
        shift = torch.tensor([(i % 4) * 0.5 - 0.75, (i // 4) * 0.5 - 0.5, 0.0], device="cuda")
        verts.append(v + shift); tris.append(t + base); cols.append(c); base += v.shape[0]
    v = torch.cat(verts).cpu().numpy(); t = torch.cat(tris).cpu().numpy(); c = torch.cat(cols).cpu().numpy()
    perm = np.random.default_rng(3).permutation(len(t))
    t = t[perm]
    counts = R.cluster_scipy(v, t)[1]
    assert len(counts) >= 12 and np.sort(counts)[-10] == np.sort(counts)[-11], np.sort(counts)     # the tie
    _, _, _, info = _same(v, t, c, clusters=R.cluster_scipy)
    aabb = [-0.8, -0.7, -0.6, 0.5, 0.7, 0.6]          # x 1.1: cuts the spheres of the first and last columns
    _same(v, t, c, aabb=aabb, clusters=R.cluster_scipy)


@pytest.mark.gpu
def test_full_size_mesh_eval_object(hip_lib):
    from tools.mesh_bench import mesh_eval_mesh
    v, t, c = mesh_eval_mesh()
    assert t.shape[0] > 400_000
    v, t, c = v.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy()
    _same(v, t, c, clusters=R.cluster_scipy)
    _same(v, t, c, aabb=[-0.3] * 3 + [0.3] * 3, clusters=R.cluster_scipy)


@pytest.mark.gpu
def test_empty_and_fully_cropped(hip_lib):
    v = np.random.default_rng(0).random((5, 3)).astype(np.float32)
    for tris, aabb in ((np.zeros((0, 3), np.int64), None), (np.zeros((0, 3), np.int64), AABB), ([[0, 1, 2], [2, 3, 4]], [2.0] * 3 + [3.0] * 3)):
        hv, ht, hc, info = _hip(v, tris, v, aabb)
        assert hv.shape == (0, 3) and ht.shape == (0, 3) and hc.shape == (0, 3) and info["cluster_n_triangles"].numel() == 0


# ---- MeshExtractor ----------------------------------------------------------------------------------------------------------
def _turntable(res=256):
    from lara_amd import cameras
    c2w = torch.cat([cameras.turntable_c2w(16, e) for e in (0.0, -30.0, 30.0)])
    return cameras.make_cameras(c2w, res, res, 0.75, 0.75, 1.906 - 0.8, 1.906 + 0.8, device="cuda")


def _scene_params(seed=123, grid=32):
    from lara_amd import synthetic
    sc = synthetic.make_scene(grid=grid, K=2, regime="trained", seed=seed, device="cuda")
    mask = torch.sigmoid(sc["opacity"][:, 0]) > 0.005
    return (sc["centers"][mask], sc["shs"][mask], sc["opacity"], sc["scales"], sc["rotations"], mask)


def _by_hand(params, render, cams, aabb, voxel_size=2 / 256, sdf_trunc=0.08, origin_res=None):
    """meshExtractor.py:51-135 composed from the library's pieces one view at a time (render_img + integrate_render)."""
    from lara_amd.batch import build_rays, fov_to_ixt
    from lara_amd.mesh import _cam_c2w, clean_mesh
    from lara_amd.tsdf import TSDFVolume
    centers, shs, opacity, scaling, rotation, mask = params
    origin, vs, res = origin_res
    box = None if aabb is None else np.array(aabb, np.float64).reshape(2, 3) * 1.1
    if box is not None:
        center, radius = box.mean(0), np.linalg.norm(box[1] - box[0]) * 0.5
        sdf_trunc = 2 * vs
    vol = TSDFVolume(origin, vs, sdf_trunc, res)
    for cam in cams:
        ixt = fov_to_ixt(torch.tensor((cam.FoVx, cam.FoVy)), (cam.image_width, cam.image_height))
        rays = build_rays(_cam_c2w(cam)[None].cuda(), ixt[None].cuda(), cam.image_height, cam.image_width)[0]
        pkg = render.render_img(cam, rays, centers, shs, opacity[mask], scaling[mask], rotation[mask], "cuda")
        dt = 10.0 if box is None else float(np.linalg.norm(cam.camera_center.cpu().numpy() - center) + radius)
        vol.integrate_render(cam, pkg, alpha_thres=0.08, depth_trunc=dt)
    v, t, c = vol.extract_triangle_mesh()
    return clean_mesh(v, t, c, aabb=aabb)


@pytest.mark.gpu
@pytest.mark.parametrize("aabb", [None, AABB])
def test_mesh_extractor_equals_the_steps_composed_by_hand(hip_lib, tmp_path, aabb):
    from lara_amd.mesh import MeshExtractor, read_obj
    from lara_amd.renderer import Renderer
    params, cams = _scene_params(), _turntable()
    render = Renderer(sh_degree=1, white_background=True)
    ex = MeshExtractor(params, render, aabb)
    path = str(tmp_path / "mesh.obj")
    v, t, c = ex.extract(path, None, cams=cams)
    torch.cuda.synchronize()
    assert t.shape[0] > 5000 and ex.last_grid[2] % 16 == 0
    hv, ht, hc, _ = _by_hand(params, render, cams, aabb, origin_res=ex.last_grid)
    assert torch.equal(t, ht) and torch.equal(v, hv) and torch.equal(c, hc)
    rv, rt, rc = read_obj(path)
    assert rv.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(rt, t.cpu().numpy()) and rc.tobytes() == c.cpu().numpy().tobytes()
    if aabb is None:           # a grid one 16-voxel block larger on every side: the same mesh (the extent bound holds)
        big = MeshExtractor(params, render, aabb)
        big.grid_pad_blocks = 1
        bv, bt, bc = big.extract(str(tmp_path / "big.obj"), None, cams=cams)
        assert big.last_grid[2] == ex.last_grid[2] + 32
        assert torch.equal(bt, t)
        assert (bv - v).abs().max() <= 1e-6 and (bc - c).abs().max() <= 1e-6
    else:
        box = np.array(aabb).reshape(2, 3) * 1.1
        vn = v.cpu().numpy()
        assert (vn >= box[0]).all() and (vn <= box[1]).all()


@pytest.mark.gpu
def test_return_buffer_feeds_the_mesh_extractor(hip_lib, tmp_path):
    from lara_amd.mesh import MeshExtractor
    from tests.test_pipeline import _small_problem
    dev = torch.device("cuda:0")
    pipe, batch, feat_vol = _small_problem(dev)
    pipe.eval()
    pipe.n_streams = 1          # (creates no HIP streams: the later stream-safety tests see the process as before)
    with torch.no_grad():
        a = pipe(batch, feat_vol, with_fine=True)
        b = pipe(batch, feat_vol, with_fine=True, return_buffer=True)
        g = pipe.gaussians(feat_vol)
    assert set(b) == set(a) | {"render_pkg"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    pkg = b["render_pkg"]
    B = feat_vol.shape[0]
    assert len(pkg) == 2 * B
    seen = []
    orig = pipe.gs_render.render_views

    def spy(cams, rays, centers, shs, *args, **kw):
        seen.append((centers, shs))
        return orig(cams, rays, centers, shs, *args, **kw)
    pipe.gs_render.render_views = spy
    with torch.no_grad():
        c = pipe(batch, feat_vol, with_fine=True, return_buffer=True)
    pipe.gs_render.render_views = orig
    for i in range(B):
        co, fi = c["render_pkg"][2 * i], c["render_pkg"][2 * i + 1]
        assert len(co) == 5 and len(fi) == 6
        assert torch.equal(co[0], g["centers"][i]) and torch.equal(co[2], g["opacity"][i])
        mask = fi[5]
        assert mask.dtype == torch.bool and 0 < int(mask.sum()) < mask.numel()
        assert torch.equal(fi[0], co[0][mask]) and torch.equal(fi[2], co[2]) and torch.equal(fi[3], co[3])
        fine_calls = [s for s in seen if s[0].shape[0] == int(mask.sum())]
        assert any(s[1] is fi[1] for s in fine_calls)           # the shs the fine pass rendered, not a copy
    with torch.no_grad():
        a_c = pipe(batch, feat_vol, with_fine=False, return_buffer=True)
    assert len(a_c["render_pkg"]) == B and all(len(p) == 5 for p in a_c["render_pkg"])
    path = tmp_path / "scene0.obj"
    ex = MeshExtractor(b["render_pkg"][1], pipe.gs_render, AABB)
    v, t, col = ex.extract(str(path), None, cams=_turntable(64), chunk=8)
    assert path.exists() and t.shape[1] == 3 and v.shape == col.shape
