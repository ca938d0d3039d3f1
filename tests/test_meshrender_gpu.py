"""csrc/meshrender.hip held to the float64 / integer restatement of its header (tests/meshrender_restate.py) on the cases of
tests/meshrender_cases.py: stage V against float64, then visibility, depth, normals, frames and counts against the
restatement started from the device's own stage-V array, where coverage and tie-breaking are exact.

Measured on an MI355X (worst |diff| / limit over all cases; printed by the tests): view z 0.24, depth 0.33, normal 0.15; no pixel
excluded as a near-tie, no frame component off by a code."""
import math

import numpy as np
import pytest
import torch

from tests import meshrender_cases as C
from tests import meshrender_restate as R

pytestmark = pytest.mark.gpu
ALL = ("face_id", "depth", "normal", "frames", "info")
EXCLUDED_CAP = 0.01


def _device_case(case, **kw):
    from lara_amd import meshrender
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(case["vertices"]).to(dev)
    t = torch.from_numpy(case["triangles"]).to(dev)
    c = None if case["colors"] is None else torch.from_numpy(case["colors"]).to(dev)
    kw.setdefault("outputs", ALL)
    kw.setdefault("chunk", 8)
    return meshrender.render_mesh_views(case["cams"], v, t, c, keep_workspace=True, **kw)


_cache = {}


def _run(key):
    """One device run of the case (a single chunk) and the restatement from its stage-V array, shared by the tests."""
    if key not in _cache:
        from lara_amd import meshrender
        case = C.CASES[key]()
        out = _device_case(case)
        ws, n = out.pop("workspace")
        snap, keys = meshrender.workspace_sections(ws, n, case["H"], case["W"], len(case["vertices"]), len(case["triangles"]))
        snap, keys = snap.cpu().numpy().copy(), keys.cpu().numpy().copy()
        host = {k: v.cpu().numpy() for k, v in out.items()}
        vm, pm = C.matrices(case)
        refs = []
        for i in range(n):
            z = snap[i, :, 2].copy().view(np.float32).astype(np.float64)
            refs.append(R.rasterize(snap[i, :, 0], snap[i, :, 1], z, case["triangles"], case["H"], case["W"], case["znear"],
                                    case["vertices"], case["colors"], pm[i], case["eyes"][i]))
        _cache[key] = (case, host, snap, keys, refs)
    return _cache[key]


@pytest.mark.parametrize("key", sorted(C.CASES))
def test_case_equals_the_restatement(hip_lib, key):
    case, host, snap, keys, refs = _run(key)
    vm, pm = C.matrices(case)
    H, W = case["H"], case["W"]
    worst = {"z": 0.0, "depth": 0.0, "normal": 0.0}
    for i, ref in enumerate(refs):
        # ---- stage V against float64: +-1 snapped unit inside the coordinate range, beyond it on both sides; z within
        # 4.5 u sum |terms| (tests/meshrender_restate.py: snap_vertices)
        sx, sy, z, zb = R.snap_vertices(case["vertices"], vm[i], pm[i], H, W)
        for got, want in ((snap[i, :, 0], sx), (snap[i, :, 1], sy)):
            inside = np.abs(want) <= R.RANGE
            assert np.all(np.abs(got[inside].astype(np.int64) - want[inside]) <= 1), key
            assert np.all(np.abs(got[~inside].astype(np.int64)) > R.RANGE), key
        zd = snap[i, :, 2].copy().view(np.float32).astype(np.float64)
        assert np.all(np.abs(zd - z) <= zb), (key, np.max(np.abs(zd - z) / zb))
        worst["z"] = max(worst["z"], float(np.max(np.abs(zd - z) / zb, initial=0.0)))
        assert np.all(snap[i, :, 3] == 0)
        # ---- visibility: exactly the restatement's, except where its two nearest depths are an fp32 near-tie
        excluded = R.near_tie(ref)
        covered = int((ref["face"] >= 0).sum())
        print(f"{key} view {i}: covered {covered}, excluded {int(excluded.sum())}")
        assert excluded.sum() <= EXCLUDED_CAP * covered
        if case["zero_excluded"]:
            assert excluded.sum() == 0
        ok = ~excluded
        assert np.array_equal(host["face_id"][i][ok], ref["face"][ok]), key
        hit = ok & (ref["face"] >= 0)
        key_face = np.where(keys[i] == -1, -1, keys[i] & 0xFFFFFFFF)
        assert np.array_equal(key_face, host["face_id"][i])
        assert np.array_equal((keys[i] >> 32).astype(np.uint32).view(np.float32)[keys[i] != -1], host["depth"][i][keys[i] != -1])
        # ---- depth and normal, element by element within the fp32 bound of their operands
        dd = np.abs(host["depth"][i].astype(np.float64) - ref["depth"])
        assert np.all(dd[hit] <= ref["depth_bound"][hit]), key
        assert np.all(host["depth"][i][ref["face"] < 0][ok[ref["face"] < 0]] == 0.0)
        nd = np.abs(host["normal"][i].astype(np.float64) - ref["normal"]).max(-1)
        assert np.all(nd[hit] <= ref["normal_bound"][hit]), key
        assert np.all(host["normal"][i][ok & (ref["face"] < 0)] == 0.0)
        if hit.any():
            worst["depth"] = max(worst["depth"], float(np.max(dd[hit] / ref["depth_bound"][hit])))
            worst["normal"] = max(worst["normal"], float(np.max(nd[hit] / ref["normal_bound"][hit])))
        # ---- frames: at most one code off, equal wherever float64 is further from a rounding tie than its fp32 bound
        want = R.quantize(ref["colour"])
        diff = np.abs(host["frames"][i].astype(np.int64) - want.astype(np.int64))
        assert np.all(diff[ok] <= 1), key
        sure = R.tie_margin(ref) & ok[..., None]
        assert np.all(diff[sure] == 0), key
        print(f"{key} view {i}: frame codes off by one at {int((diff[ok] == 1).sum())} of {diff[ok].size} components")
        # ---- counts, exactly
        assert host["info"][i].tolist() == ref["info"].tolist(), key
    print(f"{key}: worst |diff| / limit: z {worst['z']:.3f}, depth {worst['depth']:.3f}, normal {worst['normal']:.3f}")
    exp = case["expect"]
    if "faces" in exp:
        assert set(host["face_id"][host["face_id"] >= 0].tolist()) == exp["faces"]
    if "outer_only" in exp:
        assert host["face_id"].max() < exp["outer_only"]
    if "info" in exp:
        assert host["info"][0].tolist() == exp["info"]
    if "covered" in exp:
        assert sorted((int(x), int(y)) for y, x in zip(*np.nonzero(host["face_id"][0] >= 0))) == exp["covered"]
    if "exactly_once" in exp:      # the union's pixels, counted against the restatement's: no hole on a shared edge, no overlap
        assert refs[0]["count"].max() == 1
        assert int((host["face_id"][0] >= 0).sum()) == int(refs[0]["count"].sum())
        assert np.array_equal(host["face_id"][0] >= 0, refs[0]["count"] == 1)


def test_both_work_shapes_compute_the_same_keys(hip_lib):
    """Case (g): the icosphere of (c) with every drawn triangle forced through the wave (threshold 1) and through the single
    thread (threshold 2^30); (f) likewise: its boxes are the whole image."""
    from lara_amd import meshrender
    for key in ("c", "f"):
        case, host, snap, keys, refs = _run(key)
        for threshold in (1, 1 << 30):
            out = _device_case(C.CASES[key](), wave_box_area=threshold)
            ws, n = out.pop("workspace")
            _, k2 = meshrender.workspace_sections(ws, n, case["H"], case["W"], len(case["vertices"]), len(case["triangles"]))
            assert np.array_equal(k2.cpu().numpy(), keys), (key, threshold)
            for name in ALL:
                assert np.array_equal(out[name].cpu().numpy(), host[name]), (key, threshold, name)


def test_two_runs_are_bit_identical(hip_lib):
    from lara_amd import meshrender
    for key in ("c", "d"):
        case, host, snap, keys, refs = _run(key)
        out = _device_case(C.CASES[key]())
        ws, n = out.pop("workspace")
        s2, k2 = meshrender.workspace_sections(ws, n, case["H"], case["W"], len(case["vertices"]), len(case["triangles"]))
        assert np.array_equal(k2.cpu().numpy(), keys) and np.array_equal(s2.cpu().numpy(), snap)
        for name in ALL:
            assert np.array_equal(out[name].cpu().numpy(), host[name]), (key, name)


def test_null_outputs_and_prefilled_buffers(hip_lib):
    """Each output alone equals the same output of the full call (a NULL neighbour changes nothing), and buffers the caller
    pre-filled with 0xFF bytes (NaN as floats) come back fully written."""
    from lara_amd import _native, meshrender
    case, host, snap, keys, refs = _run("i")
    for name in ALL:
        out = _device_case(C.CASES["i"](), outputs=(name,))
        assert np.array_equal(out[name].cpu().numpy(), host[name]), name
    dev = torch.device("cuda", 0)
    n, H, W = len(case["cams"]), case["H"], case["W"]
    v, t = torch.from_numpy(case["vertices"]).to(dev), torch.from_numpy(case["triangles"]).to(dev, torch.int32)
    view, proj, eye = meshrender.camera_tensors(case["cams"], dev)
    shapes = {"face_id": ((n, H, W), torch.int32), "depth": ((n, H, W), torch.float32), "normal": ((n, H, W, 3), torch.float32),
              "frames": ((n, H, W, 3), torch.uint8), "info": ((n, 4), torch.int32)}
    bufs = {}
    for name, (shape, dtype) in shapes.items():
        raw = torch.full((int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size(),), 255, dtype=torch.uint8, device=dev)
        bufs[name] = raw.view(dtype).view(shape)
    assert torch.isnan(bufs["depth"]).all()
    ws = torch.empty(_native.query("lara_meshrender_workspace_bytes", n, H, W, len(v), len(t)), dtype=torch.uint8, device=dev)
    shading = _native.host_array("f", [*meshrender.ALBEDO, *meshrender.BACKGROUND, meshrender.AMBIENT, meshrender.DIFFUSE])
    _native.call("lara_meshrender_views", dev, n, H, W, len(v), len(t), v, t, None, view, proj, eye, case["znear"], shading, 0,
                 *[bufs[k] for k in ALL], None, ws)
    for name in ALL:
        assert np.array_equal(bufs[name].cpu().numpy(), host[name]), name


def test_chunked_call_equals_unchunked(hip_lib):
    """Case (k): 3 views at chunk = 2 (a full chunk and a shorter one) against the one-chunk run."""
    case, host, snap, keys, refs = _run("k")
    assert case["chunk"] == 2 and len(case["cams"]) == 3
    for chunk in (2, 1):
        out = _device_case(C.CASES["k"](), chunk=chunk)
        for name in ALL:
            assert np.array_equal(out[name].cpu().numpy(), host[name]), (chunk, name)


def test_render_mesh_from_an_obj_equals_render_mesh_from_tensors(hip_lib, tmp_path):
    from lara_amd import meshrender
    from lara_amd.evaluate import render_mesh_turntable
    from lara_amd.mesh import write_obj
    case, host, *_ = _run("d")
    dev = torch.device("cuda", 0)
    mesh = tuple(torch.from_numpy(case[k]).to(dev) for k in ("vertices", "triangles", "colors"))
    path = str(tmp_path / "mesh.obj")
    write_obj(path, *mesh)
    cams = C.CASES["d"]()["cams"]
    for white in (True, False):
        a, b = meshrender.render_mesh(cams, path, white_bg=white), meshrender.render_mesh(cams, mesh, white_bg=white)
        assert a.is_cuda and a.dtype == torch.uint8 and tuple(a.shape) == (2, 48, 48, 3) and torch.equal(a, b)
    assert np.array_equal(b.cpu().numpy(), host["frames"])                    # (the default background is the reference's)
    assert np.array_equal(render_mesh_turntable(mesh, cams, chunk=1).cpu().numpy(), host["frames"])


def test_an_index_outside_the_vertices_raises(hip_lib):
    case = C.CASES["a"]()
    case["triangles"] = np.array([[0, 1, 2], [0, 1, 3]])
    with pytest.raises(RuntimeError, match=r"outside \[0, Nv\)"):
        _device_case(case)
    out = _device_case(case, check=False)                                    # the good triangle is drawn, the word is set
    assert int(out["error"].item()) == 1 and out["info"][0].tolist() == [1, 0, 0, 0]
    assert np.array_equal(out["face_id"].cpu().numpy(), _run("a")[1]["face_id"])


def _sphere_scene(V, H, W, radius=0.3, dist=1.5, fov=0.75):
    """Analytic depth maps of a sphere from cameras spread over all directions, in the rasteriser's pixel convention (sample
    points at integer pixels: cx = (W - 1) / 2): (depth, color, K, E, c2w)."""
    f = 0.5 * W / math.tan(0.5 * fov)
    K = np.tile(np.array([f, f, (W - 1) / 2, (H - 1) / 2], np.float32), (V, 1))
    E, depth = np.zeros((V, 4, 4), np.float32), np.zeros((V, H, W), np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    for v in range(V):
        zc = 1 - 2 * (v + 0.5) / V
        cpos = dist * np.array([math.sqrt(1 - zc * zc) * math.cos(2.399963 * v), math.sqrt(1 - zc * zc) * math.sin(2.399963 * v), zc])
        up = [0, 1.0, 0] if abs(zc) > 0.9 else [0, 0, 1.0]
        fwd = -cpos / np.linalg.norm(cpos)
        right = np.cross(fwd, up); right /= np.linalg.norm(right)
        Rm = np.stack([right, np.cross(fwd, right), fwd])
        E[v, :3, :3], E[v, :3, 3], E[v, 3, 3] = Rm, -Rm @ cpos, 1
        dirs = np.stack([(xs - K[v, 2]) / f, (ys - K[v, 3]) / f, np.ones_like(xs, float)], -1)
        o = E[v, :3, 3].astype(np.float64)
        b, dd = (dirs * o).sum(-1), (dirs * dirs).sum(-1)
        disc = b * b - dd * (o @ o - radius * radius)
        depth[v] = np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / dd, 0)
    color = np.full((V, H, W, 3), 128.0, np.float32)
    return depth, color, K, E, np.linalg.inv(E.astype(np.float64)).astype(np.float32)


def test_mesh_of_a_fused_volume_registers_with_the_fused_depth(hip_lib):
    """TSDF fusion -> marching cubes -> clean_mesh -> render_mesh_views from one of the fusing cameras: the mesh's depth
    agrees with that camera's fused depth map within 2 voxels on the pixels both cover, and they share most of the mask."""
    from lara_amd import cameras, meshrender
    from lara_amd.mesh import clean_mesh
    from lara_amd.tsdf import TSDFVolume
    res, H, W, fov = 48, 64, 64, 0.75
    voxel = 1.0 / res
    depth, color, K, E, c2w = _sphere_scene(16, H, W, fov=fov)
    vol = TSDFVolume((-0.5, -0.5, -0.5), voxel, 3 * voxel, res)
    vol.integrate(depth, color, K, E, 10.0)
    v, t, c = vol.extract_triangle_mesh()
    v, t, c, _ = clean_mesh(v, t, c)
    cams = cameras.make_cameras(torch.from_numpy(c2w[:1]), W, H, fov, fov, 0.1, 10.0, device="cuda")
    out = meshrender.render_mesh_views(cams, v, t, c, outputs=("depth", "info"))
    got = out["depth"][0].cpu().numpy()
    drawn, behind, degenerate, out_of_range = out["info"][0].tolist()
    assert drawn + degenerate == t.shape[0] and behind == 0 and out_of_range == 0      # (slivers may vanish at 1/256 pixel)
    assert degenerate < 0.01 * t.shape[0]
    mask, both = depth[0] > 0, (depth[0] > 0) & (got > 0)
    print(f"e2e: mask {int(mask.sum())}, both {int(both.sum())}, worst |diff| / voxel {np.abs(got - depth[0])[both].max() / voxel:.3f}")
    assert both.sum() > 0.5 * mask.sum()
    assert np.all(np.abs(got - depth[0])[both] <= 2 * voxel)
