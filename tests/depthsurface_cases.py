"""The inputs of tests/test_depthsurface.py and tests/test_depthsurface_gpu.py: analytic, built in numpy, at the smallest shapes at
which the kernels of csrc/depthsurface.hip can still go wrong (a compaction workgroup covers 1024 items in four passes of 256, a
wave 64).  Every case is a dict: depth [V,H,W] fp32, mask (or None), ixt [V,3,3] and c2w [V,4,4] float64, plus what it adds."""
import numpy as np

RADIUS = 0.5
SPHERE4_EYES = ((2.0, 0.0, 0.3), (-1.0, 1.7, 0.2), (-0.8, -1.6, -0.7), (0.1, 0.2, 2.0))


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """c2w [4,4] float64 of a camera at ``eye`` looking at ``target``: x right, y down, z forward."""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = r, d, f, eye
    return M


def intrinsics(V, fx, fy, cx, cy):
    K = np.zeros((V, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = fx, fy, cx, cy, 1.0
    return K


def raycast_spheres(c2w, K, H, W, radii=(RADIUS,)):
    """(depth [V,H,W] fp32 -- the view-space z of the first hit of concentric spheres at the origin, 0 where the ray misses --,
    mask [V,H,W] uint8, world normals [V,H,W,3] float64 of the hit), ray-cast in float64."""
    V = len(c2w)
    depth, mask, nrm = np.zeros((V, H, W), np.float32), np.zeros((V, H, W), np.uint8), np.zeros((V, H, W, 3))
    x, y = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    for v in range(V):
        dirs = np.stack([(x - K[v, 0, 2]) / K[v, 0, 0], (y - K[v, 1, 2]) / K[v, 1, 1], np.ones_like(x)], axis=-1) @ c2w[v, :3, :3].T
        o = c2w[v, :3, 3]
        a, b = (dirs * dirs).sum(-1), (dirs * o).sum(-1)
        best = np.full((H, W), np.inf)
        for rad in radii:
            disc = b * b - a * (o @ o - rad * rad)
            s = (-b - np.sqrt(np.where(disc >= 0, disc, 0))) / a
            best = np.where((disc >= 0) & (s > 0) & (s < best), s, best)
        hit = np.isfinite(best)
        depth[v], mask[v] = np.where(hit, best, 0.0), hit
        p = o + np.where(hit, best, 0.0)[..., None] * dirs
        nrm[v] = np.where(hit[..., None], p / np.maximum(np.linalg.norm(p, axis=-1, keepdims=True), 1e-30), 0.0)
    return depth, mask, nrm


_cache = {}


def sphere4():
    """A sphere of radius 0.5 seen by four cameras looking at the origin, 24 x 32 (not square: a swapped axis shows), fx = fy = 40,
    the principal point at (W / 2, H / 2): 332 to 368 valid pixels per view."""
    if "sphere4" not in _cache:
        H, W = 24, 32
        c2w = np.stack([look_at(e) for e in SPHERE4_EYES])
        K = intrinsics(4, 40.0, 40.0, W / 2, H / 2)
        depth, mask, nrm = raycast_spheres(c2w, K, H, W)
        _cache["sphere4"] = {"depth": depth, "mask": mask, "ixt": K, "c2w": c2w, "normal_map": nrm.astype(np.float32)}
    return _cache["sphere4"]


def mask_as(mask, kind):
    """The uint8 0 / 1 mask in another spelling: "uint8" (1 and 255), "bool", "float32" (1, 0.5 and a NaN count; 0 and -0 do not)."""
    m = np.asarray(mask) != 0
    flat = np.arange(m.size).reshape(m.shape)
    if kind == "bool":
        return m
    if kind == "uint8":
        return np.where(m, np.where(flat % 2 == 0, 1, 255), 0).astype(np.uint8)
    assert kind == "float32"
    on = np.choose(flat % 3, [np.float32(1.0), np.float32(0.5), np.float32(np.nan)])
    off = np.where(flat % 2 == 0, np.float32(0.0), np.float32(-0.0))
    return np.where(m, on, off).astype(np.float32)


EDGES_DEPTH_MAX = 5.0


def edges(total):
    """V = 3, H = 5, W = 67 (a row longer than a wave, and odd; 1005 pixels: the last compaction workgroup is not full); view 1
    entirely invalid (an empty stretch in the middle of the scan); exactly ``total`` valid pixels (255, 256, 257: the ends of a
    pass of 256).  The invalid pixels cycle through NaN, +inf, a negative and a zero depth (mask 1), a positive depth under mask 0
    and a depth above depth_max = 5 (mask 1)."""
    V, H, W = 3, 5, 67
    g = np.random.default_rng(100 + total)
    depth = (1.0 + g.random((V, H, W))).astype(np.float32)
    mask = np.ones((V, H, W), np.uint8)
    ok = np.zeros((V, H, W), bool)
    pool = np.concatenate([np.arange(0, H * W), np.arange(2 * H * W, 3 * H * W)])
    chosen = g.choice(pool, total, replace=False)
    chosen[:2] = [0, V * H * W - 1]          # the first and the last pixel of all
    chosen = np.unique(chosen)
    while len(chosen) < total:
        chosen = np.unique(np.append(chosen, g.choice(pool)))
    ok.reshape(-1)[chosen] = True
    bad = np.nonzero(~ok.reshape(-1))[0]
    kinds = np.arange(len(bad)) % 6
    d, m = depth.reshape(-1), mask.reshape(-1)
    d[bad[kinds == 0]] = np.nan
    d[bad[kinds == 1]] = np.inf
    d[bad[kinds == 2]] = -1.25
    d[bad[kinds == 3]] = 0.0
    m[bad[kinds == 4]] = 0
    d[bad[kinds == 5]] = 9.0
    c2w = np.stack([look_at((2.0, 0.5, 0.3)), look_at((-1.0, 1.7, 0.2)), look_at((0.3, -1.9, 1.1))])
    return {"depth": depth, "mask": mask, "ixt": intrinsics(V, 50.0, 45.0, 33.25, 2.5), "c2w": c2w, "depth_max": EDGES_DEPTH_MAX,
            "total": total}


def single():
    """V = H = W = 1, no mask."""
    return {"depth": np.array([[[1.5]]], np.float32), "mask": None, "ixt": intrinsics(1, 2.0, 2.0, 0.5, 0.5),
            "c2w": look_at((1.0, 2.0, 3.0))[None]}


def stride_case():
    """V = 2, H = 7, W = 9, every pixel valid but three: strides 2 and 3 take every 2nd / 3rd row and column from 0."""
    g = np.random.default_rng(7)
    depth = (1.0 + g.random((2, 7, 9))).astype(np.float32)
    mask = np.ones((2, 7, 9), np.uint8)
    mask[0, 0, 0] = mask[1, 6, 6] = mask[1, 2, 4] = 0
    return {"depth": depth, "mask": mask, "ixt": intrinsics(2, 9.0, 9.0, 4.5, 3.5), "c2w": np.stack([look_at((2, 0, 0.3)), look_at((0, -2, 1))])}


BACKPROJECT_CASES = {"sphere4": sphere4, "edges_255": lambda: edges(255), "edges_256": lambda: edges(256), "edges_257": lambda: edges(257),
                     "single": single, "stride": stride_case}

TAU = 0.01
QUERY_SIZES = (1, 255, 256, 257, 4096)


def fibonacci_sphere(n):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def queries(n):
    """``n`` fp32 points on the sphere of `sphere4`, their radius moved by a seeded uniform +-0.03 (tau = 0.01: some lie in front
    of the seen surface, some further behind it than tau)."""
    g = np.random.default_rng(1000 + n)
    return (fibonacci_sphere(n) * (RADIUS + g.uniform(-0.03, 0.03, n))[:, None]).astype(np.float32)


def queries_special():
    """Behind a camera, outside every frustum, non-finite, near the centre (occluded everywhere), and a point in front of the
    sphere."""
    eyes = np.asarray(SPHERE4_EYES)
    return np.concatenate([eyes * 1.5, [[50.0, 60.0, 70.0], [3.0, -7.0, -40.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0],
                                       [0.1, -np.inf, np.nan], [0.013, 0.021, 0.005], [1.0, 0.013, 0.16]]]).astype(np.float32)


def thin_sets():
    """{name: (points [N,3] fp32, voxel)}: the sphere4 points at about 16 cells per axis; 1000 copies of one point; a single
    point; 300 points in one cell; the sphere4 points with NaN / infinite rows in front, inside and at the end."""
    from tests import depthsurface_restate as R
    c = sphere4()
    k, pose = R.cameras(c["ixt"], c["c2w"])
    P = R.backproject(c["depth"], c["mask"], k, pose)["points32"]
    g = np.random.default_rng(5)
    bad = P.copy()
    bad[0] = [np.nan, 0, 0]
    bad[100, 1] = np.inf
    bad[101, 2] = -np.inf
    bad[-1] = np.nan
    return {"sphere4": (P, 1.0 / 16), "copies": (np.tile(np.float32([[0.25, -3.0, 1e-3]]), (1000, 1)), 0.01),
            "single": (np.float32([[0.3, -0.2, 0.9]]), 0.5), "one_cell": ((g.random((300, 3)) * 0.01).astype(np.float32), 1.0),
            "nan_rows": (bad, 1.0 / 16)}


def uv_sphere(radius, n_lat=24, n_lon=48):
    """(vertices [Nv,3] fp32, triangles [T,3] int64) of a UV sphere, outward orientation."""
    V = [[0.0, 0.0, radius]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            V.append([radius * np.sin(th) * np.cos(ph), radius * np.sin(th) * np.sin(ph), radius * np.cos(th)])
    V.append([0.0, 0.0, -radius])
    F = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    for j in range(n_lon):
        F.append([0, ring(1, j), ring(1, j + 1)])
        F.append([len(V) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            F.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            F.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    return np.asarray(V, np.float32), np.asarray(F, np.int64)


def nested_spheres():
    """The UV sphere of radius 0.5 plus an inner one of radius 0.3 that no view can see: (vertices, triangles, the inner sphere's
    share of the area, 0.3^2 / (0.5^2 + 0.3^2) = 0.2647)."""
    Va, Fa = uv_sphere(RADIUS)
    Vb, Fb = uv_sphere(0.3)
    return np.concatenate([Va, Vb]), np.concatenate([Fa, Fb + len(Va)]), 0.09 / 0.34
