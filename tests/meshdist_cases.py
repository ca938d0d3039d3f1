"""The (queries, mesh) cases tests/test_meshdist.py replays through the restated grid search and tests/test_meshdist_gpu.py runs
through the kernels: each is held to float64 brute force.  Triangle counts cover 1, 2, 63, 257 and 1 280, query counts 1, 63,
257, 1 000 and 4 096; the named meshes have the sizes their construction gives."""
import numpy as np

from tests import meshdist_restate as R
from tests import meshmetrics_restate as MR

F32 = np.float32


def _rng(seed):
    return np.random.default_rng(seed)


def soup(T, seed, size=0.08):
    """T small triangles scattered in the unit cube (a vertex list of their own each)."""
    g = _rng(seed)
    base = g.random((T, 1, 3))
    V = (base + (g.random((T, 3, 3)) - 0.5) * size).reshape(-1, 3).astype(F32)
    return V, np.arange(3 * T, dtype=np.int64).reshape(T, 3)


def case_soup(T, N, seed):
    V, F = soup(T, seed)
    return _rng(seed + 100).random((N, 3)).astype(F32), V, F


def case_one_triangle():
    """One triangle and queries over its interior, over each edge region and over each vertex region, at three heights (0: in the
    plane), and the three vertices themselves."""
    V = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], F32)
    bary = [(0.3, 0.3, 0.4), (0.6, 0.6, -0.2), (-0.3, 0.7, 0.6), (0.5, -0.4, 0.9), (1.5, -0.2, -0.3), (-0.3, 1.6, -0.3), (-0.2, -0.3, 1.5)]
    Q = [b[0] * V[0] + b[1] * V[1] + b[2] * V[2] + np.array([0, 0, z]) for z in (0.0, 0.5, -2.0) for b in bary]
    return np.concatenate([np.array(Q, F32), V, _rng(1).normal(size=(63 - 24, 3)).astype(F32) * 3]), V, np.array([[0, 1, 2]], np.int64)


def case_icosphere():
    V, F = R.icosphere(3)
    return R.rippled_sphere_points(1000, 2), V, F


def case_uv_sphere():
    """64 x 8: slivers of aspect 1 : 8 at the poles."""
    V, F = MR.uv_sphere(n_lat=8, n_lon=64)
    return R.rippled_sphere_points(1000, 3), V, F


def case_sphere_square():
    """The icosphere and, as its last two triangles, a square through its middle that spans the whole box: they go to the large
    list.  The last 257 queries lie within 0.03 of the square and at least 0.4 inside the sphere."""
    V, F = R.icosphere(3)
    sq = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F32)
    F = np.concatenate([F, len(V) + np.array([[0, 1, 2], [0, 2, 3]])])
    g = _rng(4)
    near = np.concatenate([(g.random((257, 2)) - 0.5) * 0.8, (g.random((257, 1)) - 0.5) * 0.06], 1).astype(F32)
    return np.concatenate([R.rippled_sphere_points(743, 5), near]), np.concatenate([V, sq]), F


def case_fan():
    """256 wedges around the origin; queries within 0.01 of the disc."""
    V, F = R.fan(256)
    g = _rng(6)
    rad, ang = np.sqrt(g.random(1000)) * 0.98, g.random(1000) * 2 * np.pi
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), (g.random(1000) - 0.5) * 0.02], 1).astype(F32), V, F


def case_degenerate():
    """200 small triangles and 57 without area among them: collinear ones, ones with a vertex repeated twice, and single points."""
    V, F = soup(257, 7)
    g = _rng(8)
    for k, i in enumerate(g.permutation(257)[:57]):
        a, b = V[3 * i].copy(), V[3 * i + 1].copy()
        if k % 3 == 0:
            V[3 * i + 2] = a + (b - a) * F32(2.0)          # collinear
        elif k % 3 == 1:
            V[3 * i + 2] = a                                # a vertex twice: the segment a b
        else:
            F[i] = F[i, 0]                                  # one vertex three times: a point
    return g.random((257, 3)).astype(F32), V, F


def case_cell_faces():
    """R = 8 over [0, 1]^3, h = 1/8 exactly: 256 triangles whose vertices are lattice points i / 8 (on grid planes, some on the box's
    maximum corner); queries: lattice points (on cell faces, edges and corners), cell centres, and random ones."""
    g = _rng(9)
    base = g.integers(0, 7, (256, 1, 3))
    tri = np.clip(base + g.integers(0, 3, (256, 3, 3)), 0, 8)
    tri[0], tri[1] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[8, 8, 8], [7, 8, 8], [8, 7, 8]]
    V = (tri.reshape(-1, 3) / 8.0).astype(F32)
    Q = np.concatenate([g.integers(0, 9, (129, 3)) / 8.0, (g.integers(0, 8, (64, 3)) + 0.5) / 8.0, g.random((64, 3))]).astype(F32)
    return Q, V, np.arange(768, dtype=np.int64).reshape(256, 3)


def case_outside():
    """Queries outside the box on every side, near and 10 x the extent away, along axes and diagonals."""
    V, F = R.icosphere(3)
    g = _rng(10)
    Q = []
    for axis in range(3):
        for side in (-1, 1):
            for far in (0.01, 0.5, 10.0):
                q = g.random(3) * 2 - 1
                q[axis] = side * (1 + far)
                Q.append(q)
    for sign in ((1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1)):
        for far in (0.1, 10.0):
            Q.append(np.array(sign, np.float64) * (1 + far))
    Q = np.array(Q)
    return np.concatenate([Q, g.random((63 - len(Q), 3)) * 60 - 30]).astype(F32), V, F


def case_inside():
    """Queries within radius 0.3 of the icosphere's centre: the surface is more than RMAX rings away."""
    V, F = R.icosphere(3)
    g = _rng(11)
    d = g.normal(size=(257, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True) * 0.3 * g.random((257, 1))).astype(F32), V, F


def case_termination():
    """R = 16 over [0, 1]^3 (1 000 triangles, h = 1/16), every triangle 0.01 h small.  Each query sits near a corner of its cell; its
    own cell (ring 0) holds a triangle at the far corner, 1.4 h away, and the nearest one lies 0.26 h away in the DIAGONAL cell of
    ring 1 (or in the edge-diagonal cell): stopping at the first ring that holds a candidate returns the wrong face.  A third group:
    ring 1 holds a candidate 2.5 h away in its corner cell while the nearest lies 1.55 h away in a cell of ring 2.  The nearest
    triangles have odd ids from 3 on."""
    g = _rng(12)
    h = 1.0 / 16
    Q, P = [], [[0, 0, 0], [1, 1, 1]]
    cells = [(8, 8, 8), (3, 12, 5), (12, 4, 10), (5, 5, 13), (10, 10, 2), (13, 7, 7), (6, 2, 9)]
    for k, (cx, cy, cz) in enumerate(cells):
        c = np.array([cx, cy, cz], np.float64)
        j = g.random(3) * 0.02
        if k % 3 == 0:
            Q.append((c + 0.9 + j) * h); P.append((c + 0.1) * h); P.append((c + 1.05) * h)
        elif k % 3 == 1:
            Q.append((c + [0.9, 0.9, 0.5] + j) * h); P.append((c + [0.1, 0.1, 0.5]) * h); P.append((c + [1.05, 1.05, 0.5]) * h)
        else:
            Q.append((c + 0.5 + j) * h); P.append((c - 0.95) * h); P.append((c + [2.05, 0.5, 0.5]) * h)
    P = np.array(P)
    P = np.concatenate([P, g.random((1000 - len(P), 3)) * [0.08, 1, 1]])          # the filler is far away: x < 0.08
    off = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) * (0.01 * h)
    tri = P[:, None, :] + off[None]
    tri[1] = [[1, 1, 1], [1 - 0.01 * h, 1, 1], [1, 1 - 0.01 * h, 1]]              # the box stays [0, 1]^3
    V = tri.reshape(-1, 3).astype(F32)
    return np.concatenate([np.array(Q, F32)] * 9)[:63], V, np.arange(3000, dtype=np.int64).reshape(1000, 3)


def case_identical():
    """Two identical triangles: face 0 everywhere."""
    V = np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.6]], F32)
    return (_rng(13).random((257, 3)) * 2 - 0.5).astype(F32), np.concatenate([V, V]), np.array([[0, 1, 2], [3, 4, 5]], np.int64)


BAD = (5, 9, 20)


def case_bad_triangles():
    """63 triangles; number 5 has an index beyond Nv, number 9 a negative one, number 20 a vertex with a NaN coordinate.  The first
    queries sit on the sound vertices of those triangles: a search that kept them in any form would return them there."""
    V, F = soup(63, 14)
    F[5, 2], F[9, 0] = len(V) + 3, -1
    V[3 * 20 + 1, 1] = np.nan
    g = _rng(15)
    Q = g.random((63, 3)).astype(F32)
    Q[0], Q[1], Q[2] = V[F[5, 0]], V[F[9, 1]], V[F[20, 0]]
    return Q, V, F


CASES = {
    "soup_1_4096": lambda: case_soup(1, 4096, 21), "soup_2_1000": lambda: case_soup(2, 1000, 22),
    "soup_63_257": lambda: case_soup(63, 257, 23), "soup_257_63": lambda: case_soup(257, 63, 24),
    "soup_1280_1": lambda: case_soup(1280, 1, 25), "soup_1280_4096": lambda: case_soup(1280, 4096, 26),
    "one_triangle": case_one_triangle, "icosphere": case_icosphere, "uv_sphere": case_uv_sphere,
    "sphere_square": case_sphere_square, "fan": case_fan, "degenerate": case_degenerate, "cell_faces": case_cell_faces,
    "outside": case_outside, "inside": case_inside, "termination": case_termination, "identical": case_identical,
    "bad_triangles": case_bad_triangles,
}
NEAR_SURFACE = ("icosphere", "uv_sphere", "sphere_square", "fan")          # the fallback share must stay <= 1 %
FALLBACK_CAP = 0.01


def check_against_brute_force(key, Q, V, F, d, face, d64_min, d2_all):
    """The two bars of the issue for one case: (worst distance ratio, worst choice ratio), both <= 1 to pass.  ``d`` [N] as the
    code under test returned it (float64 of an fp32), ``face`` [N]; ``d64_min``, ``d2_all`` from ``R.brute``."""
    S = R.scale(Q, V, F)
    slack = 2.0 ** -40 * S
    assert np.all((face >= 0) & (face < len(F))), key
    d64 = np.sqrt(d2_all[np.arange(len(Q)), face])
    assert np.all(np.isfinite(d64)), (key, "an invalid triangle was chosen")
    r_dist = float((np.abs(d - d64) / (8 * R.U * d64 + slack)).max()) if slack > 0 else float(np.abs(d - d64).max() > 0)
    r_choice = float(((d64 - d64_min) / (8 * R.U * d64_min + slack)).max()) if slack > 0 else float((d64 - d64_min).max() > 0)
    return r_dist, r_choice
