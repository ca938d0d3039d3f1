"""The (points, mesh) cases tests/test_meshsign.py replays on the CPU and tests/test_meshsign_gpu.py runs through the kernels, each
held to restated brute force (tests/meshsign_restate.py).  The meshes are those of tests/meshray_cases.CASES and the points are the
origins of their rays (around and inside the mesh, on faces' planes, non-finite ones among them); the seeded points of the analytic
test; the cube with dyadic vertices and the points from which a ray meets a corner or an edge exactly; the three triangles that
leave the origin without a usable ray."""
import numpy as np

from tests import meshdist_restate as R
from tests import meshray_cases as MC
from tests import meshsign_restate as S

F32 = np.float32
_cache = {}


def case(key):
    """{"V", "F", "P" [n,3] fp32, "cross" [n,3] int32, "wind" [n,3] int32}: the restated brute force of all three rays, computed
    once and shared by the tests; nothing changes it."""
    if key not in _cache:
        c = MC.case(key)
        P = np.array(c["o"], F32)
        cross, wind = S.rows(P, S.MAX_RAYS, c["V"], c["F"])
        out = {"V": c["V"], "F": c["F"], "P": P, "cross": cross, "wind": wind}
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def analytic_points(n=1500, seed=77):
    """n seeded points in [-1.3, 1.3]^3."""
    return (np.random.default_rng(seed).random((n, 3)) * 2.6 - 1.3).astype(F32)


def inscribed_radius(V, F):
    """The smallest distance from the origin to a triangle, float64."""
    p0, p1, p2 = R.corners(V, F)
    return float(np.sqrt(R.point_triangle(np.zeros((1, 3), F32), p0, p1, p2)[0].min()))


def cube():
    """(V [8,3], F [12,3]): the cube with vertices +-0.5, outward windings; vertex i = (bit 0, bit 1, bit 2 of i) - 0.5."""
    V = np.array([[(i & 1) - 0.5, (i >> 1 & 1) - 0.5, (i >> 2 & 1) - 0.5] for i in range(8)], F32)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    F = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)
    return V, F


def touching_points():
    """[(ray k, points)]: from V - 0.25 D0 ray 0 meets corner V, from V - 2 D1 ray 1 does, and from the fp32 midpoint of each
    face's first edge less 0.125 D2 ray 2 meets that edge.  Every product is exact in fp32: the meeting is exact too."""
    V, F = cube()
    D = S.DIRECTIONS
    mid = ((V[F[:, 0]] + V[F[:, 1]]) * F32(0.5)).astype(F32)
    return [(0, (V - F32(0.25) * D[0]).astype(F32)), (1, (V - F32(2) * D[1]).astype(F32)), (2, (mid - F32(0.125) * D[2]).astype(F32))]


def no_usable_ray():
    """(V, F): three small triangles, triangle k with its first vertex at 2 D_k; from the origin every ray meets a vertex."""
    D = S.DIRECTIONS.astype(np.float64)
    V = []
    for k in range(3):
        a = 2 * D[k]
        u = np.cross(D[k], D[(k + 1) % 3])
        v = np.cross(D[k], u)
        V += [a, a + 0.125 * u + 0.0625 * v, a - 0.0625 * u + 0.125 * v]
    return np.array(V, F32), np.arange(9, dtype=np.int64).reshape(3, 3)
