"""The (points, mesh) cases tests/test_meshwind.py replays on the CPU and tests/test_meshwind_gpu.py runs through the kernels, each
held to the restatement (tests/meshwind_restate.py).  The meshes come from the suite's generators: the 1 280-face icosphere and the
8 x 64 UV sphere, the icosphere with the faces of centroid z >= 0.8 removed (1 148 left: a hole of about a tenth of the sphere), the
sphere plus an open square, the dyadic cube, the mesh with 57 triangles without area, a 257-triangle soup, 4 096 copies of one
triangle, T = 1 and T = 0 -- and each of them again with its triangles permuted ("... permuted").  The smallest shapes that still
give several levels (1 280 faces: 160 leaves under 20, 3 and 1 slots), a ragged last leaf, flagged slots and a run longer than a
leaf.  The points are
``meshsign_cases.analytic_points(1500)``, every (distinct) vertex of the mesh, points in faces' planes (on the face and beside it)
and three points that are not finite.  Everything is computed once, shared by the tests, and read-only."""
import numpy as np

from tests import meshbvh_cases as BC
from tests import meshbvh_restate as RB
from tests import meshdist_cases as C
from tests import meshdist_restate as R
from tests import meshsign_cases as SC
from tests import meshwind_restate as W

F32 = np.float32
BETAS = (2.0, 3.0, 4.0)


def holed_icosphere():
    V, F = R.icosphere(3)
    keep = V[F].astype(np.float64).mean(1)[:, 2] < 0.8
    return V, F[keep]


def _empty():
    return np.zeros((3, 3), F32), np.zeros((0, 3), np.int64)


MESHES = {
    "icosphere": lambda: R.icosphere(3), "uv_sphere": lambda: C.case_uv_sphere()[1:], "holed_icosphere": holed_icosphere,
    "sphere_square": lambda: C.case_sphere_square()[1:], "cube": SC.cube, "degenerate": lambda: C.case_degenerate()[1:],
    "soup_257": lambda: C.soup(257, 24), "copies_4096": lambda: BC.copies(4096)[1:3], "soup_1": lambda: C.soup(1, 21),
    "empty": _empty,
}
KEYS = tuple(MESHES) + tuple(k + " permuted" for k in MESHES)
CLOSED = ("icosphere", "uv_sphere", "cube")
_cache = {}


def in_plane_points(V, F, limit=48):
    """Two points per chosen face, computed in fp32 from its vertices: one on the face, one in its plane beside it."""
    if len(F) == 0:
        return np.zeros((0, 3), F32)
    ok = np.nonzero(R.valid_triangles(V, F))[0]
    pick = ok[::max(1, len(ok) // limit)][:limit]
    p0, p1, p2 = (np.asarray(V, F32)[F[pick, k]] for k in range(3))
    on = (p0 + (p1 - p0) * F32(0.25) + (p2 - p0) * F32(0.5)).astype(F32)
    beside = (p0 + (p1 - p0) * F32(1.5) + (p2 - p0) * F32(-0.75)).astype(F32)
    return np.concatenate([on, beside])


def points(V, F):
    finite_v = np.asarray(V, F32)[np.isfinite(V).all(1)]
    used = np.unique(finite_v, axis=0) if len(F) else finite_v[:0]
    bad = np.array([[np.nan, 0, 0], [0.25, np.inf, 0], [0, 0.5, -np.inf]], F32)
    return np.concatenate([SC.analytic_points(1500), used, in_plane_points(V, F), bad]).astype(F32)


def case(key):
    """{"V", "F", "P" [n,3] fp32, "w" [n] float64 brute force in id order, "mag" [n] its sum of |terms|, "n_valid"}."""
    if key not in _cache:
        name, _, permuted = key.partition(" ")
        V, F = MESHES[name]()
        V, F = np.asarray(V, F32), np.asarray(F, np.int64)
        if permuted:
            F = F[np.random.default_rng(5).permutation(len(F))]
        P = points(V, F)
        w, mag = W.brute(P, V, F)
        out = {"V": V, "F": F, "P": P, "w": w, "mag": mag}
        for a in out.values():
            a.setflags(write=False)
        out["n_valid"] = int(R.valid_triangles(V, F).sum()) if len(F) else 0
        _cache[key] = out
    return _cache[key]


def moments(key):
    """The restated hierarchy and moments of the case (None for T = 0)."""
    k = ("moments", key)
    if k not in _cache:
        c = case(key)
        _cache[k] = W.Moments(RB.BVH(c["V"], c["F"])) if len(c["F"]) else None
    return _cache[k]


def walked(key, beta):
    """(w, n_tri, n_far, mag) of the restated walk of the case under ``beta``."""
    k = ("walk", key, float(beta))
    if k not in _cache:
        c, M = case(key), moments(key)
        out = W.walk(M, c["P"], beta) if M is not None else W.winding(c["V"], c["F"], c["P"], beta)
        for a in out:
            a.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def multiplicity(key):
    """max(1, M(q)) per point, M(q) = sum |Omega_t(q)| / 4 pi from float64 brute force: how many sheets of surface the point sees.
    At most 1.5 on every mesh here but the 4 096 copies, where it reaches 1 400."""
    return np.maximum(1.0, case(key)["mag"] / W.FOUR_PI)


def approximation_error(beta, keys=KEYS):
    """{key: (max |w_walk(beta) - w_brute64|, the same with each point's error divided by ``multiplicity``)} over the case's finite
    points.  The reference is float64 brute force, never the code under test."""
    out = {}
    for key in keys:
        c = case(key)
        fin = np.isfinite(c["P"]).all(1)
        err = np.abs(walked(key, beta)[0][fin] - c["w"][fin])
        out[key] = (float(err.max()), float((err / multiplicity(key)[fin]).max()))
    return out


def E(beta, keys=KEYS, per_sheet=False):
    """The approximation error of the restated walk under ``beta`` over ``keys``: the issue's max |w_walk - w_brute64|, or the
    same per sheet of surface (see ``multiplicity``)."""
    k = ("E", float(beta), tuple(keys), per_sheet)
    if k not in _cache:
        _cache[k] = max(v[1 if per_sheet else 0] for v in approximation_error(beta, keys).values())
    return _cache[k]


def surfaces():
    """The cases whose points see at most two sheets of surface: all but the 4 096 copies."""
    return tuple(k for k in KEYS if multiplicity(k).max() <= 2.0)


def margin(key, beta=2.0):
    """Per point: 2 E_case(beta) x multiplicity, E_case the case's own error per sheet -- never more than twice the issue's E over
    all cases, and on the 4 096 copies, whose absolute error of 2.4 would exempt every point of every case, in proportion to the
    1 400 sheets a point sees there.  A point whose float64 brute-force w is farther than this from the threshold must classify as
    brute force does: the walk's error at that point is at most half of it, by the definition of E_case."""
    return 2.0 * E(beta, (key,), per_sheet=True) * multiplicity(key)


def term_pairs():
    """{name: (q [n,3], triangles [n,3,3])}: the (query, triangle) groups of tests/meshbvh_cases.bound_pairs -- random ones over seven
    decades, flat ones with the query a rounding above the plane, queries on the box, triangles that are a point or a segment --
    and, from the cases, every in-plane point and every vertex against faces of its own mesh."""
    out = {k: (v[0], v[1]) for k, v in BC.bound_pairs().items()}
    for key in ("cube", "icosphere", "degenerate", "copies_4096"):
        c = case(key)
        tri = np.asarray(c["V"], F32)[c["F"]]
        P = c["P"][1500:-3]
        take = np.arange(len(P) * 12) % len(tri)
        out["case " + key] = (np.repeat(P, 12, 0), tri[(take + np.repeat(np.arange(len(P)), 12)) % len(tri)])
    V, F = SC.cube()
    tri = V[F]
    on = in_plane_points(V, F)
    out["cube, every in-plane point x every face"] = (np.repeat(on, len(tri), 0), np.tile(tri, (len(on), 1, 1)))
    out["cube, every vertex x every face"] = (np.repeat(V, len(tri), 0), np.tile(tri, (len(V), 1, 1)))
    return out
