"""The (rays, mesh) cases tests/test_meshray.py replays through the restated walk and tests/test_meshray_gpu.py runs through the
kernels, each held to restated brute force (tests/meshray_restate.py); the watertightness rays; the adversarial (ray, triangle,
box) groups of the bound.  The meshes are those of tests/meshdist_cases.py; ray counts cover 1, 63, 257, 1 000 and 4 096."""
import numpy as np

from tests import meshbvh_cases as BC
from tests import meshdist_cases as C
from tests import meshdist_restate as R
from tests import meshray_restate as RR

F32 = np.float32
KINDS = ("random", "from inside", "axis-aligned", "negative d[kz]", "misses", "in a face's plane", "at a vertex or an edge",
         "t_min past the first hit", "t_max before the first hit", "special")


def rays(V, F, n, seed):
    """(o [n,3], d [n,3], t_min [n], t_max [n]) fp32: ray i is of kind KINDS[i % 10].
      random                       origins around the mesh, any direction
      from inside                  origins near the middle of the mesh's box
      axis-aligned                 two zero components, through a face's centroid
      negative d[kz]               from beyond the box's upper corner back to a centroid: the dominant component is negative
      misses                       outside, pointing away
      in a face's plane            from a point of the face's plane outside the face to its centroid
      at a vertex or an edge       aimed at a vertex or at the midpoint of an edge
      t_min past the first hit     the window starts 2^-10 behind the first hit: the second must come back
      t_max before the first hit   from inside, the window [-4, first hit less 2^-10]: a hit BEHIND the origin comes back, or none
      special                      d = 0, a NaN or an infinity in d or o, d denormal, in turn"""
    g = np.random.default_rng(seed)
    ok = R.valid_triangles(V, F)
    p = [x[ok].astype(np.float64) for x in R.corners(V, F)]
    cen = (p[0] + p[1] + p[2]) / 3.0
    lo, hi = np.stack(p).min((0, 1)), np.stack(p).max((0, 1))
    mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 1e-2)
    kind = (np.arange(n) + (2 if n == 1 else 0)) % 10          # (a single ray: one that hits)
    pick = g.integers(0, len(cen), n)
    target = cen[pick]
    unit = g.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    o = mid + (g.random((n, 3)) * 3 - 1.5) * ext                                                  # random
    d = g.normal(size=(n, 3))
    k = kind == 1
    o[k] = (mid + (g.random((n, 3)) - 0.5) * 0.2 * ext)[k]
    k = kind == 2
    axis, sign = g.integers(0, 3, n), g.choice([-1.0, 1.0], n)
    ax = np.zeros((n, 3))
    ax[np.arange(n), axis] = sign * (0.5 + 1.5 * g.random(n))
    o[k], d[k] = (target - ax * (1 + 2 * g.random((n, 1))) * ext.max())[k], ax[k]
    k = kind == 3
    off = (g.random((n, 3)) * 0.5 + [0.0, 0.0, 0.0]) * ext
    off[np.arange(n), axis] += 2 * ext.max()
    o[k], d[k] = (target + off)[k], (-off)[k]
    k = kind == 4
    o[k], d[k] = (mid + unit * 3 * np.linalg.norm(ext))[k], (unit + 0.2 * g.normal(size=(n, 3)))[k]
    k = kind == 5
    ab = np.array([[-1.5, 0.7], [0.6, 1.9], [2.2, -0.4], [-0.8, -0.8]])[g.integers(0, 4, n)]
    start = p[0][pick] + ab[:, :1] * (p[1][pick] - p[0][pick]) + ab[:, 1:] * (p[2][pick] - p[0][pick])
    o[k], d[k] = start[k], (target - start)[k]
    k = (kind >= 6) & (kind <= 8)
    corner = np.stack(p, 1)[pick, g.integers(0, 3, n)]
    edge = (np.stack(p, 1)[pick, 0].astype(F32) + np.stack(p, 1)[pick, 1].astype(F32)) * F32(0.5)
    aim = np.where((kind == 6)[:, None], np.where((np.arange(n) % 20 < 10)[:, None], corner, edge), target)
    o[k] = (mid + unit * (1.5 + g.random((n, 1))) * np.linalg.norm(ext))[k]
    o[kind == 8] = (mid + (g.random((n, 3)) - 0.5) * 0.2 * ext)[kind == 8]
    o, d = o.astype(F32), d.astype(F32)
    d[k] = (aim.astype(F32) - o)[k]
    k = kind == 9
    o[k], d[k] = (mid + (g.random((n, 3)) - 0.5) * 0.2 * ext).astype(F32)[k], (aim.astype(F32) - o)[k]
    for j, i in enumerate(np.nonzero(k)[0]):
        which = j % 7
        if which == 0:
            d[i] = 0
        elif which == 1:
            d[i, j % 3] = np.nan
        elif which == 2:
            d[i, j % 3] = np.inf
        elif which == 3:
            o[i, j % 3] = np.nan
        elif which == 4:
            o[i, j % 3] = -np.inf
        elif which == 5:
            d[i] = d[i] * F32(2.0 ** -140)                                                         # denormal components
    t_min, t_max = np.zeros(n, F32), np.full(n, np.inf, F32)
    w = (kind == 7) | (kind == 8)
    if w.any():
        first = RR.brute(o[w], d[w], V, F)[3]
        first = np.where(np.isfinite(first), first, 1.0)
        idx = np.nonzero(w)[0]
        past = kind[idx] == 7
        t_min[idx[past]] = (first[past] * (1 + 2.0 ** -10)).astype(F32)
        t_min[idx[~past]], t_max[idx[~past]] = F32(-4), (first[~past] * (1 - 2.0 ** -10)).astype(F32)
    return o, d, t_min, t_max


def _mesh(key):
    return C.CASES[key]()[1:]


def _copies():
    return BC.copies(4096)[1:3]


CASES = {
    "one_triangle": (lambda: _mesh("one_triangle"), 63), "icosphere": (lambda: _mesh("icosphere"), 1000),
    "uv_sphere": (lambda: _mesh("uv_sphere"), 1000), "sphere_square": (lambda: _mesh("sphere_square"), 4096),
    "fan": (lambda: _mesh("fan"), 257), "degenerate": (lambda: _mesh("degenerate"), 257),
    "bad_triangles": (lambda: _mesh("bad_triangles"), 63), "copies_4096": (_copies, 257),
    "soup_1": (lambda: C.soup(1, 21), 4096), "soup_2": (lambda: C.soup(2, 22), 1000), "soup_63": (lambda: C.soup(63, 23), 257),
    "soup_257": (lambda: C.soup(257, 24), 63), "soup_257_one_ray": (lambda: C.soup(257, 24), 1),
}
_cache = {}


def case(key):
    """{"V", "F", "o", "d", "t_min", "t_max", and the restated brute force: "t" fp32, "face", "bary", "t64", "hits", "rejected"},
    computed once and shared by the tests; nothing changes it."""
    if key not in _cache:
        make, n = CASES[key]
        V, F = make()
        o, d, t_min, t_max = rays(V, F, n, 700 + sorted(CASES).index(key))
        t, face, bary, t64, hits, rej = RR.brute(o, d, V, F, t_min, t_max)
        c = {"V": V, "F": F, "o": o, "d": d, "t_min": t_min, "t_max": t_max, "t": t, "face": face, "bary": bary, "t64": t64,
             "hits": hits, "rejected": rej}
        for a in c.values():
            a.setflags(write=False)
        _cache[key] = c
    return _cache[key]


WATERTIGHT_ORIGINS = ((0.0, 0.0, 0.0), (0.3, -0.2, 0.1), (0.5, 0.25, -0.125))


def watertight_meshes():
    return {"icosphere": _mesh("icosphere"), "uv_sphere": _mesh("uv_sphere")}


def watertight_rays(V, F, origin, scale=1.0):
    """(o, d): from ``origin`` to every vertex, to the fp32 midpoint of the first two edges of every face and to every fp32
    centroid; d = fl32(target - o), times ``scale``."""
    V = np.asarray(V, F32)
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    targets = np.concatenate([V, (p0 + p1) * F32(0.5), (p1 + p2) * F32(0.5), ((p0 + p1) + p2) / F32(3)]).astype(F32)
    o = np.broadcast_to(np.asarray(origin, F32), targets.shape).copy()
    return o, ((targets - o).astype(F32) * F32(scale)).astype(F32)


def visibility_cases():
    """{name: (V, F, points [N,3], skip [N] or None, eyes [E,3], shrink)}: samples ON the icosphere seen from outside (half of
    them face away from an eye) with their faces skipped; the same without the skip list and a larger shrink; points inside and
    outside the sphere plus square, eyes inside and outside, non-finite points, a point that is an eye; 64 eyes around the fan."""
    g = np.random.default_rng(900)
    out = {}
    V, F = _mesh("icosphere")
    f = g.integers(0, len(F), 257)
    w = g.dirichlet(np.ones(3), 257)
    P = (w[:, :, None] * V[F[f]].astype(np.float64)).sum(1).astype(F32)
    eyes = np.array([[3, 0, 0.5], [-2, 2, 0], [0.1, -0.2, 4], [0, 0, 0], [-1.5, -1.5, -1.5]], F32)
    out["icosphere, own faces skipped"] = (V, F, P, f.astype(np.int32), eyes, 2.0 ** -10)
    out["icosphere, nothing skipped"] = (V, F, P, None, eyes, 2.0 ** -6)
    V, F = _mesh("sphere_square")
    P = ((g.random((1000, 3)) * 2.6 - 1.3)).astype(F32)
    P[5], P[6], P[7] = [np.nan, 0, 0], [0, np.inf, 0], [0.25, 0.5, 2.0]
    eyes = np.array([[0.25, 0.5, 2.0], [0.2, 0.1, 0.5], [0.2, 0.1, -0.5], [-3, -2, 1], [0, 0, 0], [2, 2, 2], [1, 0, 0]], F32)
    out["sphere and square"] = (V, F, P, None, eyes, 2.0 ** -10)
    V, F = R.fan(256)
    ang = 2 * np.pi * np.arange(64) / 64
    eyes = np.stack([1.5 * np.cos(ang), 1.5 * np.sin(ang), np.where(np.arange(64) % 2 == 0, 0.5, -0.5)], 1).astype(F32)
    P = np.concatenate([g.random((63, 2)) * 2 - 1, (g.random((63, 1)) - 0.5) * 0.6], 1).astype(F32)
    out["fan, 64 eyes"] = (V, F, P, None, eyes, 0.0)
    return out


def _tight(tri):
    return tri.min(1), tri.max(1)


def bound_groups(n=6000):
    """{name: (o, d, t_min, t_max, triangles [n,3,3], box lo, box hi)} fp32, the box holding the triangle's vertices: tight unless
    the name says larger.  Every ray is aimed at a point of its triangle (interior, edge or vertex), so most of them hit."""
    g = np.random.default_rng(910)
    out = {}

    def aimed(tri, origin=None, shift=0.0):
        """(o, d, t_min, t_max): rays at a point of each triangle -- in one of four at an edge, in one of four at a vertex -- from
        an origin 0.01 to 10 sizes away (or ``origin``), d scaled by 0.01 to 100, half of the windows ending at twice the aim."""
        tri64 = tri.astype(np.float64)
        m = len(tri)
        w = g.dirichlet(np.ones(3), m)
        sel = g.integers(0, 4, m)
        w[sel == 1, 2] = 0.0                                                                    # on the edge p0 p1
        w[sel == 1] /= w[sel == 1].sum(1, keepdims=True)
        w[sel == 2] = np.eye(3)[g.integers(0, 3, (sel == 2).sum())]                            # at a vertex
        aim = (w[:, :, None] * tri64).sum(1)
        S = np.abs(tri64 - shift).max((1, 2))[:, None]
        if origin is None:
            origin = aim + g.normal(size=(m, 3)) * S * 10.0 ** g.integers(-2, 2, (m, 1))
        o = origin.astype(F32)
        scale = 10.0 ** g.integers(-2, 3, (m, 1))                                               # t = 1 / scale at the aim
        d = ((aim.astype(F32) - o).astype(F32) * scale.astype(F32)).astype(F32)
        t_max = np.where(g.random(m) < 0.5, np.inf, 2.0 / scale[:, 0])
        return o, d, np.where(g.random(m) < 0.3, -1.0, 0.0).astype(F32), t_max.astype(F32)

    tri = ((g.random((n, 3, 3)) * 2 - 1) * 10.0 ** g.integers(-3, 4, (n, 1, 1))).astype(F32)
    out["tight"] = aimed(tri) + (tri,) + _tight(tri)
    S = np.abs(tri).max((1, 2))[:, None]
    grow = (g.random((2, n, 3)) * S).astype(F32)
    out["larger box"] = aimed(tri) + (tri, (tri.min(1) - grow[0]).astype(F32), (tri.max(1) + grow[1]).astype(F32))

    def flat(shift=(0.0, 0.0, 0.0)):
        t = g.random((n, 3, 3)) * 2 - 1
        axis = g.integers(0, 3, n)
        t[np.arange(n), :, axis] = (g.random(n) * 2 - 1)[:, None]
        return (t + np.asarray(shift)).astype(F32), axis
    tf, axis = flat()
    out["flat"] = aimed(tf) + (tf,) + _tight(tf)
    ts, _ = flat((100.0, -50.0, 25.0))
    out["flat, shifted"] = aimed(ts, shift=np.array([100.0, -50.0, 25.0])) + (ts,) + _tight(ts)
    # axis-aligned rays onto flat triangles: two zero components, the hit in a box without thickness
    w = g.dirichlet(np.ones(3), n)
    hitp = (w[:, :, None] * tf.astype(np.float64)).sum(1).astype(F32)
    dd = np.zeros((n, 3), F32)
    dd[np.arange(n), axis] = g.choice([-1.0, 1.0], n) * (0.25 + g.random(n))
    oo = (hitp - dd * F32(2)).astype(F32)
    out["flat, axis-aligned rays"] = (oo, dd, np.zeros(n, F32), np.full(n, np.inf, F32), tf) + _tight(tf)
    # origins inside the box
    lo, hi = _tight(tri)
    inside = lo + (hi - lo) * g.random((n, 3)).astype(F32)
    out["origin inside the box"] = aimed(tri, origin=np.clip(inside, lo, hi).astype(np.float64)) + (tri, lo, hi)
    # rays inside a box face, one zero component: through the vertex that makes the face
    face_axis = g.integers(0, 3, n)
    vert = tri[np.arange(n), tri[np.arange(n), :, face_axis].argmin(1)]
    offs = (g.normal(size=(n, 3)) * np.abs(tri).max((1, 2))[:, None]).astype(F32)
    offs[np.arange(n), face_axis] = 0
    of = (vert + offs).astype(F32)
    of[np.arange(n), face_axis] = vert[np.arange(n), face_axis]
    df = (vert - of).astype(F32)
    out["in a box face"] = (of, df, np.zeros(n, F32), np.full(n, np.inf, F32), tri, lo, hi)
    shift = np.array([100.0, -50.0, 25.0])
    small = np.abs(tri).max((1, 2)) <= 10
    tsh = (tri[small] + shift).astype(F32)
    out["shifted"] = aimed(tsh, shift=shift) + (tsh,) + _tight(tsh)
    a = (g.random((n, 3)) * 2 - 1).astype(F32)
    pt = np.stack([a, a, a], 1)
    out["a point"] = aimed(pt) + (pt,) + _tight(pt)
    return out


FLAT = ("flat", "flat, shifted", "flat, axis-aligned rays")
