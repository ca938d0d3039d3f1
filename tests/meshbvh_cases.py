"""Meshes and (query, box) pairs tests/test_meshbvh.py and tests/test_meshbvh_gpu.py share, next to the cases of
tests/meshdist_cases.py.  Dyadic coordinates wherever a tie has to be exact."""
import numpy as np

F32 = np.float32


def mirror_pair(swap=False, padding=100):
    """Two mirror-image triangles at x = -1 and x = +1 and ``padding`` tiny ones whose Morton codes lie between theirs (x < 0,
    2 <= y < 4, z >= 0.75: farther than 1.8 from every query), plus one at y = 8 that stretches the box: the pair ends up in
    different level-1 nodes.  Every query on the plane x = 0 is exactly as far from the one as from the other.  Returns
    (Q, V, F, id of the triangle at x = -1, id of the one at x = +1): ids 0 and T - 1, or swapped."""
    g = np.random.default_rng(50)
    plus = np.array([[1, 0, 0], [1, 1, 0], [1, 0, 1]], np.float64)
    minus = plus * [-1, 1, 1]
    base = np.stack([-1 + g.integers(0, 32, padding) / 64.0, 2 + g.integers(0, 120, padding) / 64.0,
                     0.75 + g.integers(0, 15, padding) / 64.0], 1)
    pad = base[:, None, :] + np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]]) / 256.0
    far = np.array([[[0, 8, 0], [0.25, 8, 0], [0, 7.75, 0]]])
    first, last = (plus, minus) if swap else (minus, plus)
    tri = np.concatenate([first[None], pad, far, last[None]])
    T = len(tri)
    Q = np.array([[0, 0.25, 0.25], [0, 0.5, 0.25], [0, 0.125, 0.5], [0, -1, -1], [0, 0.75, 0.5], [0, 0, 2], [0, 0.75, 0.75],
                  [0, 0.5, 0.5], [0, 0.25, -3]], F32)
    ids = (T - 1, 0) if swap else (0, T - 1)
    return Q, tri.reshape(-1, 3).astype(F32), np.arange(3 * T, dtype=np.int64).reshape(T, 3), ids[0], ids[1]


def copies(n=4096):
    """``n`` copies of one triangle (a vertex list of their own each) and queries around it, the first ones ON it."""
    tri = np.array([[0.25, 0.5, 0.125], [1.0, 0.25, 0.5], [0.5, 1.0, 0.75]], F32)
    on = [tri[0], tri[1], tri[2], (tri[0] + tri[1]) / 2, (tri[1] + tri[2]) / 2, (tri[0] + tri[1]) / 4 + tri[2] / 2]
    Q = np.concatenate([np.array(on, F32), (np.random.default_rng(51).random((250, 3)) * 3 - 1).astype(F32)])
    return Q, np.tile(tri, (n, 1)), np.arange(3 * n, dtype=np.int64).reshape(n, 3), tri


def _tight(tri):
    return tri.min(1), tri.max(1)


def bound_pairs():
    """{name: (q [n,3], triangles [n,3,3], box lo [n,3], box hi [n,3])} fp32, the box holding the triangle's vertices: tight
    unless the name says "larger".  "flat ..." are the cases on which an unmargined float64 bound exceeds the computed d2."""
    g = np.random.default_rng(52)
    out = {}
    n = 20000
    tri = ((g.random((n, 3, 3)) * 2 - 1) * 10.0 ** g.integers(-3, 4, (n, 1, 1))).astype(F32)
    S = np.abs(tri).max((1, 2))[:, None].astype(np.float64)
    q = (tri.astype(np.float64).mean(1) + g.normal(size=(n, 3)) * S * 10.0 ** g.integers(-3, 2, (n, 1))).astype(F32)
    out["random"] = (q, tri) + _tight(tri)
    grow = (g.random((2, n, 3)) * S).astype(F32)
    out["random, larger box"] = (q, tri, (tri.min(1) - grow[0]).astype(F32), (tri.max(1) + grow[1]).astype(F32))

    def flat(height, shift=(0.0, 0.0, 0.0)):
        """Triangles in a plane of constant coordinate (each axis in turn), the query over the interior at ``height`` (None:
        random heights up to the triangle's size)."""
        t = g.random((n, 3, 3)) * 2 - 1
        axis = g.integers(0, 3, n)
        level = g.random(n) * 2 - 1
        t[np.arange(n), :, axis] = level[:, None]
        t = (t + np.asarray(shift)).astype(F32)
        b = g.dirichlet(np.ones(3), n)
        p = (b[:, :, None] * t.astype(np.float64)).sum(1)
        h = g.random(n) if height is None else np.full(n, height)
        p[np.arange(n), axis] = t[np.arange(n), 0, axis].astype(np.float64) + h * g.choice([-1.0, 1.0], n)
        return (p.astype(F32), t) + _tight(t)
    out["flat"] = flat(None)
    for h in (1e-3, 1e-6, 1e-9):
        out[f"flat, {h:g} above"] = flat(h)
    out["flat, shifted"] = flat(None, (100.0, -50.0, 25.0))
    out["flat, 1e-03 above, shifted"] = flat(1e-3, (100.0, -50.0, 25.0))
    q, tri, lo, hi = out["random"]
    shift = np.array([100.0, -50.0, 25.0])
    small = np.abs(tri).max((1, 2)) <= 10
    ts = (tri[small] + shift).astype(F32)
    out["random, shifted"] = ((q[small] + shift).astype(F32), ts) + _tight(ts)
    # queries on a face, an edge and a corner of the box (and inside it): the bound is 0 there
    m = 3000
    tri = (g.random((m, 3, 3)) * 2 - 1).astype(F32)
    lo, hi = _tight(tri)
    pick = g.integers(0, 3, (m, 3))          # per axis: the lower face, the upper face, or inside
    inside = (lo + (hi - lo) * g.random((m, 3)).astype(F32)).astype(F32)
    q = np.where(pick == 0, lo, np.where(pick == 1, hi, np.clip(inside, lo, hi))).astype(F32)
    out["on the box"] = (q, tri, lo, hi)
    # boxes without volume: a point (one vertex three times) and a segment (collinear, a vertex twice)
    a, b = (g.random((m, 3)) * 2 - 1).astype(F32), (g.random((m, 3)) * 2 - 1).astype(F32)
    q = (g.random((m, 3)) * 4 - 2).astype(F32)
    tri = np.stack([a, a, a], 1)
    out["a point"] = (q, tri) + _tight(tri)
    tri = np.stack([a, b, a], 1)
    out["a segment"] = (q, tri) + _tight(tri)
    ax = np.stack([a, a, a], 1)
    ax[:, 1, 0] = b[:, 0]                     # an axis-parallel segment: a box that is a segment
    out["an axis-parallel segment"] = (q, ax) + _tight(ax)
    return out


FLAT = ("flat", "flat, 0.001 above", "flat, 1e-06 above", "flat, 1e-09 above", "flat, shifted", "flat, 1e-03 above, shifted")
