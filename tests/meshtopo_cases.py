"""The meshes tests/test_meshtopo.py runs through the host entries and tests/test_meshtopo_gpu.py through the kernels, each held to
tests/meshtopo_restate.py.  The generators are the suite's own (tests/meshdist_restate.py, tests/meshmetrics_restate.py,
tests/meshdist_cases.py).  Every case exists twice: as built, and as ``<name>/permuted`` with its triangles in a seeded random order.
``case(key)`` computes a case's restatement once and keeps it; nothing changes it afterwards."""
import functools

import numpy as np

from tests import meshdist_cases as DC
from tests import meshdist_restate as R
from tests import meshmetrics_restate as MR
from tests import meshtopo_restate as S

F32 = np.float32


def icosphere():
    return R.icosphere(3)                                   # 642 vertices, 1 280 faces


def uv_sphere():
    return MR.uv_sphere(8, 64)                              # 450 vertices, 896 faces, the poles have degree 64


def face_removed():
    V, F = icosphere()
    return V, F[1:]


def face_flipped():
    V, F = icosphere()
    F = F.copy()
    F[7] = F[7, ::-1]
    return V, F


def extra_triangles():
    """Two more triangles on the edge (a, b) of face 0, each with a vertex of its own: that edge has four faces, no other edge more
    than two."""
    V, F = icosphere()
    a, b = F[0, 0], F[0, 1]
    extra = (V[a] + V[b])[None] * np.array([[0.7], [0.9]], F32)
    return np.concatenate([V, extra.astype(F32)]), np.concatenate([F, [[a, b, len(V)], [b, a, len(V) + 1]]])


def unreferenced():
    V, F = icosphere()
    return np.concatenate([V, np.random.default_rng(3).random((5, 3)).astype(F32)]), F


def degenerate():
    return DC.case_degenerate()[1:]


def bad_triangles():
    return DC.case_bad_triangles()[1:]


def copies_4096():
    V = np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.6]], F32)
    return V, np.tile(np.array([[0, 1, 2]], np.int64), (4096, 1))


def fan_300():
    return R.fan(300)                                       # vertex 0 has 300 neighbours and 300 faces: a row longer than a workgroup


def soup_257():
    return DC.soup(257, 31)                                 # Nv = 771, no shared vertex


def one_triangle():
    return np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], F32), np.array([[0, 1, 2]], np.int64)


def no_triangle():
    return np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], F32), np.zeros((0, 3), np.int64)


BASE = {"icosphere": icosphere, "uv_sphere": uv_sphere, "face_removed": face_removed, "face_flipped": face_flipped,
        "extra_triangles": extra_triangles, "unreferenced": unreferenced, "degenerate": degenerate, "bad_triangles": bad_triangles,
        "copies_4096": copies_4096, "fan_300": fan_300, "soup_257": soup_257, "one_triangle": one_triangle, "no_triangle": no_triangle}
CASES = sorted(list(BASE) + [k + "/permuted" for k in BASE])
RAISES = ("bad_triangles", "bad_triangles/permuted")         # an index outside [0, Nv): python raises
STEPS = {"pass": [0.5], "pass_mu": [-0.53], "laplacian_3": [0.5] * 3, "taubin_10": [0.5, -0.53] * 10}


def mesh(key):
    name, _, permuted = key.partition("/")
    V, F = BASE[name]()
    V, F = np.ascontiguousarray(V, F32), np.asarray(F, np.int64).reshape(-1, 3)
    if permuted:
        F = F[np.random.default_rng(len(F) + 17).permutation(len(F))]
    return V, np.ascontiguousarray(F)


@functools.lru_cache(maxsize=None)
def case(key):
    """{"V", "F", "topo" (the restated edge table), "report", "vv", "vf" (the CSR tables), "normals" {weighting: (normals, zero
    count)}, "smooth" {(name of STEPS, fix_boundary): positions}} of one case.  A case that raises in python still has its restated
    tables, over its sound triangles: the host entries are compared on them."""
    V, F = mesh(key)
    topo = S.Topology(len(V), F)
    vv, vf = topo.vertex_neighbors(), topo.vertex_faces()
    out = {"V": V, "F": F, "topo": topo, "report": topo.report(), "vv": vv, "vf": vf}
    out["normals"] = {w: S.vertex_normals(V, F, vf[0], vf[1], w) for w in (S.AREA, S.UNIFORM)}
    out["smooth"] = {(name, fix): S.smooth(V, topo, steps, fix) for name, steps in STEPS.items() for fix in (False, True)}
    return out


def noisy_icosphere():
    """The icosphere with radial noise, the input of the smoothing teeth."""
    V, F = icosphere()
    return (V * (1 + 0.02 * np.random.default_rng(5).standard_normal((len(V), 1)))).astype(F32), F
