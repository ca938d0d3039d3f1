"""Simplify a triangle mesh on the device by vertex clustering (include/lara_meshsimplify.h,
csrc/meshsimplify.hip); opt-in like every module here.  The last stage of the mesh path: it reads (vertices, triangles, colors)
as ``lara_amd.mesh.clean_mesh`` returns them and returns the same triple.

  * ``simplify_vertex_clustering``  one cluster per occupied cell of a grid of pitch ``voxel_size``; the cluster's vertex is the
                                    mean of its members (``"average"``) or the minimiser of the area-weighted plane quadric of
                                    the triangles around them, regularised towards the mean and clamped to the cell
                                    (``"quadric"``); triangles are re-indexed, collapsed and repeated ones dropped;
  * ``simplify_to``                 a geometric bisection on ``voxel_size`` for a triangle budget; the probes only count.

The semantics are those of Open3D's ``simplify_vertex_clustering`` [RECALLED]; Open3D is absent, so parity with it is unpinned:
the contract is the header's, restated in numpy by tests/meshsimplify_restate.py.  Results are bit-reproducible (integer atomics
only; per-cluster double sums in a fixed order over ascending members).  No CPU path: tensors must live on the GPU."""
from __future__ import annotations

import numpy as np
import torch

from ._native import alloc_bytes, call, query, require_device
from .mesh import _compact

ERR_INDEX, ERR_PROBE, ERR_NONFINITE, ERR_NEGATIVE, ERR_EXTENT = 1, 2, 4, 8, 16      # include/lara_meshsimplify.h
MAX_CELL = 1 << 21
N_DEGENERATE, N_DUPLICATE, N_ZERO_AREA, N_CLAMPED, COUNTERS = 0, 1, 2, 3, 4
CONTRACTIONS = ("average", "quadric")


def _raise_on(err_word):
    what = "lara_amd.meshsimplify"
    if err_word & ERR_NONFINITE:
        raise RuntimeError(f"{what}: a vertex is not finite")
    if err_word & ERR_NEGATIVE:
        raise RuntimeError(f"{what}: a vertex lies below the origin (negative cell index)")
    if err_word & ERR_EXTENT:
        raise RuntimeError(f"{what}: voxel_size too small for this extent (a cell index reaches 2^21)")
    if err_word & ERR_INDEX:
        raise RuntimeError(f"{what}: a triangle indexes a vertex outside [0, Nv)")
    if err_word & ERR_PROBE:
        raise RuntimeError(f"{what}: internal error (a hash table ran full)")


def _inputs(vertices, triangles, colors):
    require_device(vertices)
    dev = vertices.device
    V = vertices.detach().to(torch.float32).contiguous()
    if V.dim() != 2 or V.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError("lara_amd.meshsimplify: expected vertices [Nv,3] and triangles [T,3]")
    if V.shape[0] >= 2 ** 31 or 3 * triangles.shape[0] >= 2 ** 31:
        raise RuntimeError("lara_amd.meshsimplify: meshes need Nv < 2^31 and 3 T < 2^31 (int32 indices)")
    F = triangles.to(device=dev, dtype=torch.int32).contiguous()
    C = None if colors is None else colors.detach().to(device=dev, dtype=torch.float32).contiguous()
    if C is not None and C.shape != V.shape:
        raise RuntimeError("lara_amd.meshsimplify: expected colors [Nv,3]")
    return dev, V, F, C


def _pitch(voxel_size):
    h32 = float(np.float32(voxel_size))
    if not (h32 > 0.0 and np.isfinite(h32)):
        raise ValueError(f"lara_amd.meshsimplify: voxel_size must be a positive finite fp32 number, got {voxel_size!r}")
    return h32


def _origin(V, h32, origin):
    """[3] fp32 on the device: the caller's, or min over the vertices - 0.5f h (fp32; no host read)."""
    if origin is not None:
        return torch.as_tensor(origin, dtype=torch.float64).reshape(3).to(device=V.device, dtype=torch.float32).contiguous()
    return (V.amin(0) - 0.5 * h32).contiguous()          # 0.5 h is exact; one fp32 rounding in the subtraction


class _Stages:
    """Optional HIP-event bracketing of the stages (tools/meshsimplify_bench.py): ``marks`` collects (name, event)."""

    def __init__(self, marks):
        self.marks = marks

    def __call__(self, name):
        if self.marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.marks.append((name, e))


def _cluster_and_count(dev, V, F, h32, org, mark):
    """The integer part: cells, clusters, triangle survival.  One host read for n_cells, one for the output sizes.
    Returns a dict of device tensors and sizes."""
    Nv, T = V.shape[0], F.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    err = torch.zeros(1, **i32)
    counters = torch.zeros(COUNTERS, **i32)
    slot = torch.empty(Nv, **i32)
    is_leader = torch.empty(Nv, **i32)
    ws = alloc_bytes(query("lara_meshsimplify_cells_workspace_bytes", Nv), dev)
    call("lara_meshsimplify_cells", dev, Nv, V, h32, org, slot, is_leader, ws, err)
    leader_ends = torch.cumsum(is_leader, 0, dtype=torch.int64)
    n_cells, e = torch.stack([leader_ends[-1], err[0].long()]).tolist()              # host read: the number of clusters
    _raise_on(e)
    vc = torch.empty(Nv, **i32)
    leader_vertex = torch.empty(n_cells, **i32)
    call("lara_meshsimplify_clusters", dev, Nv, slot, leader_ends, ws, vc, leader_vertex)
    del ws, slot, is_leader, leader_ends
    mark("cells and clusters")
    mapped = torch.empty(T, 3, **i32)
    keep = torch.empty(T, **i32)
    referenced = torch.zeros(n_cells, **i32)
    if T:
        tws = alloc_bytes(query("lara_meshsimplify_triangles_workspace_bytes", T), dev)
        call("lara_meshsimplify_triangles", dev, Nv, T, n_cells, F, vc, mapped, keep, referenced, counters, tws, err)
        del tws
    tends = torch.cumsum(keep, 0, dtype=torch.int64)
    T2, e = torch.stack([tends[-1], err[0].long()]).tolist() if T else (0, 0)        # host read: the surviving triangles
    _raise_on(e)
    mark("triangles")
    return dict(n_cells=n_cells, vc=vc, leader_vertex=leader_vertex, mapped=mapped, keep=keep, tends=tends, T2=T2,
                referenced=referenced, counters=counters, err=err)


def _empty(dev, V, C, Nv):
    info = {"vertex_cluster": torch.full((Nv,), -1, dtype=torch.int32, device=dev), "n_cells": 0, "n_degenerate": 0,
            "n_duplicate": 0, "n_clamped": 0, "n_zero_area": 0}
    return V[:0].clone(), torch.zeros(0, 3, dtype=torch.int64, device=dev), None if C is None else C[:0].clone(), info


def _bucket(dev, key, n_keys):
    """(ends [n_keys] int64, items int32): the items of every key in ascending order (lara_meshsimplify_bucket_*)."""
    n = key.numel()
    count = torch.empty(n_keys, dtype=torch.int32, device=dev)
    call("lara_meshsimplify_bucket_count", dev, n, n_keys, key, count)
    ends = torch.cumsum(count, 0, dtype=torch.int64)
    items = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ws = alloc_bytes(max(256, query("lara_meshsimplify_bucket_workspace_bytes", n, n_keys)), dev)
    call("lara_meshsimplify_bucket_fill", dev, n, n_keys, key, ends, items, ws)
    return ends, items


@torch.no_grad()
def simplify_vertex_clustering(vertices, triangles, colors=None, voxel_size=None, contraction="quadric", origin=None,
                               remove_unreferenced=True, *, _marks=None):
    """vertices [Nv,3] fp32 on the device, triangles [T,3] of any integer type, colors [Nv,3] or None.  Returns
    (vertices', triangles' int64, colors', info).

    Cells: ``h = float32(voxel_size)``, ``origin`` = the given 3 numbers or min over the vertices - h / 2 (fp32),
    ``cell = floorf((v - origin) / h)`` in fp32.  One output vertex per occupied cell, numbered by ascending smallest member.
    ``"average"``: the fp64 mean of the members, rounded to fp32.  ``"quadric"``: with A = sum w n n^T and
    b = sum w (n . (p0 - m)) n over the corners of the cluster (w = the triangle's area, n its unit normal, in fp64),
    x = m + (A + 2^-10 tr(A) I)^-1 b clamped to the cell's box; m where tr(A) = 0.  Colours are the members' mean.
    Triangles: corners -> clusters; a triangle with two equal corners is dropped; of equal oriented triples (smallest id first)
    the lowest original index stays; order is kept.  ``remove_unreferenced``: clusters no surviving triangle uses are dropped.

    ``info``: ``vertex_cluster`` [Nv] int32 (the output vertex of every input vertex, -1 if removed), ``n_cells``,
    ``n_degenerate``, ``n_duplicate``, ``n_zero_area`` (input triangles without a finite non-zero area), ``n_clamped`` (output
    vertices a clamp moved).  Raises RuntimeError for a non-finite vertex, a vertex below a given origin, a voxel_size so
    small that a cell index reaches 2^21, and a triangle index outside [0, Nv).  Everything stays on the device; the host
    reads sizes, counters and the error word."""
    if contraction not in CONTRACTIONS:
        raise ValueError(f"lara_amd.meshsimplify: contraction must be one of {CONTRACTIONS}, got {contraction!r}")
    if voxel_size is None:
        raise ValueError("lara_amd.meshsimplify: voxel_size is required")
    dev, V, F, C = _inputs(vertices, triangles, colors)
    h32 = _pitch(voxel_size)
    Nv, T = V.shape[0], F.shape[0]
    if Nv == 0:
        if T:
            raise RuntimeError("lara_amd.meshsimplify: a triangle indexes a vertex outside [0, Nv)")
        return _empty(dev, V, C, 0)
    quadric = int(contraction == "quadric")
    mark = _Stages(_marks)
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        mark("start")
        org = _origin(V, h32, origin)
        s = _cluster_and_count(dev, V, F, h32, org, mark)
        n_cells, vc, referenced, counters = s["n_cells"], s["vc"], s["referenced"], s["counters"]
        if not remove_unreferenced:
            referenced = torch.ones(n_cells, **i32)
        # buckets and sums
        vends, vitems = _bucket(dev, vc, n_cells)
        ckey = torch.empty(3 * T, **i32)
        call("lara_meshsimplify_corner_keys", dev, Nv, T, V, F, vc, ckey, counters)
        if quadric:
            cends, citems = _bucket(dev, ckey, n_cells)
            Ab = torch.empty(n_cells, 9, dtype=torch.float64, device=dev)
        else:
            cends = citems = Ab = None
        mean = torch.empty(n_cells, 3, dtype=torch.float64, device=dev)
        colors_all = None if C is None else torch.empty(n_cells, 3, dtype=torch.float32, device=dev)
        call("lara_meshsimplify_sums", dev, Nv, T, n_cells, V, C, F, vends, vitems, cends, citems, quadric, mean, colors_all, Ab)
        mark("bucket and sums")
        pos_all = torch.empty(n_cells, 3, dtype=torch.float32, device=dev)
        call("lara_meshsimplify_solve", dev, Nv, n_cells, quadric, mean, Ab, V, s["leader_vertex"], h32, org, referenced, pos_all,
             counters)
        mark("solve")
        # compaction
        gends = torch.cumsum(referenced, 0, dtype=torch.int64)
        sizes = torch.cat([gends[-1:], counters.long(), s["err"].long()]).tolist()     # host read: the output size, the counters
        Nv2, e = sizes[0], sizes[-1]
        _raise_on(e)
        F2 = _compact(s["mapped"], s["keep"], s["tends"], s["T2"])
        out_t = torch.empty_like(F2)
        call("lara_mesh_remap", dev, n_cells, s["T2"], F2, gends, out_t, s["err"])
        V2 = _compact(pos_all, referenced, gends, Nv2)
        C2 = None if C is None else _compact(colors_all, referenced, gends, Nv2)
        vmap = torch.empty(Nv, **i32)
        call("lara_meshsimplify_vertex_map", dev, Nv, n_cells, vc, referenced, gends, vmap)
        mark("compaction")
    info = {"vertex_cluster": vmap, "n_cells": n_cells, "n_degenerate": sizes[1 + N_DEGENERATE], "n_duplicate": sizes[1 + N_DUPLICATE],
            "n_clamped": sizes[1 + N_CLAMPED], "n_zero_area": sizes[1 + N_ZERO_AREA], "voxel_size": h32}
    return V2, out_t.long(), C2, info


@torch.no_grad()
def count_triangles(vertices, triangles, voxel_size, origin=None):
    """The number of triangles ``simplify_vertex_clustering`` would return at ``voxel_size``: cells, clusters and triangle
    survival only, no placement (the probe of ``simplify_to``)."""
    dev, V, F, _ = _inputs(vertices, triangles, None)
    h32 = _pitch(voxel_size)
    if V.shape[0] == 0 or F.shape[0] == 0:
        if F.shape[0]:
            raise RuntimeError("lara_amd.meshsimplify: a triangle indexes a vertex outside [0, Nv)")
        return 0
    with torch.cuda.device(dev):
        return _cluster_and_count(dev, V, F, h32, _origin(V, h32, origin), _Stages(None))["T2"]


@torch.no_grad()
def simplify_to(vertices, triangles, colors=None, target_triangles=None, contraction="quadric", max_probes=12):
    """The finest clustering found with at most ``target_triangles`` triangles: a geometric bisection on the voxel size
    between diag 2^-20 and diag, the bounding box's diagonal.  The first probe is diag itself (the coarsest grid; should even
    that leave more than the target, RuntimeError), every further one the geometric mean of the bracket; each is a count-only
    pass.  Returns ``simplify_vertex_clustering`` at the finest probed size whose count fits, with ``info["probes"]`` =
    [(voxel_size, count), ...] in probing order.  A mesh that already fits is returned as a copy (``info["probes"]`` = [])."""
    if target_triangles is None or int(target_triangles) < 0:
        raise ValueError("lara_amd.meshsimplify: target_triangles must be a non-negative integer")
    if contraction not in CONTRACTIONS:
        raise ValueError(f"lara_amd.meshsimplify: contraction must be one of {CONTRACTIONS}, got {contraction!r}")
    N = int(target_triangles)
    dev, V, F, C = _inputs(vertices, triangles, colors)
    if F.shape[0] <= N:
        info = {"vertex_cluster": torch.arange(V.shape[0], dtype=torch.int32, device=dev), "n_cells": None, "n_degenerate": 0,
                "n_duplicate": 0, "n_clamped": 0, "n_zero_area": None, "voxel_size": None, "probes": []}
        return V.clone(), F.long(), None if C is None else C.clone(), info
    lo_hi = torch.stack([V.amin(0), V.amax(0)]).double().cpu().numpy()                # host read: the bounding box
    diag = float(np.linalg.norm(lo_hi[1] - lo_hi[0]))
    if not (diag > 0.0 and np.isfinite(diag)):
        raise RuntimeError("lara_amd.meshsimplify: the mesh has no finite extent")
    probes = []

    def probe(h):
        h = _pitch(h)
        n = count_triangles(V, F, h)
        probes.append((h, n))
        return h, n

    best, n = probe(diag)
    if n > N:
        raise RuntimeError(f"lara_amd.meshsimplify: the coarsest grid leaves {n} triangles, more than the target {N}")
    lo, hi = diag * 2.0 ** -20, best
    for _ in range(max(0, int(max_probes) - 1)):
        h, n = probe((lo * hi) ** 0.5)
        if n <= N:
            best = hi = h
        else:
            lo = h
    V2, F2, C2, info = simplify_vertex_clustering(V, F, C, best, contraction)
    info["probes"] = probes
    return V2, F2, C2, info
