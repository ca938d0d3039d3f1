"""Times `lara_amd.meshtopo` on one MI355X: HIP events after warm-up, the UV sphere of 556 516 triangles of the neighbouring benches
(tools/meshbvh_bench.py, tools/meshsign_bench.py).  Nothing in this package built an edge table, a vertex normal or a smoothing pass
before, so no time is gated and there is no baseline; the torch rows give context only.

  * the build of `MeshTopology` (with its one host read), and inside it the stable sort of the 3 T half-edge keys alone;
  * the two CSR tables (a sort each);
  * `report_row` (the device part of `report`) and `report(components=True)` with `meshclean`'s labelling;
  * `vertex_normals` for both weightings;
  * one smoothing pass and 10 Taubin iterations (20 passes);
  * the `extract`-style use: the build, 10 Taubin iterations and the normals of the result, from two tensors to two tensors;
  * context: the same area-weighted normals and the same pass written in torch operators (`index_add_`, float64);
  * the same pass and normals on a sphere of as many triangles whose poles have half the degree: the longest CSR row is walked by one
    thread, and this row shows what it costs;
  * the algorithmic bytes of a pass -- the own position, the gathered neighbours with their indices, an offset, the result -- over
    its time, as a fraction of the device-to-device copy rate measured beside it.

Every figure is the mean of --steps runs in ONE process run: no spread is measured.  Nothing is read from outside the repository.
    python tools/meshtopo_bench.py [--steps 20] [--warmup 3] [--quick] [--out profiles/meshtopo_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402


def torch_normals(V, F):
    """Area-weighted vertex normals in torch operators: float64 cross products scattered with index_add_ (its order is not fixed)."""
    P = V.double()
    c = torch.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]], dim=1)
    s = torch.zeros_like(P)
    for k in range(3):
        s.index_add_(0, F[:, k], c)
    return (s / s.norm(dim=1, keepdim=True)).float()


def torch_pass(V, src, dst, degree, s):
    """One smoothing pass in torch operators over the directed pairs (src -> dst) of the unique edges."""
    P = V.double()
    m = torch.zeros_like(P).index_add_(0, src, P[dst]) / degree[:, None]
    return (P + s * (m - P)).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a small sphere, one step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshtopo_bench: needs an MI355X")
    from lara_amd import _native, meshtopo
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V, F, V2 = sphere_pair(n_lat, n_lon, dev)
    Nv, T = int(V.shape[0]), int(F.shape[0])
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    topo = meshtopo.MeshTopology(V2, F)
    rep = topo.report(components=True)
    E = topo.n_edges
    res = {"Nv": Nv, "T": T, "E": E, "steps": steps, "warmup": warmup, "one_run": True, "copy_rate_GBps": rate / 1e9,
           "report": {k: rep[k] for k in ("euler", "is_closed", "is_oriented", "n_boundary", "n_nonmanifold", "max_degree", "n_components",
                                          "genus")}}
    # the build and its sort
    keys = torch.empty(3 * T, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.call("lara_meshtopo_halfedge_keys", dev, Nv, T, topo.triangles, keys, err)
    res["build_ms"] = timed(lambda: meshtopo.MeshTopology(V2, F), steps, warmup)
    res["build_sort_ms"] = timed(lambda: torch.sort(keys, stable=True), steps, warmup)
    res["build_sort_share"] = res["build_sort_ms"] / res["build_ms"]

    def fresh(table):
        topo._neighbors = topo._faces = None
        return getattr(topo, table)()
    res["vertex_neighbors_ms"] = timed(lambda: fresh("vertex_neighbors"), steps, warmup)
    res["vertex_faces_ms"] = timed(lambda: fresh("vertex_faces"), steps, warmup)
    topo.vertex_neighbors(), topo.vertex_faces(), topo.boundary_vertices()
    res["report_row_ms"] = timed(topo.report_row, steps, warmup)
    res["components_ms"] = timed(topo.n_components, max(1, steps // 4), 1)
    # the per-vertex kernels
    res["normals_area_ms"] = timed(lambda: topo.vertex_normals("area"), steps, warmup)
    res["normals_uniform_ms"] = timed(lambda: topo.vertex_normals("uniform"), steps, warmup)
    res["smooth_pass_ms"] = timed(lambda: topo.smooth_laplacian(1), steps, warmup)
    res["smooth_pass_fix_boundary_ms"] = timed(lambda: topo.smooth_laplacian(1, fix_boundary=True), steps, warmup)
    res["taubin_10_ms"] = timed(lambda: topo.smooth_taubin(10), steps, warmup)
    # what binds a pass: the same kernel on a sphere of as many triangles whose poles have half the degree
    _, F3, V3 = sphere_pair(n_lon, n_lat // 2 * 2, dev)
    other = meshtopo.MeshTopology(V3, F3)
    other.vertex_neighbors(), other.vertex_faces()
    res["half_pole"] = {"T": int(F3.shape[0]), "max_degree": other.report()["max_degree"],
                        "smooth_pass_ms": timed(lambda: other.smooth_laplacian(1), steps, warmup),
                        "normals_area_ms": timed(lambda: other.vertex_normals("area"), steps, warmup)}
    res["pass_bytes"] = Nv * 12 + 2 * E * 16 + Nv * 8 + Nv * 12
    res["pass_in_taubin_ms"] = res["taubin_10_ms"] / 20
    res["pass_fraction_of_copy_rate"] = res["pass_bytes"] / (res["pass_in_taubin_ms"] * 1e-3) / rate
    res["normals_bytes"] = 3 * T * (8 + 12 + 36) + Nv * 8 + Nv * 12
    res["normals_fraction_of_copy_rate"] = res["normals_bytes"] / (res["normals_area_ms"] * 1e-3) / rate

    def whole():
        t = meshtopo.MeshTopology(V2, F)
        return t.vertex_normals(vertices=t.smooth_taubin(10))
    res["extract_style_ms"] = timed(whole, max(1, steps // 2), 1)
    smoothed = topo.smooth_taubin(10)
    radii = lambda X: float(X.double().norm(dim=1).std())
    res["radii_spread"] = {"input": radii(V2), "taubin_10": radii(smoothed), "laplacian_10": radii(topo.smooth_laplacian(10))}
    # context rows, not baselines
    offsets, neighbors = topo.vertex_neighbors()
    degree = (offsets[1:] - offsets[:-1]).double()
    src = torch.repeat_interleave(torch.arange(Nv, device=dev), offsets[1:] - offsets[:-1])
    dst = neighbors.long()
    tn, kn = torch_normals(V2, F), topo.vertex_normals("area")
    tp, kp = torch_pass(V2, src, dst, degree, 0.5), topo.smooth_laplacian(1)
    res["context_torch"] = {"normals_ms": timed(lambda: torch_normals(V2, F), steps, warmup),
                            "normals_max_abs_difference": float((tn - kn).abs().max()),
                            "pass_ms": timed(lambda: torch_pass(V2, src, dst, degree, 0.5), steps, warmup),
                            "pass_max_abs_difference": float((tp - kp).abs().max())}

    def rounded(x):
        if isinstance(x, float):
            return float(f"{x:.6g}")
        if isinstance(x, dict):
            return {k: rounded(v) for k, v in x.items()}
        return x
    line = json.dumps(rounded(res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
