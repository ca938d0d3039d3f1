"""The cases of the mesh rasteriser's tests (no GPU): each at most 64 x 64 pixels, 3 views and a few thousand triangles.

A case is a dict: name, H, W, cams (``lara_amd.cameras`` cameras on the CPU), eyes [n,3] (the cameras' positions), vertices
[Nv,3] fp32, triangles [T,3] int64, colors [Nv,3] fp32 or None, znear, chunk, zero_excluded (no near-tie may be excluded), and
``expect``: what the case asserts beyond the restatement.

The flat cases use the pinhole at the origin looking down +z with tan(fov / 2) = 1/2 and put their vertices on the plane
z = 2, where a vertex meant for pixel (px, py) of a power-of-two image is x = (2 px + 1) / W - 1: every step of stage V is
then exact in fp32 and the vertex lands on px exactly (multiples of 1/256 pixel included)."""
import math

import numpy as np
import torch

from lara_amd import cameras

FOV_HALF = 2.0 * math.atan(0.5)


def flat_camera(W, H):
    return cameras.make_cameras(torch.eye(4)[None], W, H, FOV_HALF, FOV_HALF, 0.5, 10.0), np.zeros((1, 3), np.float32)


def flat_vertex(px, py, W, H, z=2.0):
    """The point of the plane z that projects to pixel (px, py) (exactly, for z = 2 and power-of-two sides)."""
    return [((2.0 * px + 1.0) / W - 1.0) * z / 2.0, ((2.0 * py + 1.0) / H - 1.0) * z / 2.0, z]


def orbit_cameras(n, W, H, fovx=0.75, fovy=0.75):
    c2w = cameras.turntable_c2w(n)
    return cameras.make_cameras(c2w, W, H, fovx, fovy, 0.5, 2.5), c2w[:, :3, 3].numpy().astype(np.float32)


def icosphere(subdivisions, radius=0.5):
    """(vertices fp32, triangles int64): 20 x 4^subdivisions triangles, outward winding."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    v = [tuple(np.asarray(p, np.float64) / np.linalg.norm(p)) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = (np.asarray(v[a]) + np.asarray(v[b])) / 2.0
                v.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v, np.float64) * radius).astype(np.float32), np.asarray(f, np.int64)


def _case(name, H, W, cams_eyes, vertices, triangles, colors=None, chunk=8, zero_excluded=False, **expect):
    cams, eyes = cams_eyes
    return {"name": name, "H": H, "W": W, "cams": cams, "eyes": eyes, "vertices": np.asarray(vertices, np.float32).reshape(-1, 3),
            "triangles": np.asarray(triangles, np.int64).reshape(-1, 3), "colors": colors, "znear": float(cams[0].znear),
            "chunk": chunk, "zero_excluded": zero_excluded, "expect": expect}


def case_a():
    """One triangle, vertices on sample points (0,0), (4,0), (0,4) plus the offset (2,2): its legs are a top and a left edge
    (they own their samples), the hypotenuse runs through sample points it does not own."""
    W = H = 16
    v = [flat_vertex(2, 2, W, H), flat_vertex(6, 2, W, H), flat_vertex(2, 6, W, H)]
    covered = sorted((2 + x, 2 + y) for y in range(4) for x in range(4 - y))       # x, y >= 0 and x + y < 4: ten samples
    return _case("a_fill_rule", H, W, flat_camera(W, H), v, [[0, 1, 2]], zero_excluded=True, covered=covered)


def case_b():
    """A fan around (16, 16) whose rim lies on sample points and on 1/256-pixel positions, and a strip below it sharing the
    fan's bottom edge: every sample under the union is covered exactly once."""
    W = H = 32
    rim = [(26, 16), (24.5, 22.25), (16, 26), (9 + 3 / 256, 23), (6, 16), (8, 8.5), (16, 6), (23.75, 9 + 129 / 256)]
    v = [flat_vertex(16, 16, W, H)] + [flat_vertex(x, y, W, H) for x, y in rim]
    t = [[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)]
    # the strip: the fan's edge (24.5, 22.25) - (16, 26) and three more vertices further down
    base = len(v)
    v += [flat_vertex(27, 29.5, W, H), flat_vertex(18, 30, W, H), flat_vertex(10, 29, W, H)]
    t += [[2, base, 3], [3, base, base + 1], [3, base + 1, base + 2], [3, base + 2, 4]]
    return _case("b_fan_and_strip", H, W, flat_camera(W, H), v, t, zero_excluded=True, exactly_once=True)


def case_c():
    v, t = icosphere(3)
    return _case("c_icosphere", 64, 64, orbit_cameras(3, 64, 64), v, t)


def case_d():
    vo, to = icosphere(2, 0.5)
    vi, ti = icosphere(2, 0.3)
    v, t = np.concatenate([vo, vi]), np.concatenate([to, ti + len(vo)])
    rng = np.random.default_rng(5)
    colors = rng.uniform(0.1, 1.0, (len(v), 3)).astype(np.float32)
    return _case("d_nested", 48, 48, orbit_cameras(2, 48, 48), v, t, colors=colors, outer_only=len(to))


def case_e():
    """Two coincident quads (separate vertices at the same positions, the same order): the tie goes to the lower id."""
    W = H = 16
    q = [flat_vertex(3, 3, W, H), flat_vertex(12.5, 3, W, H), flat_vertex(12.5, 11, W, H), flat_vertex(3, 11, W, H)]
    # the second quad comes FIRST in the triangle list's id order only for its second triangle: ids 0, 3 belong to one copy
    t = [[0, 1, 2], [4, 6, 7], [4, 5, 6], [0, 2, 3]]
    return _case("e_coincident", H, W, flat_camera(W, H), q + q, t, zero_excluded=True, faces={0, 1})


def case_f():
    """One triangle covering the whole image and, behind it, one far larger: clamped boxes of the full image, the
    wave-per-triangle shape."""
    W = H = 16
    v = [flat_vertex(-2, -2, W, H), flat_vertex(40, -2, W, H), flat_vertex(-2, 40, W, H),
         flat_vertex(-500, -300, W, H, 3.0), flat_vertex(900, -300, W, H, 3.0), flat_vertex(-500, 1200, W, H, 3.0)]
    return _case("f_whole_image", H, W, flat_camera(W, H), v, [[3, 4, 5], [0, 1, 2]], zero_excluded=True, faces={1})


def case_h():
    """A quad, plus one triangle with a vertex behind znear, one degenerate triangle and one with a vertex projected beyond
    the coordinate range: three dropped, two drawn, the image that of the quad alone."""
    W = H = 32
    v = [flat_vertex(4, 4, W, H), flat_vertex(20, 5, W, H), flat_vertex(21, 22, W, H), flat_vertex(5, 20, W, H),
         [0.0, 0.0, 0.1],                                   # behind znear = 0.5
         flat_vertex(10, 10, W, H, 1.5), flat_vertex(14, 14, W, H, 1.5), flat_vertex(18, 18, W, H, 1.5),      # collinear
         [5000.0, 0.0, 2.0]]                                # pixel 80 000: beyond 2^22 / 256 = 16 384
    t = [[0, 1, 2], [0, 4, 1], [5, 6, 7], [0, 2, 3], [1, 8, 2]]
    return _case("h_dropped", H, W, flat_camera(W, H), v, t, info=[2, 1, 1, 1], same_as=[[0, 1, 2], [0, 2, 3]], faces={0, 3})


def case_i():
    v, t = icosphere(2)
    return _case("i_37x29", 29, 37, orbit_cameras(2, 37, 29, 0.75, 0.6), v, t)


def case_j():
    v, _ = icosphere(0)
    return _case("j_no_triangles", 16, 16, orbit_cameras(1, 16, 16), v, np.zeros((0, 3), np.int64), zero_excluded=True, faces=set())


def case_k():
    v, t = icosphere(2)
    return _case("k_chunk_boundary", 32, 32, orbit_cameras(3, 32, 32), v, t, chunk=2)


CASES = {"a": case_a, "b": case_b, "c": case_c, "d": case_d, "e": case_e, "f": case_f, "h": case_h, "i": case_i, "j": case_j,
         "k": case_k}
# (g) is case (c) drawn with the area threshold's two sides forced: tests/test_meshrender_gpu.py


def matrices(case):
    """(view [n,16], proj [n,16]) fp32, as the library takes them."""
    view = np.stack([c.world_view_transform.cpu().numpy().reshape(16) for c in case["cams"]]).astype(np.float32)
    proj = np.stack([c.full_proj_transform.cpu().numpy().reshape(16) for c in case["cams"]]).astype(np.float32)
    return view, proj
