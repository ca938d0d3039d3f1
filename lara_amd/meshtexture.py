"""A texture atlas for a mesh, baked on the device from the views that were rendered to build it
(include/lara_meshtexture.h, csrc/meshtexture.hip, csrc/texatlas.h); opt-in like every module here.  Per-vertex colours
carry a voxel's worth of appearance per vertex; once ``meshsimplify`` has run, a triangle spans many voxels and the surface between
its vertices is a blend of three colours.  The rendered views still hold the appearance at image resolution: this module writes it
into an atlas the simplified mesh carries along.

  * ``atlas``              the layout (S, C, Wa, Ha): every triangle gets the same S-texel patch, two triangles share a cell of
                           (S + 1) x S texels, C cells per row; closed-form and integer only, no unwrapping.  A bilinear read inside a
                           triangle's UV triangle touches only texels the triangle owns;
  * ``corner_uvs``         [T,3,2] fp32 texture coordinates of the corners, OBJ's convention (v points up);
  * ``texels``             per texel the owning face, its surface point and its anchor (the point pulled onto the triangle);
  * ``bake``               the atlas from ``images`` [V,H,W,3] and their cameras: per texel the views that see it
                           (``meshray.visibility`` on the anchors), face it (cos >= ``min_cos``) and hold all four bilinear taps are
                           blended with weight cos^power, or the best one is taken; a texel no view accepts falls back to the
                           barycentric blend of ``vertex_colors`` or to ``fill``, with alpha 0;
  * ``Texture``            what ``bake`` returns: ``layout``, ``texture`` [Ha,Wa,4] uint8, ``weight`` [Ha,Wa] fp32, ``view`` [Ha,Wa]
                           int32 (``blend="weighted"``: THE NUMBER OF ACCEPTED VIEWS; ``blend="best"``: the view taken, -1 for none),
                           ``uvs``, ``coverage`` and ``sample(face, bary)``;
  * ``render_textured``    ``meshray.pixel_rays`` + ``raycast(return_bary=True)`` + ``sample``: [V,H,W,3] views of the textured mesh;
  * ``write_textured_obj`` / ``read_textured_obj``, ``write_png`` / ``read_png``: OBJ text with ``vt`` lines, a ``.mtl`` and the
                           atlas as an 8-bit RGBA PNG through the standard library's ``zlib``, on the host.

``host=True`` (``texels``, ``bake_texels``, ``sample``, and ``bake`` with ``occlusion=False`` or a ``mask``) runs the library's host
twins on CPU tensors: the same functions, for tests and tools.  Everything else takes GPU tensors and nothing falls back.
"""
from __future__ import annotations

import math
import os
import struct
import zlib

import numpy as np
import torch

from ._native import call, call_on, host_array, require_device

MIN_PATCH, MAX_PATCH, MAX_VIEWS, MAX_POWER = 3, 4096, 64, 8      # include/lara_meshtexture.h
MAX_TEXELS = 1 << 30
DEFAULT_PATCH = 8
BLENDS = {"weighted": 0, "best": 1}


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def _cells_per_row(S, T, width):
    """C: from ``width`` (the widest atlas of at most that many texels), else the one that makes the atlas about square."""
    if width is not None:
        return max(1, int(width) // (S + 1))
    cells = (T + 1) // 2
    return max(1, math.isqrt(max(0, cells * S // (S + 1) - 1)) + 1) if cells else 1


def _layout(S, T, width):
    C = _cells_per_row(S, T, width)
    return S, C, C * (S + 1), max(1, -(-((T + 1) // 2) // C)) * S


def atlas(T, patch=None, width=None, max_texels=None):
    """The layout (S, C, Wa, Ha) for ``T`` triangles.  ``patch``: S (default 8); ``max_texels``: the largest S whose atlas holds at
    most that many texels (one of the two at most); ``width``: the atlas is at most that wide, C = width // (S + 1) (default: about
    square).  Raises for S < 3 and for an atlas of 2^30 texels or more.  T = 0 gives an S-high atlas without an owner."""
    T = int(T)
    if T < 0:
        raise ValueError("lara_amd.meshtexture: T must be >= 0")
    if patch is not None and max_texels is not None:
        raise ValueError("lara_amd.meshtexture: give patch or max_texels, not both")
    if max_texels is not None:
        fits = [S for S in range(MIN_PATCH, MAX_PATCH + 1) if (lambda L: L[2] * L[3])(_layout(S, T, width)) <= int(max_texels)]
        if not fits:
            raise ValueError(f"lara_amd.meshtexture: no patch of {MIN_PATCH} texels or more fits {T} triangles into {max_texels} texels")
        S = max(fits)
    else:
        S = DEFAULT_PATCH if patch is None else int(patch)
    if not MIN_PATCH <= S <= MAX_PATCH:
        raise ValueError(f"lara_amd.meshtexture: the patch size must lie in [{MIN_PATCH}, {MAX_PATCH}]")
    L = _layout(S, T, width)
    if L[2] * L[3] >= MAX_TEXELS:
        raise ValueError("lara_amd.meshtexture: an atlas of 2^30 texels and more")
    return L


def _checked_layout(layout, T):
    S, C, Wa, Ha = (int(x) for x in layout)
    size = host_array("l", 2)
    call("lara_meshtexture_atlas_size", None, S, C, int(T), size)
    if (size[0], size[1]) != (Wa, Ha):
        raise ValueError(f"lara_amd.meshtexture: the layout {tuple(layout)} is not the one of {T} triangles")
    return S, C, Wa, Ha


def corner_uvs(layout, T):
    """[T,3,2] fp32 (u, v) of the three corners of every triangle: u = x / Wa, v = 1 - y / Ha with (x, y) the corner's texel centre
    in texel units, computed in double and rounded once (host numpy)."""
    S, C, Wa, Ha = (int(x) for x in layout)
    f = np.arange(int(T), dtype=np.int64)
    cell, odd = f // 2, (f & 1).astype(bool)
    a = np.array([0, S - 2, 0], np.int64)[None, :]
    b = np.array([0, 0, S - 2], np.int64)[None, :]
    i = np.where(odd[:, None], S - a, a)
    j = np.where(odd[:, None], S - 1 - b, b)
    x = ((cell % C) * (S + 1))[:, None] + i + 0.5
    y = ((cell // C) * S)[:, None] + j + 0.5
    return torch.from_numpy(np.stack([x / np.float64(Wa), 1.0 - y / np.float64(Ha)], -1).astype(np.float32))


# ---- the three entries ----------------------------------------------------------------------------------------------------------------
def _mesh(vertices, triangles, host):
    V = vertices.detach().to(torch.float32).contiguous()
    if V.dim() != 2 or V.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError("lara_amd.meshtexture: expected vertices [Nv,3] and triangles [T,3]")
    if host:
        if V.is_cuda:
            raise RuntimeError("lara_amd.meshtexture: host=True takes CPU tensors")
    else:
        require_device(V)
    return V, triangles.detach().to(device=V.device, dtype=torch.int32).contiguous()


@torch.no_grad()
def texels(layout, vertices, triangles, host=False):
    """(face [Ha,Wa] int32, point [Ha,Wa,3] fp32, anchor [Ha,Wa,3] fp32): the owner of every texel (-1: none, or an invalid
    triangle), its surface point (extrapolated on the gutter row) and the same with the barycentrics clamped onto the triangle;
    NaN where unowned."""
    V, F = _mesh(vertices, triangles, host)
    S, C, Wa, Ha = _checked_layout(layout, F.shape[0])
    face = torch.empty(Ha, Wa, dtype=torch.int32, device=V.device)
    point = torch.empty(Ha, Wa, 3, dtype=torch.float32, device=V.device)
    anchor = torch.empty(Ha, Wa, 3, dtype=torch.float32, device=V.device)
    call_on("lara_meshtexture_texels", V.device, S, C, F.shape[0], V.shape[0], V, F, face, point, anchor)
    return face, point, anchor


def _cameras(ixt, c2w, dev):
    """(k [V,4], w2c [V,16], eyes [V,3]) fp32 on ``dev``, ``depthsurface.cameras``' convention; V = 0 passes."""
    from .depthsurface import cameras
    if len(ixt) == 0:
        z = torch.zeros(0, dtype=torch.float32, device=dev)
        return z.view(0, 4), z.view(0, 16), z.view(0, 3)
    k, w2c = cameras(ixt, c2w, invert=True)
    _, pose = cameras(ixt, c2w)
    eyes = np.ascontiguousarray(pose.reshape(-1, 4, 4)[:, :3, 3])
    return torch.from_numpy(k).to(dev), torch.from_numpy(w2c).to(dev), torch.from_numpy(eyes).to(dev)


@torch.no_grad()
def bake_texels(layout, vertices, triangles, face, point, anchor, images, k, w2c, eyes, mask=None, *, vertex_colors=None,
                blend="weighted", power=2, min_cos=0.1, two_sided=False, near=0.0, fill=(0, 0, 0), host=False):
    """(texture [Ha,Wa,4] uint8, weight [Ha,Wa] fp32, view [Ha,Wa] int32) of the texels ``texels`` wrote: the bake kernel alone, with
    the cameras as arrays and the visibility ``mask`` [Ha,Wa] int64 (None: every view) as given."""
    V, F = _mesh(vertices, triangles, host)
    S, C, Wa, Ha = _checked_layout(layout, F.shape[0])
    if blend not in BLENDS:
        raise ValueError('lara_amd.meshtexture: blend is "weighted" or "best"')
    power = int(power)
    if not 0 <= power <= MAX_POWER:
        raise ValueError(f"lara_amd.meshtexture: power must be an integer in [0, {MAX_POWER}]")
    if math.isnan(float(min_cos)) or math.isnan(float(near)):
        raise ValueError("lara_amd.meshtexture: min_cos and near must be numbers")
    dev = V.device
    I = images.detach().to(dev, torch.float32).contiguous()
    if I.dim() != 4 or I.shape[3] != 3:
        raise ValueError("lara_amd.meshtexture: expected images [V,H,W,3]")
    n_views, H, W = I.shape[:3]
    if n_views > MAX_VIEWS:
        raise ValueError(f"lara_amd.meshtexture: at most {MAX_VIEWS} views")
    if n_views * H * W >= 1 << 31:
        raise ValueError("lara_amd.meshtexture: 2^31 source pixels and more")
    if tuple(k.shape) != (n_views, 4) or tuple(w2c.shape) != (n_views, 16) or tuple(eyes.shape) != (n_views, 3):
        raise ValueError("lara_amd.meshtexture: one camera per image")
    cols = None
    if vertex_colors is not None:
        cols = vertex_colors.detach().to(dev, torch.float32).contiguous()
        if tuple(cols.shape) != tuple(V.shape):
            raise RuntimeError("lara_amd.meshtexture: expected vertex_colors [Nv,3]")
    if mask is not None:
        mask = mask.detach().to(dev, torch.int64).contiguous()
        if mask.numel() != Ha * Wa:
            raise RuntimeError("lara_amd.meshtexture: the mask must be [Ha,Wa]")
    face, point, anchor = face.contiguous(), point.contiguous(), anchor.contiguous()
    if face.numel() != Ha * Wa or point.numel() != 3 * Ha * Wa or anchor.numel() != 3 * Ha * Wa or face.dtype != torch.int32:
        raise RuntimeError("lara_amd.meshtexture: face, point and anchor must be those of this layout")
    texture = torch.empty(Ha, Wa, 4, dtype=torch.uint8, device=dev)
    weight = torch.empty(Ha, Wa, dtype=torch.float32, device=dev)
    view = torch.empty(Ha, Wa, dtype=torch.int32, device=dev)
    fill = [float(x) for x in fill]
    call_on("lara_meshtexture_bake", dev, S, C, F.shape[0], V.shape[0], V, F, face, point, anchor, n_views, H, W, I, k.contiguous(),
            w2c.contiguous(), eyes.contiguous(), mask, float(near), float(min_cos), power, int(bool(two_sided)), BLENDS[blend], cols,
            fill[0], fill[1], fill[2], texture, weight, view)
    return texture, weight, view


@torch.no_grad()
def sample(layout, T, texture, face, bary, alpha=False, background=(0, 0, 0), host=False):
    """[N,3] fp32 RGB in [0, 1] (``alpha``: [N,4]) of the atlas at ``face`` [N] and ``bary`` [N,3] (b1 and b2 are read, clamped into
    the triangle): four taps in a fixed order.  A face outside [0, T) gives ``background`` and alpha 0."""
    S, C, Wa, Ha = _checked_layout(layout, T)
    if host == texture.is_cuda:
        raise RuntimeError("lara_amd.meshtexture: host=True takes CPU tensors, host=False tensors on the GPU")
    dev = texture.device
    if texture.dtype != torch.uint8 or tuple(texture.shape) != (Ha, Wa, 4):
        raise RuntimeError("lara_amd.meshtexture: expected texture [Ha,Wa,4] uint8")
    f = face.detach().to(dev, torch.int32).contiguous().view(-1)
    b = bary.detach().to(dev, torch.float32).contiguous().view(-1, 3)
    N = f.shape[0]
    if b.shape[0] != N or N >= 1 << 30:
        raise RuntimeError("lara_amd.meshtexture: expected face [N] and bary [N,3], N < 2^30")
    channels = 4 if alpha else 3
    out = torch.empty(N, channels, dtype=torch.float32, device=dev)
    bg = [float(x) for x in background]
    call_on("lara_meshtexture_sample", dev, S, C, int(T), N, texture.contiguous(), f, b, channels, bg[0], bg[1], bg[2], out)
    return out


# ---- the bake -------------------------------------------------------------------------------------------------------------------------
class Texture:
    """A baked atlas: ``layout`` (S, C, Wa, Ha), ``n_triangles``, ``texture`` [Ha,Wa,4] uint8 RGBA, ``weight`` [Ha,Wa] fp32, ``view``
    [Ha,Wa] int32, ``face`` [Ha,Wa] int32 (the owner map), ``uvs`` [T,3,2] fp32 (host), ``mask`` (the visibility the bake used, or
    None)."""

    def __init__(self, layout, n_triangles, texture, weight, view, face, mask=None, blend="weighted"):
        self.layout, self.n_triangles, self.texture, self.weight, self.view = tuple(layout), int(n_triangles), texture, weight, view
        self.face, self.mask, self.blend = face, mask, blend
        self.uvs = corner_uvs(layout, n_triangles)
        self._coverage = None

    @property
    def coverage(self):
        """The share of owned texels some view coloured (alpha 255); 0 without an owned texel.  The one host read, made once."""
        if self._coverage is None:
            owned = self.face >= 0
            n = torch.stack([owned.sum(), (owned & (self.texture[..., 3] == 255)).sum()]).cpu().tolist()
            self._coverage = n[1] / n[0] if n[0] else 0.0
        return self._coverage

    def sample(self, face, bary, alpha=False, background=(0, 0, 0)):
        return sample(self.layout, self.n_triangles, self.texture, face, bary, alpha, background, host=not self.texture.is_cuda)


@torch.no_grad()
def bake(vertices, triangles, images, ixt, c2w, *, patch=None, max_texels=None, width=None, vertex_colors=None, blend="weighted",
         power=2, min_cos=0.1, two_sided=False, occlusion=True, bvh=None, near=0.0, fill=(0, 0, 0), mask=None, host=False):
    """A ``Texture`` for the mesh from ``images`` [V,H,W,3] fp32 in [0, 1] seen through ``ixt`` [V,3,3], ``c2w`` [V,4,4]
    (``depthsurface.cameras``' convention), V <= 64.  ``occlusion``: a view colours a texel only when ``meshray.visibility`` sees the
    texel's anchor from its eye past the mesh (``bvh``: the mesh's ``meshbvh.TriangleBVH``, built here when None); a precomputed
    ``mask`` [Ha,Wa] int64 stands in for that walk.  ``vertex_colors`` [Nv,3] in [0, 1]: the fallback of a texel no view accepts
    (else ``fill``).  See the module's text for the rest."""
    V, F = _mesh(vertices, triangles, host)
    I = torch.as_tensor(images)
    if I.dim() != 4 or I.shape[3] != 3:
        raise ValueError("lara_amd.meshtexture: expected images [V,H,W,3]")
    if I.shape[0] > MAX_VIEWS:
        raise ValueError(f"lara_amd.meshtexture: at most {MAX_VIEWS} views")
    T = F.shape[0]
    layout = atlas(T, patch, width, max_texels)
    k, w2c, eyes = _cameras(ixt, c2w, V.device)
    face, point, anchor = texels(layout, V, F, host)
    if mask is None and occlusion and T > 0 and I.shape[0] > 0:
        if host:
            raise RuntimeError("lara_amd.meshtexture: host=True has no visibility walk; pass mask= or occlusion=False")
        from . import meshray
        if bvh is None:
            from .meshbvh import TriangleBVH
            bvh = TriangleBVH(V, F)
        mask = meshray.visibility(bvh, anchor.view(-1, 3), eyes, faces=face.view(-1)).view(face.shape)
    texture, weight, view = bake_texels(layout, V, F, face, point, anchor, I, k, w2c, eyes, mask, vertex_colors=vertex_colors,
                                        blend=blend, power=power, min_cos=min_cos, two_sided=two_sided, near=near, fill=fill, host=host)
    return Texture(layout, T, texture, weight, view, face, mask, blend)


@torch.no_grad()
def render_textured(bvh, tex, ixt, c2w, H, W, background=(0, 0, 0)):
    """[V,H,W,3] fp32: the textured mesh of ``bvh`` (a ``meshbvh.TriangleBVH``) through the pixel centres of the cameras; a ray
    that misses gives ``background``."""
    from . import meshray
    H, W = int(H), int(W)
    o, d = meshray.pixel_rays(ixt, c2w, H, W, bvh.device)
    _, face, bary = meshray.raycast(bvh, o.view(-1, 3), d.view(-1, 3), return_bary=True)
    return tex.sample(face, bary, background=background).view(o.shape[0], H, W, 3)


# ---- files (host) -----------------------------------------------------------------------------------------------------------------------
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, rgba):
    """``rgba`` [H,W,4] uint8 as an 8-bit RGBA PNG: one IDAT, every row with filter 0, through ``zlib``."""
    a = np.ascontiguousarray(_host(rgba))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("lara_amd.meshtexture: write_png takes [H,W,4] uint8")
    H, W = a.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, W * 4)], 1)
    data = _PNG_MAGIC + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
    with open(path, "wb") as f:
        f.write(data + _chunk(b"IEND", b""))


def read_png(path):
    """[H,W,4] uint8 of a PNG ``write_png`` wrote (8-bit RGBA, no interlace, filter 0 on every row); anything else raises."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError("lara_amd.meshtexture: not a PNG")
    o, idat, head = 8, b"", None
    while o + 12 <= len(data):
        n, kind = struct.unpack(">I", data[o:o + 4])[0], data[o + 4:o + 8]
        body = data[o + 8:o + 8 + n]
        if struct.unpack(">I", data[o + 8 + n:o + 12 + n])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError("lara_amd.meshtexture: a PNG chunk fails its CRC")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            break
        o += 12 + n
    if head is None or head[2:] != (8, 6, 0, 0, 0):
        raise ValueError("lara_amd.meshtexture: read_png reads 8-bit RGBA without interlace only")
    W, H = head[:2]
    rows = np.frombuffer(zlib.decompress(idat), np.uint8)
    if rows.size != H * (1 + 4 * W):
        raise ValueError("lara_amd.meshtexture: the PNG's data has the wrong size")
    rows = rows.reshape(H, 1 + 4 * W)
    if rows[:, 0].any():
        raise ValueError("lara_amd.meshtexture: read_png reads filter 0 only")
    return rows[:, 1:].reshape(H, W, 4).copy()


def _host(x):
    """A host numpy array of a tensor or an array (an array is taken as it is)."""
    return x if isinstance(x, np.ndarray) else torch.as_tensor(x).detach().cpu().numpy()


def _lines(prefix, columns, fmt):
    line = np.full(len(columns[0]), prefix, dtype=object).astype(str)
    for col in columns:
        line = np.char.add(np.char.add(line, " "), np.char.mod(fmt, col) if fmt else col)
    return line


def write_textured_obj(path, vertices, triangles, tex):
    """``path`` (.obj) with ``mtllib``, ``usemtl``, one ``v x y z`` line per vertex, three ``vt u v`` lines per triangle and one
    ``f a/ta b/tb c/tc`` line per triangle (``%.9g``: fp32 values read back to the same bits); beside it ``<stem>.mtl`` naming
    ``<stem>.png``, the atlas.  Returns the three paths."""
    path = str(path)
    stem, ext = os.path.splitext(path)
    if ext.lower() != ".obj":
        raise ValueError("lara_amd.meshtexture: a textured mesh is written as .obj")
    v = _host(vertices).astype(np.float32, copy=False).reshape(-1, 3)
    t = _host(triangles).astype(np.int64, copy=False).reshape(-1, 3)
    uv = tex.uvs.numpy().reshape(-1, 2)
    if len(uv) != 3 * len(t):
        raise ValueError("lara_amd.meshtexture: the texture was baked for another mesh")
    name = os.path.basename(stem)
    parts = [np.array([f"mtllib {name}.mtl", "usemtl atlas"])]
    if len(v):
        parts.append(_lines("v", [v[:, c].astype(np.float64) for c in range(3)], "%.9g"))
    if len(t):
        parts.append(_lines("vt", [uv[:, c].astype(np.float64) for c in range(2)], "%.9g"))
        ti = 3 * np.arange(len(t), dtype=np.int64)
        cols = [np.char.add(np.char.add((t[:, c] + 1).astype(str), "/"), (ti + c + 1).astype(str)) for c in range(3)]
        parts.append(_lines("f", cols, None))
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(np.concatenate(parts).tolist()) + "\n")
    with open(stem + ".mtl", "w") as f:
        f.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    write_png(stem + ".png", tex.texture)
    return path, stem + ".mtl", stem + ".png"


def read_textured_obj(path):
    """(vertices [Nv,3] fp32, triangles [T,3] int64, uvs [T,3,2] fp32, rgba [H,W,4] uint8) of files ``write_textured_obj`` wrote: the
    image is found through ``mtllib`` and the ``.mtl``'s ``map_Kd``."""
    path = str(path)
    vs, vts, fs, mtl = [], [], [], None
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                vs.append(w[1:4])
            elif w[0] == "vt":
                vts.append(w[1:3])
            elif w[0] == "f":
                fs.append([p.split("/")[:2] for p in w[1:4]])
            elif w[0] == "mtllib":
                mtl = w[1]
    if mtl is None:
        raise ValueError("lara_amd.meshtexture: the OBJ names no mtllib")
    image = None
    with open(os.path.join(os.path.dirname(os.path.abspath(path)), mtl)) as f:
        for line in f:
            w = line.split()
            if w and w[0] == "map_Kd":
                image = w[1]
    if image is None:
        raise ValueError("lara_amd.meshtexture: the .mtl names no map_Kd")
    v = np.array(vs, np.float64).reshape(-1, 3).astype(np.float32)
    vt = np.array(vts, np.float64).reshape(-1, 2).astype(np.float32)
    idx = np.array(fs, np.int64).reshape(-1, 3, 2) - 1
    uvs = vt[idx[:, :, 1]] if len(idx) else np.zeros((0, 3, 2), np.float32)
    return v, idx[:, :, 0], uvs, read_png(os.path.join(os.path.dirname(os.path.abspath(path)), image))
