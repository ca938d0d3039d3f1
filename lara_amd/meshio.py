"""The extracted mesh as a file, serialised on the device (include/lara_meshio.h, csrc/meshio.hip, csrc/fmt9g.h); opt-in like
every module here.  ``mesh.write_obj`` copies the mesh to the host and formats ~850 k lines with numpy string operations; here the
text is built by kernels and the host only copies and writes it:

  * ``obj_bytes``   the bytes ``mesh.write_obj`` writes for the same arguments, as a uint8 tensor on the device (``%.9g`` exactly, for
                    every fp32 bit pattern; integer arithmetic only);
  * ``ply_bytes``   a binary little-endian PLY (positions, optional normals, optional uchar colours, int32 faces);
  * ``write_mesh``  one of the two by the path's extension, as the reference's ``o3d.io.write_triangle_mesh`` picks its format
                    (tools/meshExtractor.py:135): the bytes, one device-to-host copy into a pinned buffer, one ``f.write``;
  * ``read_ply`` / ``read_mesh``  read the files back (``np.frombuffer``; ``.obj`` goes to ``mesh.read_obj``).

Open3D is absent here, so parity with its own writers is unpinned: the PLY property names (x y z, nx ny nz, red green blue,
vertex_indices) are the common ones [RECALLED], the header carries a comment line of this module, and ``read_ply`` reads the files
this module wrote, not PLY in general.  No CPU path: tensors must live on the GPU."""
from __future__ import annotations

import os
import re

import numpy as np
import torch

from . import mesh
from ._native import StreamWorkspace, call, query, require_device

BLOCK_LINES, MAX_F32_TOKEN, MAX_U32_TOKEN, MAX_VERTEX_LINE, MAX_FACE_LINE = 256, 15, 10, 98, 35     # include/lara_meshio.h
PLY_FACE_ROW, MAX_VERTICES, MAX_TRIANGLES, MAX_INDEX = 13, 2 ** 31 - 1, (2 ** 31 - 1) // 3, 2 ** 31 - 2
FORMATS = ("obj", "ply")

_bytes = StreamWorkspace()
_pinned = None        # the host side of write_mesh's one copy, grown on demand


def _workspace(dev, nbytes):
    return _bytes(dev, nbytes)[:nbytes].view(torch.int64)


def _mark(marks, name):
    if marks is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))


def _rows(x, dev, what):
    require_device(x)
    x = x.detach().to(dev, torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f"lara_amd.meshio: expected {what} [Nv,3]")
    return x


def _inputs(vertices, triangles, colors, normals):
    """(V fp32 [Nv,3], F int32 or int64 [T,3], bytes per index, C or None, N or None), contiguous on the vertices' device."""
    require_device(vertices)
    require_device(triangles)
    dev = vertices.device
    V = _rows(vertices, dev, "vertices")
    F = triangles.detach().to(dev)
    if F.dim() != 2 or F.shape[1] != 3:
        raise RuntimeError("lara_amd.meshio: expected triangles [T,3]")
    if F.dtype.is_floating_point or F.dtype.is_complex or F.dtype == torch.bool:
        raise ValueError("lara_amd.meshio: triangles must have an integer type")
    if F.dtype != torch.int32:
        F = F.to(torch.int64)          # (the kernels check the range on the 64-bit value, then write it as an int32)
    F = F.contiguous()
    if V.shape[0] > MAX_VERTICES or F.shape[0] > MAX_TRIANGLES:
        raise RuntimeError("lara_amd.meshio: meshes need Nv < 2^31 and 3 T < 2^31 (int32 indices)")
    C = None if colors is None else _rows(colors, dev, "colors")
    N = None if normals is None else _rows(normals, dev, "normals")
    for x, what in ((C, "colors"), (N, "normals")):
        if x is not None and x.shape[0] != V.shape[0]:
            raise RuntimeError(f"lara_amd.meshio: {what} must have one row per vertex")
    return V, F, F.element_size(), C, N


def _raise_on(err_word):
    if err_word & 1:
        raise RuntimeError("lara_amd.meshio: a triangle index lies outside [0, 2^31 - 1)")


@torch.no_grad()
def obj_bytes(vertices, triangles, colors=None, *, _marks=None):
    """The bytes ``mesh.write_obj(path, vertices, triangles, colors)`` writes, as a uint8 tensor on the device: every
    ``v x y z [r g b]`` line (``%.9g``), then every 1-based ``f a b c`` line, each ended by a newline; an empty part is omitted, an
    empty mesh gives a tensor of length 0.  vertices / colors [Nv,3] (cast to fp32 as ``write_obj`` casts them), triangles [T,3] of any
    integer type.  One host read (the size, and the error word with it): an index outside [0, 2^31 - 1) raises RuntimeError; indices
    are not compared with Nv, as in ``write_obj``."""
    V, F, ib, C, _ = _inputs(vertices, triangles, colors, None)
    dev = V.device
    Nv, T = V.shape[0], F.shape[0]
    if Nv == 0 and T == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _mark(_marks, "start")
        ws = _workspace(dev, query("lara_meshio_obj_workspace_bytes", Nv, T))
        nb = ws.numel() - 1
        call("lara_meshio_obj_lengths", dev, Nv, V, C, T, F, ib, ws)
        _mark(_marks, "lengths")
        ends = torch.cumsum(ws[:nb], 0)
        total, e = torch.stack([ends[-1], ws[nb]]).tolist()          # the one host read: the size and the error word
        _raise_on(e)
        offsets = ends - ws[:nb]
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        _mark(_marks, "scan + host read")
        call("lara_meshio_obj_emit", dev, Nv, V, C, T, F, ib, offsets, out)
        _mark(_marks, "emit")
    return out


def ply_header(n_vertices, n_triangles, normals=False, colors=False):
    """The header text of the files ``ply_bytes`` builds, as bytes."""
    lines = ["ply", "format binary_little_endian 1.0", "comment lara_amd.meshio", f"element vertex {int(n_vertices)}"]
    lines += [f"property float {a}" for a in "xyz"]
    if normals:
        lines += [f"property float n{a}" for a in "xyz"]
    if colors:
        lines += [f"property uchar {a}" for a in ("red", "green", "blue")]
    lines += [f"element face {int(n_triangles)}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


@torch.no_grad()
def ply_bytes(vertices, triangles, colors=None, normals=None, *, _marks=None):
    """A binary little-endian PLY as a uint8 tensor on the device: ``ply_header`` (built on the host), then packed vertex rows --
    float x y z, float nx ny nz with ``normals``, uchar red green blue with ``colors``: 12, 15, 24 or 27 bytes -- and packed face
    rows of 13 bytes (the byte 3 and three int32 indices, 0-based).  Floats are bit copies; a colour becomes
    floor(255.0 * clamp(c, 0, 1) + 0.5) in double, NaN 0.  Parity with Open3D's writer is unpinned (Open3D is absent); the property
    names are the common ones [RECALLED].  One host read (the error word): an index outside [0, 2^31 - 1) raises RuntimeError."""
    V, F, ib, C, N = _inputs(vertices, triangles, colors, normals)
    dev = V.device
    Nv, T = V.shape[0], F.shape[0]
    header = ply_header(Nv, T, N is not None, C is not None)
    body = query("lara_meshio_ply_body_bytes", Nv, T, int(N is not None), int(C is not None))
    with torch.cuda.device(dev):
        _mark(_marks, "start")
        out = torch.empty(len(header) + body, dtype=torch.uint8, device=dev)
        out[:len(header)] = torch.frombuffer(bytearray(header), dtype=torch.uint8).to(dev)
        if Nv or T:
            ws = _workspace(dev, query("lara_meshio_ply_workspace_bytes"))
            call("lara_meshio_ply_pack", dev, Nv, V, N, C, T, F, ib, out.data_ptr() + len(header), ws)
            _mark(_marks, "pack")
            _raise_on(int(ws[0]))                                     # the one host read: the error word
            _mark(_marks, "host read")
    return out


def _format_of(path, format):
    if format is None:
        format = os.path.splitext(os.fspath(path))[1][1:].lower()
        if format not in FORMATS:
            raise ValueError(f"lara_amd.meshio: the extension of {path!r} names no format (.obj, .ply); pass format=")
    if format not in FORMATS:
        raise ValueError(f'lara_amd.meshio: format is "obj" or "ply", not {format!r}')
    return format


@torch.no_grad()
def write_mesh(path, vertices, triangles, colors=None, normals=None, *, format=None, _marks=None):
    """Write the mesh to ``path`` as OBJ text (``obj_bytes``) or binary PLY (``ply_bytes``): ``format`` "obj" / "ply", or None for
    the path's extension (any letter case; anything else raises ValueError).  ``normals`` with "obj" raises ValueError (``vn`` lines
    are out of scope).  The bytes are built on the device, copied once into a pinned host buffer and written by one ``f.write``; the
    directory is created as ``mesh.write_obj`` creates it.  Nothing is written when the mesh is refused.  Returns the number of
    bytes written."""
    global _pinned
    format = _format_of(path, format)
    if format == "obj" and normals is not None:
        raise ValueError("lara_amd.meshio: OBJ output takes no normals (vn lines are out of scope)")
    if format == "obj":
        data = obj_bytes(vertices, triangles, colors, _marks=_marks)
    else:
        data = ply_bytes(vertices, triangles, colors, normals, _marks=_marks)
    n = data.numel()
    if _pinned is None or _pinned.numel() < n:
        _pinned = torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=True)
    host = _pinned[:n]
    host.copy_(data)                                                  # the one device-to-host copy (waits for the stream)
    _mark(_marks, "copy")
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(memoryview(host.numpy()))
    return n


_HEADER_RE = re.compile(rb"ply\nformat binary_little_endian 1\.0\ncomment lara_amd\.meshio\nelement vertex (\d+)\n"
                        rb"property float x\nproperty float y\nproperty float z\n(property float nx\nproperty float ny\nproperty float nz\n)?"
                        rb"(property uchar red\nproperty uchar green\nproperty uchar blue\n)?"
                        rb"element face (\d+)\nproperty list uchar int vertex_indices\nend_header\n")


def read_ply(path, return_normals=False):
    """(vertices [Nv,3] fp32, triangles [T,3] int64, colors [Nv,3] fp32 = u8 / 255 or None) of a file this module wrote: the rows
    through ``np.frombuffer`` with a structured dtype built from the header.  Normals, when the file has them, are skipped, or with
    ``return_normals`` returned as a fourth item ([Nv,3] fp32, the file's bits; None when the file has none).  Any
    other header, a face that is no triangle or a size that does not fit raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    m = _HEADER_RE.match(data)
    if m is None:
        raise ValueError(f"lara_amd.meshio.read_ply: {path!r} does not start with a header this module writes")
    nv, nt, has_n, has_c = int(m.group(1)), int(m.group(4)), m.group(2) is not None, m.group(3) is not None
    fields = [(a, "<f4") for a in "xyz"] + ([(f"n{a}", "<f4") for a in "xyz"] if has_n else []) \
        + ([(a, "u1") for a in ("red", "green", "blue")] if has_c else [])
    vtype, ftype = np.dtype(fields), np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(data) != m.end() + nv * vtype.itemsize + nt * ftype.itemsize:
        raise ValueError(f"lara_amd.meshio.read_ply: {path!r} has {len(data)} bytes, its header promises "
                         f"{m.end() + nv * vtype.itemsize + nt * ftype.itemsize}")
    rows = np.frombuffer(data, vtype, nv, m.end())
    faces = np.frombuffer(data, ftype, nt, m.end() + nv * vtype.itemsize)
    if np.any(faces["n"] != 3):
        raise ValueError(f"lara_amd.meshio.read_ply: {path!r} holds a face that is no triangle")
    v = np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)
    c = None
    if has_c:
        c = np.stack([rows["red"], rows["green"], rows["blue"]], axis=1).astype(np.float32) / np.float32(255) if nv \
            else np.zeros((0, 3), np.float32)
    t = faces["i"].astype(np.int64).reshape(-1, 3)
    if not return_normals:
        return v, t, c
    n = None
    if has_n:
        n = np.stack([rows["nx"], rows["ny"], rows["nz"]], axis=1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)
    return v, t, c, n


def read_mesh(path):
    """``read_ply`` for ``.ply``, ``mesh.read_obj`` for ``.obj`` (any letter case): (vertices, triangles, colors or None)."""
    return read_ply(path) if _format_of(path, None) == "ply" else mesh.read_obj(path)
