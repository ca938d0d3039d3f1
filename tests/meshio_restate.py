"""numpy / Python restatements of include/lara_meshio.h: the "%.9g" token, the decimal index, the PLY file as a structured
array's ``tobytes()``, the colour rule in float64.  The OBJ text is not restated: its target is the file ``mesh.write_obj`` writes."""
import numpy as np


def fmt9g(x):
    """The token of one fp32 value."""
    return "%.9g" % float(np.float32(x))


def fmt9g_of_bits(bits):
    """The tokens of fp32 bit patterns, as a numpy array of byte strings."""
    with np.errstate(invalid="ignore"):          # (a signalling NaN among the patterns)
        v = np.asarray(bits, np.uint32).view(np.float32).astype(np.float64)
    return np.char.mod("%.9g", v).astype("S16")


def color_u8(c):
    """floor(255.0 * clamp(c, 0, 1) + 0.5) in float64, NaN -> 0."""
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(c), 0.0, np.minimum(np.maximum(c, 0.0), 1.0))
    return np.floor(255.0 * x + 0.5).astype(np.uint8)


def ply_header(nv, nt, normals, colors):
    h = "ply\nformat binary_little_endian 1.0\ncomment lara_amd.meshio\n" + "element vertex %d\n" % nv
    h += "property float x\nproperty float y\nproperty float z\n"
    if normals:
        h += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors:
        h += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    return (h + "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % nt).encode("ascii")


def ply_bytes(vertices, triangles, colors=None, normals=None):
    """The whole file: header, packed vertex rows, packed face rows."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    fields = [("p", "<f4", (3,))] + ([("n", "<f4", (3,))] if normals is not None else []) + ([("c", "u1", (3,))] if colors is not None else [])
    rows = np.zeros(len(v), np.dtype(fields))
    assert rows.dtype.itemsize == 12 + (12 if normals is not None else 0) + (3 if colors is not None else 0)
    rows["p"] = v
    if normals is not None:
        rows["n"] = np.asarray(normals, np.float32).reshape(-1, 3)
    if colors is not None:
        rows["c"] = color_u8(np.asarray(colors, np.float32).reshape(-1, 3))
    faces = np.zeros(len(t), np.dtype([("k", "u1"), ("i", "<i4", (3,))]))
    assert faces.dtype.itemsize == 13
    faces["k"] = 3
    faces["i"] = t.astype(np.int32)
    return ply_header(len(v), len(t), normals is not None, colors is not None) + rows.tobytes() + faces.tobytes()
