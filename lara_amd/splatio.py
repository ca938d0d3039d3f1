"""The predicted surfels on disk: the 2DGS / 3DGS ``point_cloud.ply`` written from and read back into the tensors
``Renderer.render_img`` / ``render_views`` take; opt-in like every module here, imported by nothing on the default routes.

``render_pkg`` (``LaRaPipeline(..., return_buffer=True)``, lightning/network.py:483, :515) holds the PRE-activation values --
opacity logit, log scales, unnormalised quaternion; renderer_2dgs.py:181-189 applies sigmoid / exp / normalize inside
``render_img`` -- and that is what the file stores.  Values are copied as 32-bit words, never recomputed: a round trip through a
file returns every tensor's bits (NaN payloads, infinities, -0.0 and denormals included), and a render of the loaded file is the
render of the original tensors.

  * ``SurfelCloud``           the five tensors, ``from_render_pkg`` / ``render_args`` / ``gs_params`` / ``to``;
  * ``scene_item``            one scene's coarse or fine entry of ``render_pkg``;
  * ``select`` / ``concatenate``  ordered row selection (opacity, box) and joining;
  * ``check_fields``          the five tensors of a cloud as ``splatrefine``'s and ``splatdensify``'s kernels take them;
  * ``ply_header`` / ``ply_bytes`` / ``write_ply``  one packed [P, F] fp32 buffer where the tensors lie, one copy to the host;
  * ``read_ply``              properties by name in any order, other scalar properties skipped, a third scale dropped and reported.

The layout is that of the 2DGS / 3DGS code bases' ``save_ply`` [RECALLED: neither code base nor `plyfile` is in the build image]:
binary little-endian, every property ``float``, in the order ``x y z  nx ny nz  f_dc_0..2  f_rest_*  opacity  scale_*  rot_0..3``;
``f_rest_{c (n - 1) + k} = shs[p, 1 + k, c]`` (channel-major: ``features_rest.transpose(1, 2).flatten(1)``); ``rot_i`` in the
stored order, which the reference's ``build_rotation`` reads as w, x, y, z; normals zero.

No kernel of the library is launched: the module works on tensors on any device (torch operators only), the write is a host step.
The 32-byte ``.splat`` format and the web viewers' compressed PLY (both lossy) are ``lara_amd.splatpack``'s; ASCII and big-endian
files are out of scope.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

SH_COEFFS = {1: 0, 4: 1, 9: 2, 16: 3}          # coefficients per channel -> SH degree
_WHO = "lara_amd.splatio"


# ---------------------------------------------------------------------------------------------------------- the cloud

class SurfelCloud:
    """A set of P surfels as ``render_img`` takes them: ``centers`` [P,3], ``shs`` [P,n,3] (n = (d+1)^2, d in 0..3), ``opacity``
    [P,1], ``scales`` [P,2], ``rotations`` [P,4]; all fp32 on one device, all pre-activation, detached."""

    FIELDS = ("centers", "shs", "opacity", "scales", "rotations")

    def __init__(self, centers, shs, opacity, scales, rotations):
        ts = [torch.as_tensor(t).detach() for t in (centers, shs, opacity, scales, rotations)]
        P = ts[0].shape[0] if ts[0].dim() else -1
        n = ts[1].shape[1] if ts[1].dim() == 3 else -1
        want = ((P, 3), (P, n, 3), (P, 1), (P, 2), (P, 4))
        for name, t, w in zip(self.FIELDS, ts, want):
            if tuple(t.shape) != w or n not in SH_COEFFS:
                raise ValueError(f"{_WHO}: expected centers [P,3], shs [P,n,3] with n in (1, 4, 9, 16), opacity [P,1], scales [P,2], "
                                 f"rotations [P,4]; {name} is {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise ValueError(f"{_WHO}: {name} is {t.dtype}; the file stores fp32 words, cast before (nothing is converted here)")
            if t.device != ts[0].device:
                raise ValueError(f"{_WHO}: {name} lies on {t.device}, centers on {ts[0].device}")
        self.centers, self.shs, self.opacity, self.scales, self.rotations = ts
        self.n_surfels, self.sh_degree = int(P), SH_COEFFS[n]

    @property
    def device(self):
        return self.centers.device

    @classmethod
    def from_render_pkg(cls, item):
        """One entry of ``render_pkg``: the coarse 5-tuple (centers, shs, opacity, scaling, rotation) as it is; of the fine 6-tuple
        (centers[mask], shs_fine, opacity, scaling, rotation, mask) centres and shs are the subset already and opacity / scaling /
        rotation are indexed by ``mask`` (network.py:524, meshExtractor.py:85)."""
        if len(item) == 6:
            centers, shs, opacity, scaling, rotation, mask = item
            opacity, scaling, rotation = opacity[mask], scaling[mask], rotation[mask]
        elif len(item) == 5:
            centers, shs, opacity, scaling, rotation = item
        else:
            raise ValueError(f"{_WHO}: an entry of render_pkg is a 5-tuple (coarse) or a 6-tuple (fine), got {len(item)} items")
        return cls(centers, shs, opacity, scaling, rotation)

    def to(self, device):
        return SurfelCloud(*(t.to(device) for t in self.render_args()))

    def render_args(self):
        """(centers, shs, opacity, scales, rotations): ``render_img``'s / ``render_views``' order."""
        return self.centers, self.shs, self.opacity, self.scales, self.rotations

    def gs_params(self):
        """The 6-tuple ``lara_amd.mesh.MeshExtractor`` takes, with an all-true mask."""
        return self.render_args() + (torch.ones(self.n_surfels, dtype=torch.bool, device=self.device),)


def scene_item(render_pkg, scene, stage="fine", with_fine=True):
    """The entry of ``render_pkg`` for ``scene`` in the list order network.py builds: per scene the coarse tuple, then the fine
    tuple when the step ran the fine stage (``with_fine``)."""
    if stage not in ("fine", "coarse"):
        raise ValueError(f'{_WHO}: stage is "fine" or "coarse", not {stage!r}')
    if stage == "fine" and not with_fine:
        raise ValueError(f"{_WHO}: a step without the fine stage has no fine entry")
    per = 2 if with_fine else 1
    if len(render_pkg) % per or not 0 <= int(scene) < len(render_pkg) // per:
        raise ValueError(f"{_WHO}: render_pkg has {len(render_pkg)} entries, {per} per scene: no scene {scene}")
    item = render_pkg[per * int(scene) + (1 if stage == "fine" else 0)]
    if len(item) != (6 if stage == "fine" else 5):
        raise ValueError(f"{_WHO}: entry {per * int(scene)} of render_pkg is not the {stage} tuple (was the step run with_fine={not with_fine}?)")
    return item


def select(cloud, min_opacity=None, aabb=None):
    """The rows that pass the given filters, in ascending index order: ``min_opacity`` keeps sigmoid(opacity) > min_opacity
    (fp32; the reference's own rule is 0.005, network.py:465), ``aabb`` = (lo [3], hi [3]) keeps lo <= centre <= hi on every axis.
    A NaN opacity or centre fails both comparisons: dropped when its filter is given, kept when none is.  Returns (the new cloud,
    the kept indices as int64)."""
    keep = torch.ones(cloud.n_surfels, dtype=torch.bool, device=cloud.device)
    if min_opacity is not None:
        keep &= torch.sigmoid(cloud.opacity[:, 0]) > float(min_opacity)
    if aabb is not None:
        box = torch.as_tensor(aabb, dtype=torch.float32).reshape(2, 3).to(cloud.device)
        keep &= ((cloud.centers >= box[0]) & (cloud.centers <= box[1])).all(dim=1)
    idx = keep.nonzero().squeeze(1)
    return SurfelCloud(*(t[idx] for t in cloud.render_args())), idx


def concatenate(clouds):
    """The clouds' rows one after the other, in the order given; they must share one SH degree (and one device)."""
    clouds = list(clouds)
    if not clouds:
        raise ValueError(f"{_WHO}: nothing to concatenate")
    if len({c.sh_degree for c in clouds}) != 1:
        raise ValueError(f"{_WHO}: the clouds have SH degrees {[c.sh_degree for c in clouds]}; they must share one")
    return SurfelCloud(*(torch.cat(ts) for ts in zip(*(c.render_args() for c in clouds))))


def check_fields(who, what, ts, like=None):
    """The five tensors of ``what`` as the surfel kernels take them (``splatrefine``, ``splatdensify``): fp32, contiguous, one
    device, a cloud's shapes (or ``like``'s).  ``who`` is the calling module's name, the head of every message."""
    FIELDS = SurfelCloud.FIELDS
    ts = list(ts)
    if len(ts) != len(FIELDS) or not all(isinstance(t, torch.Tensor) for t in ts):
        raise ValueError(f"{who}: {what} is five tensors {FIELDS}")
    if like is None:
        P = ts[0].shape[0] if ts[0].dim() == 2 else -1
        n = ts[1].shape[1] if ts[1].dim() == 3 else -1
        if n not in SH_COEFFS:
            raise ValueError(f"{who}: {what}: shs is [P,n,3] with n in (1, 4, 9, 16), got {tuple(ts[1].shape)}")
        shapes = ((P, 3), (P, n, 3), (P, 1), (P, 2), (P, 4))
    else:
        shapes = [tuple(t.shape) for t in like]
    dev = (like or ts)[0].device
    for name, t, shape in zip(FIELDS, ts, shapes):
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{who}: {what}.{name} is {tuple(t.shape)}, expected {tuple(shape)}")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: {what}.{name} is {t.dtype}; the update works on fp32 words")
        if not t.is_contiguous():
            raise ValueError(f"{who}: {what}.{name} is not contiguous")
        if t.device != dev:
            raise ValueError(f"{who}: {what}.{name} lies on {t.device}, params.centers on {dev}")
    return ts


# ---------------------------------------------------------------------------------------------------------- writing

def _names(sh_degree, n_scales, normals=True):
    """The float properties in file order [RECALLED: the order of the 2DGS / 3DGS ``construct_list_of_attributes``]."""
    n = (int(sh_degree) + 1) ** 2
    return (["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + [f"f_dc_{i}" for i in range(3)]
            + [f"f_rest_{i}" for i in range(3 * (n - 1))] + ["opacity"] + [f"scale_{i}" for i in range(n_scales)]
            + [f"rot_{i}" for i in range(4)])


def ply_header(P, sh_degree, third_scale=False):
    """The header text of the files ``ply_bytes`` builds, as bytes."""
    if int(sh_degree) not in SH_COEFFS.values() or int(P) < 0:
        raise ValueError(f"{_WHO}: SH degree 0..3 and a surfel count >= 0, got {sh_degree} and {P}")
    lines = ["ply", "format binary_little_endian 1.0", f"comment {_WHO}", f"element vertex {int(P)}"]
    lines += [f"property float {a}" for a in _names(sh_degree, 3 if third_scale else 2)] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def _thickness_word(thickness):
    if thickness is None:
        return None
    s = float(thickness)
    if not (s > 0 and math.isfinite(s)):
        raise ValueError(f"{_WHO}: thickness must be a finite number > 0, got {thickness!r}")
    return float(np.float32(math.log(s)))


@torch.no_grad()
def _pack(cloud, thickness=None):
    """The file's body as ONE [P, F] fp32 tensor where the cloud lies.  The columns are filled through the buffer's int32 view:
    32-bit words are moved, no float operation touches them."""
    third = _thickness_word(thickness)
    P, n = cloud.n_surfels, cloud.shs.shape[1]
    F = 3 + 3 + 3 * n + 1 + (2 if third is None else 3) + 4
    buf = torch.empty(P, F, dtype=torch.float32, device=cloud.device)
    w = buf.view(torch.int32)
    shs = cloud.shs.view(torch.int32)
    w[:, 0:3] = cloud.centers.view(torch.int32)
    w[:, 3:6] = 0                                                       # nx ny nz: +0.0
    w[:, 6:9] = shs[:, 0, :]
    o = 9 + 3 * (n - 1)
    w[:, 9:o].view(P, 3, n - 1).copy_(shs[:, 1:, :].transpose(1, 2))     # channel-major: f_rest_{c (n-1) + k} = shs[p, 1 + k, c]
    w[:, o:o + 1] = cloud.opacity.view(torch.int32)
    w[:, o + 1:o + 3] = cloud.scales.view(torch.int32)
    o += 3
    if third is not None:
        buf[:, o] = third
        o += 1
    w[:, o:o + 4] = cloud.rotations.view(torch.int32)
    return buf


def _body(cloud, thickness):
    """The packed rows as a host numpy array: the one copy to the host."""
    return _pack(cloud, thickness).cpu().numpy()


def ply_bytes(cloud, thickness=None):
    """The file ``write_ply`` writes, as ``bytes``: ``ply_header`` and P packed rows of floats.  ``thickness`` None: a 2DGS file
    with two scales; ``thickness = s > 0`` appends ``scale_2 = fp32(log(s))`` for viewers that expect three scales, nothing else
    changes.  The rows are packed on the cloud's device and copied to the host once; P = 0 gives the header alone."""
    return ply_header(cloud.n_surfels, cloud.sh_degree, thickness is not None) + _body(cloud, thickness).tobytes()


def write_ply(path, cloud, thickness=None):
    """Write ``ply_bytes(cloud, thickness)`` to ``path`` (the directory is created).  Nothing is written when an argument is
    refused.  Returns the number of bytes written."""
    header = ply_header(cloud.n_surfels, cloud.sh_degree, thickness is not None)
    body = _body(cloud, thickness)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(header)
        if body.size:
            f.write(memoryview(body).cast("B"))
    return len(header) + body.nbytes


# ---------------------------------------------------------------------------------------------------------- reading

_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
            "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4",
            "double": "<f8", "float64": "<f8"}
_FLOATS = ("float", "float32")
_MAX_HEADER = 1 << 20


def _parse_header(data, path):
    """(elements, body offset, comments): elements = [(name, count, [(property, type)])] in file order."""
    def bad(why):
        return ValueError(f"{_WHO}.read_ply: {path!r}: {why}")

    if data[:4] not in (b"ply\n", b"ply\r"):
        raise bad("not a PLY file (no 'ply' line)")
    end = data.find(b"end_header", 0, _MAX_HEADER)
    nl = data.find(b"\n", end) if end >= 0 else -1
    if end < 0 or nl < 0:
        raise bad("the header has no end_header line")
    lines = [ln.rstrip("\r") for ln in data[:nl].decode("latin-1").split("\n")]     # (a comment may hold any bytes)
    if lines[-1].strip() != "end_header":
        raise bad("the header has no end_header line")
    elements, comments, fmt = [], [], None
    for ln in lines[1:-1]:
        tok = ln.split()
        if not tok:
            continue
        if tok[0] in ("comment", "obj_info"):
            comments.append(ln)
        elif tok[0] == "format":
            if fmt is not None or elements:
                raise bad("a second or misplaced format line")
            fmt = tok[1:]
            if fmt != ["binary_little_endian", "1.0"]:
                raise bad(f"format {' '.join(fmt)!r}: only binary_little_endian 1.0 is read (ASCII and big-endian are out of scope)")
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit():
                raise bad(f"the line {ln!r} names no element count that fits")
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise bad("a property before any element")
            if len(tok) >= 2 and tok[1] == "list":
                if len(tok) != 5 or tok[2] not in _SCALARS or tok[3] not in _SCALARS:
                    raise bad(f"the line {ln!r} is no property")
                elements[-1][2].append((tok[4], "list"))
            elif len(tok) == 3 and tok[1] in _SCALARS:
                elements[-1][2].append((tok[2], tok[1]))
            else:
                raise bad(f"the line {ln!r} is no property")
        else:
            raise bad(f"the header line {ln!r} is not understood")
    if fmt is None:
        raise bad("the header has no format line")
    return elements, nl + 1, comments


def read_ply(path, device="cpu"):
    """(SurfelCloud on ``device``, info) of a 2DGS / 3DGS ``point_cloud.ply``: this module's files and the order those code bases'
    ``save_ply`` uses [RECALLED] both load, since properties are found by name in any order.  ``nx ny nz`` may be absent and are
    ignored; other scalar properties of any PLY type are skipped; ``comment`` / ``obj_info`` lines are skipped; a ``scale_2`` is
    dropped and reported as ``info["dropped_third_scale"] = {"min", "max"}`` (None without one).  The required properties must be
    ``float`` (their words are copied, not converted) and the number of ``f_rest_*`` 3 ((d+1)^2 - 1) for a d in 0..3.  ValueError,
    naming the file: an ASCII or big-endian file, a list property of the vertex element, a missing required property, an element
    before ``vertex``, a body shorter or longer than the header promises, a vertex count that does not fit; elements after
    ``vertex`` are allowed only with zero rows.  Nothing is truncated silently."""
    path = os.fspath(path)

    def bad(why):
        return ValueError(f"{_WHO}.read_ply: {path!r}: {why}")

    with open(path, "rb") as f:
        data = f.read()
    elements, start, comments = _parse_header(data, path)
    if not elements or elements[0][0] != "vertex":
        raise bad("the first element must be 'vertex'" + (f", not {elements[0][0]!r}" if elements else " (the file has none)"))
    for name, count, _ in elements[1:]:
        if count:
            raise bad(f"element {name!r} after 'vertex' has {count} rows; only empty ones are allowed")
    _, P, props = elements[0]
    names = [p for p, _ in props]
    if len(set(names)) != len(names):
        raise bad("a vertex property is named twice")
    if any(t == "list" for _, t in props):
        raise bad(f"the vertex element has a list property ({[p for p, t in props if t == 'list'][0]!r})")
    types = dict(props)
    n_rest = sum(1 for p in names if p.startswith("f_rest_"))
    if n_rest % 3 or (n_rest // 3 + 1) not in SH_COEFFS:
        raise bad(f"{n_rest} f_rest_* properties; 3 ((d+1)^2 - 1) for d in 0..3 is 0, 9, 24 or 45")
    degree = SH_COEFFS[n_rest // 3 + 1]
    need = _names(degree, 2, normals=False)
    for p in need:
        if p not in types:
            raise bad(f"the required property {p!r} is missing")
        if types[p] not in _FLOATS:
            raise bad(f"the property {p!r} is {types[p]}, not float")
    third = types.get("scale_2")
    if third is not None and third not in _FLOATS:
        raise bad(f"the property 'scale_2' is {third}, not float")
    # the words of the float properties are read as uint32: no float load can touch a NaN's payload
    row = np.dtype([(p, "<u4" if t in _FLOATS else _SCALARS[t]) for p, t in props])
    if len(data) - start != P * row.itemsize:
        raise bad(f"the body has {len(data) - start} bytes, the header promises {P} rows of {row.itemsize} = {P * row.itemsize}")
    rows = np.frombuffer(data, row, P, start)
    words = np.empty((P, len(need)), np.uint32)
    for j, p in enumerate(need):
        words[:, j] = rows[p]
    info = {"path": path, "n_surfels": P, "sh_degree": degree, "properties": names, "comments": comments,
            "skipped_properties": [p for p in names if p not in need and p != "scale_2"], "dropped_third_scale": None}
    if third is not None:
        s2 = np.ascontiguousarray(rows["scale_2"]).view(np.float32)
        info["dropped_third_scale"] = {"min": float(s2.min()) if P else None, "max": float(s2.max()) if P else None}
    w = torch.from_numpy(words.view(np.int32)).to(device)              # the one copy to the device
    n = n_rest // 3 + 1
    shs = torch.empty(P, n, 3, dtype=torch.int32, device=w.device)
    shs[:, 0, :] = w[:, 3:6]
    o = 6 + n_rest
    shs[:, 1:, :] = w[:, 6:o].view(P, 3, n - 1).transpose(1, 2)
    parts = (w[:, 0:3], shs, w[:, o:o + 1], w[:, o + 1:o + 3], w[:, o + 3:o + 7])
    return SurfelCloud(*(t.contiguous().view(torch.float32) for t in parts)), info
