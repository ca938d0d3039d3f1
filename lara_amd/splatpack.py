"""Packing a cloud of surfels for Gaussian-splat viewers (csrc/lara_splatpack.h, csrc/splatpack.hip): the web viewers' compressed PLY
-- 16 bytes per surfel, a 72-byte record of bounds per 256 surfels, 3 (n - 1) bytes of quantised SH per surfel -- and the 32-byte
``.splat`` row, written, read back and decoded into a ``splatio.SurfelCloud`` again.  Both are LOSSY; ``splatio.write_ply`` stays the
bit-exact file.  Opt-in like every module here, imported by nothing on the default routes.

  * ``pack`` / ``unpack``                  a cloud <-> ``PackedCloud`` (chunks, words, sh, order, dropped, sh_degree), on the cloud's device;
  * ``bounds``, ``morton_keys``, ``importance_keys``, ``encode``, ``decode``, ``splat_encode``, ``splat_decode``   the steps, one entry each;
  * ``compressed_ply_bytes`` / ``write_compressed_ply`` / ``read_compressed_ply``;
  * ``splat_bytes`` / ``write_splat`` / ``read_splat``      SH band 0 only;
  * ``write`` / ``read``                   by extension / by sniffing: ``.splat``, a PLY whose first element is ``chunk``, else ``splatio``.

[RECALLED] The formats are the PlayCanvas / SuperSplat compressed PLY and the antimatter15 ``.splat`` as recalled: neither code base is
in the build image, csrc/lara_splatpack.h is their specification here, and parity with the viewers' own readers is unpinned.

A row with a non-finite word in any field, or with a quaternion whose squared norm is 0 or not finite, is dropped and counted
(``dropped``); nothing else is filtered.  The compressed PLY's rows are in Morton order of their centres (30 bits over the box of the
valid centres), ``.splat``'s in descending ``exp(s0 + s1 + s2) alpha``; the keys are sorted with ``torch.sort`` as ``meshbvh`` sorts
its keys, and each key carries its row, so the order is total.  The viewers expect three scales: the third is ``log(thickness)``.

Tensors on the GPU go through the kernels.  Tensors on the host go through the ``*_host`` entries, the same per-row functions
compiled for the CPU (csrc/splatpack_ops.h): the reference the kernels are held to, not a fast path.  The entry points are bound here
and not by rows of ``_native.SIGNATURES``: tests/test_abi_cpu.py pins that table and include/ to a fixed number of functions.

Out of scope: parity with the viewers' own code, the SOG / ``.ksplat`` / SPZ formats, a device-side file parser, gradients through
the quantiser, per-chunk SH bounds.
"""
from __future__ import annotations

import dataclasses
import math
import os

import numpy as np
import torch

from . import splatio
from . import _native
from ._native import host_array

PLAN = 2                                 # csrc/lara_splatpack.h
ROWS = 256                               # rows per chunk
RECORD = 18
MAX_SURFELS = 1 << 27
CHUNK_PROPERTIES = tuple(f"{m}_{a}" for m in ("min", "max") for a in "xyz") + tuple(f"{m}_scale_{a}" for m in ("min", "max") for a in "xyz") + \
    tuple(f"{m}_{a}" for m in ("min", "max") for a in "rgb")
VERTEX_PROPERTIES = ("packed_position", "packed_rotation", "packed_scale", "packed_color")
_WHO = "lara_amd.splatpack"

ENTRY_POINTS = """
l lara_splatpack_workspace_bytes(l)
i lara_splatpack_bounds(i l p*5 s)
i lara_splatpack_bounds_host(i l p*5)
i lara_splatpack_morton_keys(l p*4 s)
i lara_splatpack_morton_keys_host(l p*4)
i lara_splatpack_importance_keys(p l p*4 s)
i lara_splatpack_importance_keys_host(p l p*4)
i lara_splatpack_encode(p i l*2 p*5 s)
i lara_splatpack_encode_host(p i l*2 p*5)
i lara_splatpack_decode(i l p*4 s)
i lara_splatpack_decode_host(i l p*4)
i lara_splatpack_splat_encode(p i l*2 p*3 s)
i lara_splatpack_splat_encode_host(p i l*2 p*3)
i lara_splatpack_splat_decode(l p*2 s)
i lara_splatpack_splat_decode_host(l p*2)
"""
_SIGS = _native._parse_signatures(ENTRY_POINTS)
_workspace = _native.StreamWorkspace()


def _entry(name):
    """The function ``name`` of the loaded library with its types set (once)."""
    fn = getattr(_native.load_library(), name)
    if fn.argtypes is None:
        fn.restype, fn.argtypes = _SIGS[name][0], _SIGS[name][1]
    return fn


def _call_on(name, device, *args):
    """``_native.call_on`` for the entries bound here: the device entry on the device's current stream for tensors on the GPU, its
    ``_host`` twin for tensors on the host; a tensor goes as its ``data_ptr()``, None as NULL."""
    on_gpu = device.type == "cuda"
    name = name if on_gpu else name + "_host"
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
    if on_gpu:
        with torch.cuda.device(device):
            rc = _entry(name)(*a, _native.current_stream(device))
    else:
        rc = _entry(name)(*a)
    if rc != 0:
        _native.check(rc, name)


# ---------------------------------------------------------------------------------------------------------- arguments

def plan(thickness=1e-3):
    """The plan as 2 float64 (numpy): [0] s2 = fl32(log(thickness)), the third log scale; [1] fl32(thickness)."""
    t = float(thickness)
    if not (t > 0 and math.isfinite(t)):
        raise ValueError(f"{_WHO}: thickness must be a finite number > 0, got {thickness!r}")
    return np.array([np.float32(math.log(t)), np.float32(t)], np.float64)


def _fields(cloud):
    """The cloud's five tensors as the kernels take them (a ``SurfelCloud`` or five tensors); P <= 2^27."""
    ts = cloud.render_args() if isinstance(cloud, splatio.SurfelCloud) else cloud
    ts = splatio.check_fields(_WHO, "cloud", [t.detach() for t in ts])
    if ts[0].shape[0] > MAX_SURFELS:
        raise ValueError(f"{_WHO}: at most 2^27 surfels, got {ts[0].shape[0]}")
    return ts, ts[0].device, ts[0].shape[0], splatio.SH_COEFFS[ts[1].shape[1]]


def _row(what, t, shape, dtype, dev):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{_WHO}: {what} is a contiguous {dtype} tensor {list(shape)} on {dev}")
    return t


def _plan_row(p):
    row = np.asarray(p, np.float64)
    if row.shape != (PLAN,):
        raise ValueError(f"{_WHO}: a plan is {PLAN} doubles (splatpack.plan)")
    return host_array("d", row.tolist())


def sh_width(sh_degree):
    return 3 * ((int(sh_degree) + 1) ** 2 - 1)


# ---------------------------------------------------------------------------------------------------------- the steps

@torch.no_grad()
def bounds(cloud, out=None):
    """(valid [P] uint8, box [6] fp32 = (lo xyz, hi xyz) over the valid centres, dropped [1] int64), on the cloud's device.  No host
    read.  A cloud without a valid row has the box (+inf, -inf).  ``out``: the validity bytes to fill."""
    ts, dev, P, degree = _fields(cloud)
    valid = torch.empty(P, dtype=torch.uint8, device=dev) if out is None else _row("valid", out, (P,), torch.uint8, dev)
    box = torch.empty(6, dtype=torch.float32, device=dev)
    dropped = torch.zeros(1, dtype=torch.int64, device=dev)
    if P == 0:                               # (an empty tensor has no address to hand over; nothing is launched)
        box[:3], box[3:] = math.inf, -math.inf
        return valid, box, dropped
    ws = None
    if dev.type == "cuda":
        n = int(_entry("lara_splatpack_workspace_bytes")(P))
        if n < 0:
            _native.check(n, "lara_splatpack_workspace_bytes")
        ws = _workspace(dev, n)
    _call_on("lara_splatpack_bounds", dev, degree, P, host_array("p", ts), valid, box, dropped, ws)
    return valid, box, dropped


@torch.no_grad()
def morton_keys(cloud, valid, box, out=None):
    """keys [P] int64: ``morton << 32 | row`` for a valid row, ``1 << 62 | row`` for an invalid one."""
    ts, dev, P, _ = _fields(cloud)
    _row("valid", valid, (P,), torch.uint8, dev)
    _row("box", box, (6,), torch.float32, dev)
    keys = torch.empty(P, dtype=torch.int64, device=dev) if out is None else _row("keys", out, (P,), torch.int64, dev)
    if P:
        _call_on("lara_splatpack_morton_keys", dev, P, ts[0], valid, box, keys)
    return keys


@torch.no_grad()
def importance_keys(cloud, valid, thickness=1e-3, out=None):
    """keys [P] int64: ``(0x7FFFFFFF - bits(fl32(exp(s0 + s1 + s2) alpha))) << 31 | row``; invalid rows as in ``morton_keys``."""
    ts, dev, P, _ = _fields(cloud)
    _row("valid", valid, (P,), torch.uint8, dev)
    keys = torch.empty(P, dtype=torch.int64, device=dev) if out is None else _row("keys", out, (P,), torch.int64, dev)
    if P:
        _call_on("lara_splatpack_importance_keys", dev, _plan_row(plan(thickness)), P, ts[2], ts[3], valid, keys)
    return keys


def order_of(keys, dropped):
    """The source rows of the output rows from the keys: sorted ascending (``torch.sort``), the low 31 bits, the first
    ``P - dropped``.  ``dropped`` is an int (the caller's one host read)."""
    return (torch.sort(keys)[0] & 0x7FFFFFFF)[:keys.shape[0] - int(dropped)].contiguous()


@torch.no_grad()
def encode(cloud, order, thickness=1e-3, out=None):
    """(chunks [C,18] fp32, words [P_out,4] int32, sh [P_out, 3 (n - 1)] uint8) of the rows ``order`` [P_out] int64 names, chunk by
    chunk of 256.  ``out``: the three tensors to fill (contiguous, words on a 16-byte boundary) instead of new ones."""
    ts, dev, P, degree = _fields(cloud)
    if not isinstance(order, torch.Tensor) or order.dim() != 1 or order.shape[0] > P:
        raise ValueError(f"{_WHO}: order is an int64 tensor [P_out] with P_out <= {P}")
    P_out = order.shape[0]
    _row("order", order, (P_out,), torch.int64, dev)
    C, W = (P_out + ROWS - 1) // ROWS, sh_width(degree)
    if out is None:
        out = (torch.empty(C, RECORD, dtype=torch.float32, device=dev), torch.empty(P_out, 4, dtype=torch.int32, device=dev),
               torch.empty(P_out, W, dtype=torch.uint8, device=dev))
    chunks, words, sh = (_row(w, t, s, d, dev) for w, t, s, d in zip(("chunks", "words", "sh"), out, ((C, RECORD), (P_out, 4), (P_out, W)),
                                                                     (torch.float32, torch.int32, torch.uint8)))
    if P_out:
        _call_on("lara_splatpack_encode", dev, _plan_row(plan(thickness)), degree, P, P_out, host_array("p", ts), order, chunks, words,
                 sh if W else None)
    return chunks, words, sh


def _new_cloud(P_out, degree, dev):
    n = (degree + 1) ** 2
    return [torch.empty(s, dtype=torch.float32, device=dev) for s in ((P_out, 3), (P_out, n, 3), (P_out, 1), (P_out, 2), (P_out, 4))]


def _out_fields(out, P_out, degree, dev):
    ts = splatio.check_fields(_WHO, "out", out)
    if ts[0].shape[0] != P_out or splatio.SH_COEFFS[ts[1].shape[1]] != degree or ts[0].device != dev:
        raise ValueError(f"{_WHO}: out is five tensors of {P_out} rows of SH degree {degree} on {dev}")
    return ts


@torch.no_grad()
def decode(chunks, words, sh, sh_degree, out=None):
    """The five tensors of the decoded cloud (``out``: five tensors to fill)."""
    dev, P_out, degree = words.device, words.shape[0], int(sh_degree)
    C, W = (P_out + ROWS - 1) // ROWS, sh_width(degree)
    _row("chunks", chunks, (C, RECORD), torch.float32, dev)
    _row("words", words, (P_out, 4), torch.int32, dev)
    _row("sh", sh, (P_out, W), torch.uint8, dev)
    ts = _new_cloud(P_out, degree, dev) if out is None else _out_fields(out, P_out, degree, dev)
    if P_out:
        _call_on("lara_splatpack_decode", dev, degree, P_out, chunks, words, sh if W else None, host_array("p", ts))
    return ts


@torch.no_grad()
def splat_encode(cloud, order, thickness=1e-3, out=None):
    """rows [P_out, 32] uint8: the ``.splat`` rows of the source rows ``order`` names (SH band 0 only)."""
    ts, dev, P, degree = _fields(cloud)
    if not isinstance(order, torch.Tensor) or order.dim() != 1 or order.shape[0] > P:
        raise ValueError(f"{_WHO}: order is an int64 tensor [P_out] with P_out <= {P}")
    P_out = order.shape[0]
    _row("order", order, (P_out,), torch.int64, dev)
    rows = torch.empty(P_out, 32, dtype=torch.uint8, device=dev) if out is None else _row("rows", out, (P_out, 32), torch.uint8, dev)
    if P_out:
        _call_on("lara_splatpack_splat_encode", dev, _plan_row(plan(thickness)), degree, P, P_out, host_array("p", ts), order, rows)
    return rows


@torch.no_grad()
def splat_decode(rows, out=None):
    """The five tensors (SH degree 0) of ``.splat`` rows [P_out, 32] uint8."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError(f"{_WHO}: rows is a uint8 tensor [P_out, 32]")
    dev, P_out = rows.device, rows.shape[0]
    _row("rows", rows, (P_out, 32), torch.uint8, dev)
    ts = _new_cloud(P_out, 0, dev) if out is None else _out_fields(out, P_out, 0, dev)
    if P_out:
        _call_on("lara_splatpack_splat_decode", dev, P_out, rows, host_array("p", ts))
    return ts


# ---------------------------------------------------------------------------------------------------------- pack, unpack

@dataclasses.dataclass
class PackedCloud:
    """A packed cloud: ``chunks`` [C,18] fp32, ``words`` [P_out,4] uint32 (held as int32), ``sh`` [P_out, 3 (n - 1)] uint8, ``order``
    [P_out] int64 (the source row of every packed row; None for a cloud read from a file), ``dropped`` (int) and ``sh_degree``."""
    chunks: torch.Tensor
    words: torch.Tensor
    sh: torch.Tensor
    order: torch.Tensor | None
    dropped: int
    sh_degree: int

    @property
    def n_surfels(self):
        return self.words.shape[0]

    @property
    def device(self):
        return self.words.device


def pack(cloud, thickness=1e-3):
    """``cloud`` as a ``PackedCloud`` on its device: bounds, Morton keys, ``torch.sort``, encode.  One host read (the dropped
    count, needed to size the outputs)."""
    valid, box, dropped = bounds(cloud)
    keys = morton_keys(cloud, valid, box)
    gone = int(dropped)
    order = order_of(keys, gone)
    ts, _, _, degree = _fields(cloud)
    chunks, words, sh = encode(ts, order, thickness)
    return PackedCloud(chunks, words, sh, order, gone, degree)


def unpack(packed):
    """(SurfelCloud, info): the decoded cloud on ``packed``'s device; ``info["dropped_third_scale"]`` is the range of the third
    scale, which a surfel does not have (None for an empty cloud), as ``splatio.read_ply`` reports a ``scale_2``."""
    ts = decode(packed.chunks, packed.words, packed.sh, packed.sh_degree)
    third = None
    if packed.n_surfels:
        third = {"min": float(packed.chunks[:, 8].min()), "max": float(packed.chunks[:, 11].max())}
    return splatio.SurfelCloud(*ts), {"n_surfels": packed.n_surfels, "sh_degree": packed.sh_degree, "dropped": packed.dropped,
                                      "dropped_third_scale": third}


# ---------------------------------------------------------------------------------------------------------- the compressed PLY

def compressed_ply_header(P_out, sh_degree):
    C, W = (int(P_out) + ROWS - 1) // ROWS, sh_width(sh_degree)
    lines = ["ply", "format binary_little_endian 1.0", f"element chunk {C}"] + [f"property float {p}" for p in CHUNK_PROPERTIES]
    lines += [f"element vertex {int(P_out)}"] + [f"property uint {p}" for p in VERTEX_PROPERTIES]
    if W:
        lines += [f"element sh {int(P_out)}"] + [f"property uchar f_rest_{j}" for j in range(W)]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def _as_packed(cloud_or_packed, thickness):
    return cloud_or_packed if isinstance(cloud_or_packed, PackedCloud) else pack(cloud_or_packed, thickness)


def compressed_ply_bytes(cloud_or_packed, thickness=1e-3):
    """The compressed PLY as ``bytes``: the header, the chunk records, the rows' four words, the SH bytes."""
    p = _as_packed(cloud_or_packed, thickness)
    return compressed_ply_header(p.n_surfels, p.sh_degree) + b"".join(t.cpu().numpy().tobytes() for t in (p.chunks, p.words, p.sh))


def _write(path, data):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def write_compressed_ply(path, cloud_or_packed, thickness=1e-3):
    """Write ``compressed_ply_bytes`` to ``path`` (the directory is created).  Returns the number of bytes written."""
    return _write(path, compressed_ply_bytes(cloud_or_packed, thickness))


def read_compressed_ply(path, device="cpu", packed=False):
    """(SurfelCloud on ``device``, info) of a compressed PLY; ``packed=True``: the ``PackedCloud`` itself, undecoded.  ValueError,
    naming the file: an ASCII or big-endian file, elements other than ``chunk`` (18 float), ``vertex`` (4 uint) and an optional ``sh``
    (9, 24 or 45 uchar) in that order with the properties this module writes, counts that do not agree, a body shorter or longer than
    the header promises."""
    path = os.fspath(path)

    def bad(why):
        return ValueError(f"{_WHO}.read_compressed_ply: {path!r}: {why}")

    with open(path, "rb") as f:
        data = f.read()
    elements, start, _ = splatio._parse_header(data, path)
    names = [e[0] for e in elements]
    if names not in (["chunk", "vertex"], ["chunk", "vertex", "sh"]):
        raise bad(f"the elements are {names}; a compressed PLY has chunk, vertex and optionally sh")
    for (name, _, props), want, kinds in zip(elements, (CHUNK_PROPERTIES, VERTEX_PROPERTIES), (("float", "float32"), ("uint", "uint32"))):
        for p in want:
            if p not in [q for q, _ in props]:
                raise bad(f"the required property {p!r} of element {name!r} is missing")
        if [q for q, _ in props] != list(want) or any(t not in kinds for _, t in props):
            raise bad(f"element {name!r} must hold exactly the {kinds[0]} properties {list(want)} in this order")
    (_, C, _), (_, P_out, _) = elements[:2]
    W = 0
    if len(elements) == 3:
        _, n_sh, props = elements[2]
        W = len(props)
        if W not in (9, 24, 45) or [q for q, _ in props] != [f"f_rest_{j}" for j in range(W)] or any(t not in ("uchar", "uint8") for _, t in props):
            raise bad(f"element 'sh' must hold 9, 24 or 45 uchar properties f_rest_0.., has {W}")
        if n_sh != P_out:
            raise bad(f"element 'sh' has {n_sh} rows, 'vertex' {P_out}")
    if C != (P_out + ROWS - 1) // ROWS or P_out > MAX_SURFELS:
        raise bad(f"{C} chunks do not hold {P_out} rows of {ROWS} per chunk")
    sizes = (C * RECORD * 4, P_out * 16, P_out * W)
    if len(data) - start != sum(sizes):
        raise bad(f"the body has {len(data) - start} bytes, the header promises {sum(sizes)}")
    o1, o2 = start + sizes[0], start + sizes[0] + sizes[1]
    chunks = torch.from_numpy(np.frombuffer(data, "<f4", C * RECORD, start).reshape(C, RECORD).copy())
    words = torch.from_numpy(np.frombuffer(data, "<i4", P_out * 4, o1).reshape(P_out, 4).copy())
    sh = torch.from_numpy(np.frombuffer(data, "u1", P_out * W, o2).reshape(P_out, W).copy())
    p = PackedCloud(chunks.to(device), words.to(device), sh.to(device), None, 0, {0: 0, 9: 1, 24: 2, 45: 3}[W])
    if packed:
        return p
    cloud, info = unpack(p)
    return cloud, dict(info, path=path, format="compressed")


# ---------------------------------------------------------------------------------------------------------- .splat

def splat_rows(cloud, thickness=1e-3):
    """(rows [P_out, 32] uint8 on the cloud's device, order, dropped): bounds, importance keys, ``torch.sort``, encode."""
    valid, _, dropped = bounds(cloud)
    gone = int(dropped)
    order = order_of(importance_keys(cloud, valid, thickness), gone)
    return splat_encode(cloud, order, thickness), order, gone


def splat_bytes(cloud, thickness=1e-3):
    return splat_rows(cloud, thickness)[0].cpu().numpy().tobytes()


def write_splat(path, cloud, thickness=1e-3):
    """Write the cloud's ``.splat`` file (no header: P_out rows of 32 bytes).  Returns the number of bytes written."""
    return _write(path, splat_bytes(cloud, thickness))


def read_splat(path, device="cpu", rows=False):
    """(SurfelCloud of SH degree 0 on ``device``, info) of a ``.splat`` file; ``rows=True``: the [P_out, 32] uint8 rows, undecoded.
    ValueError, naming the file, where the size is not a multiple of 32."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        data = f.read()
    if len(data) % 32:
        raise ValueError(f"{_WHO}.read_splat: {path!r}: {len(data)} bytes are not a multiple of the 32-byte row")
    t = torch.from_numpy(np.frombuffer(data, "u1").reshape(-1, 32).copy()).to(device)
    if rows:
        return t
    third = None
    if t.shape[0]:
        logs = torch.log(t.cpu().view(torch.float32)[:, 5])
        third = {"min": float(logs.min()), "max": float(logs.max())}
    return splatio.SurfelCloud(*splat_decode(t)), {"path": path, "format": "splat", "n_surfels": t.shape[0], "sh_degree": 0,
                                                   "dropped_third_scale": third}


# ---------------------------------------------------------------------------------------------------------- by extension, by sniffing

def write(path, cloud, format=None, thickness=None):
    """Write ``cloud`` by ``format`` ("ply", "compressed", "splat") or, when None, by the extension of ``path``: ``.splat``,
    ``.compressed.ply``, anything else ``splatio.write_ply`` (bit-exact; its ``thickness`` None writes two scales).  The packed formats
    need a thickness: 1e-3 when None."""
    name = os.fspath(path).lower()
    fmt = format or ("splat" if name.endswith(".splat") else "compressed" if name.endswith(".compressed.ply") else "ply")
    if fmt == "ply":
        return splatio.write_ply(path, cloud, thickness)
    if fmt not in ("compressed", "splat"):
        raise ValueError(f'{_WHO}: format is "ply", "compressed" or "splat", not {format!r}')
    return (write_compressed_ply if fmt == "compressed" else write_splat)(path, cloud, 1e-3 if thickness is None else thickness)


def read(path, device="cpu"):
    """(SurfelCloud, info) of any of the three files: ``.splat`` by its extension (the format has no signature), a PLY whose first
    element is ``chunk`` as a compressed PLY, anything else through ``splatio.read_ply``."""
    path = os.fspath(path)
    if path.lower().endswith(".splat"):
        return read_splat(path, device)
    with open(path, "rb") as f:
        head = f.read(splatio._MAX_HEADER)
    if head[:3] == b"ply":
        for ln in head.split(b"\n"):
            tok = ln.split()
            if tok[:1] == [b"element"]:
                if tok[1:2] == [b"chunk"]:
                    return read_compressed_ply(path, device)
                break
    return splatio.read_ply(path, device)
