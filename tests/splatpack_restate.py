"""csrc/lara_splatpack.h restated in numpy float64, operation by operation: what tests/test_splatpack.py holds the host entries to
(and, through them, tests/test_splatpack_gpu.py the kernels).  Clouds are dicts of float32 arrays (tests/splatio_cases.py).  Every
double operation here is one IEEE operation on the same operands in the same order as csrc/splatpack_ops.h; ``exp`` and ``log`` are
numpy's, which need not agree with the C library's in the last bit: ``alpha_pre`` and ``importance_pre`` return the values before
rounding so that a test can tell a rounding boundary from a mistake."""
import math

import numpy as np

C0 = 0.28209479177387814
ROWS, RECORD = 256, 18
FIELDS = ("centers", "shs", "opacity", "scales", "rotations")
BITS = (11, 10, 11, 11, 10, 11, 8, 8, 8)
_OTHERS = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def canon(v):
    with np.errstate(invalid="ignore"):                   # (a signalling NaN of an invalid row)
        return (np.asarray(v, np.float32) + np.float32(0.0)).astype(np.float32)


def plan(thickness):
    return np.array([np.float32(math.log(float(thickness))), np.float32(float(thickness))], np.float64)


def degree_of(c):
    return {1: 0, 4: 1, 9: 2, 16: 3}[c["shs"].shape[1]]


def pack(x, bits):
    m = float((1 << bits) - 1)
    with np.errstate(invalid="ignore"):
        v = np.floor(np.asarray(x, np.float64) * m + 0.5)
        v = np.where(v >= 0.0, v, 0.0)
    return np.minimum(v, m).astype(np.uint32)


def unit(v, lo, hi):
    v, lo, hi = (np.asarray(a, np.float64) for a in (v, lo, hi))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(hi == lo, 0.0, (v - lo) / (hi - lo))


def bounds(c):
    """(valid [P] uint8, box [6] float32, dropped)."""
    P = c["centers"].shape[0]
    ok = np.ones(P, bool)
    for k in FIELDS:
        ok &= np.isfinite(c[k]).reshape(P, int(np.prod(c[k].shape[1:]))).all(axis=1)
    q = c["rotations"].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        ok &= (n2 > 0.0) & np.isfinite(n2)
    v = canon(c["centers"][ok])
    box = np.concatenate([v.min(axis=0), v.max(axis=0)]) if ok.any() else np.array([np.inf] * 3 + [-np.inf] * 3)
    return ok.astype(np.uint8), box.astype(np.float32), int(P - ok.sum())


def morton(c, box):
    """The 30-bit codes of all rows (meaningless for invalid ones)."""
    v = canon(c["centers"]).astype(np.float64)
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = np.where(hi == lo, 0.0, np.floor((v - lo) / (hi - lo) * 1024.0))
        t = np.where(t >= 0.0, t, 0.0)
    q = np.minimum(t, 1023.0).astype(np.uint64)
    code = np.zeros(v.shape[0], np.uint64)
    for b in range(9, -1, -1):
        for a in range(3):
            code = (code << np.uint64(1)) | ((q[:, a] >> np.uint64(b)) & np.uint64(1))
    return code


def morton_keys(c, valid, box):
    row = np.arange(valid.shape[0], dtype=np.int64)
    return np.where(valid != 0, (morton(c, box).astype(np.int64) << 32) | row, (np.int64(1) << 62) | row)


def alpha(o):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(o, np.float64)))


def alpha_pre(c):
    """alpha 255 + 0.5 of every row: the value whose floor is the alpha byte."""
    return alpha(c["opacity"][:, 0]) * 255.0 + 0.5


def importance_pre(c, pl):
    s = c["scales"].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp((s[:, 0] + s[:, 1]) + pl[0]) * alpha(c["opacity"][:, 0])


def importance_keys(c, valid, pl):
    bits = f32(importance_pre(c, pl)).view(np.uint32).astype(np.int64) & 0x7FFFFFFF
    nan = np.isnan(importance_pre(c, pl))
    bits = np.where(nan, 0x7FC00000, bits)
    row = np.arange(valid.shape[0], dtype=np.int64)
    return np.where(valid != 0, ((0x7FFFFFFF - bits) << 31) | row, (np.int64(1) << 62) | row)


def order_of(keys, dropped):
    return (np.sort(keys) & 0x7FFFFFFF)[:keys.shape[0] - dropped].astype(np.int64)


def values(c, pl):
    """[P, 9] float32: canon(centre), the clamped log scales with s2 as z, canon(k)."""
    P = c["centers"].shape[0]
    s = np.concatenate([c["scales"], np.full((P, 1), np.float32(pl[0]), np.float32)], axis=1)
    with np.errstate(invalid="ignore"):
        s = canon(np.clip(s, np.float32(-20.0), np.float32(20.0)))
    with np.errstate(invalid="ignore"):
        k = canon(f32(0.5 + C0 * c["shs"][:, 0, :].astype(np.float64)))
    return np.concatenate([canon(c["centers"]), s, k], axis=1)


def rotation_words(rot):
    q = rot.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        q = q / n[:, None]
    L = np.argmax(np.abs(q), axis=1)                       # (the first of equal maxima)
    flip = np.take_along_axis(q, L[:, None], 1)[:, 0] < 0.0
    q = np.where(flip[:, None], -q, q)
    rest = np.take_along_axis(q, _OTHERS[L], 1)
    p = pack(rest * 0.70710678118654752 + 0.5, 10)
    return (L.astype(np.uint32) << 30) | (p[:, 0] << 20) | (p[:, 1] << 10) | p[:, 2]


def sh_bytes(c):
    """[P, 3 (n - 1)] uint8 in write_ply's f_rest order."""
    P, n = c["shs"].shape[:2]
    f = c["shs"][:, 1:, :].transpose(0, 2, 1).reshape(P, 3 * (n - 1)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.floor((f / 8.0 + 0.5) * 256.0)
        v = np.where(v >= 0.0, v, 0.0)
    return np.minimum(v, 255.0).astype(np.uint8)


def encode(c, order, pl):
    """(chunks [C,18] float32, words [P_out,4] uint32, sh [P_out,W] uint8) of the rows ``order`` names."""
    P_out = order.shape[0]
    C = (P_out + ROWS - 1) // ROWS
    sel = {k: c[k][order] for k in FIELDS}
    v = values(sel, pl)
    chunks = np.empty((C, RECORD), np.float32)
    words = np.empty((P_out, 4), np.uint32)
    for ch in range(C):
        r = slice(ROWS * ch, min(ROWS * ch + ROWS, P_out))
        lo, hi = v[r].min(axis=0), v[r].max(axis=0)
        for g in range(3):
            chunks[ch, 6 * g:6 * g + 3], chunks[ch, 6 * g + 3:6 * g + 6] = lo[3 * g:3 * g + 3], hi[3 * g:3 * g + 3]
        p = [pack(unit(v[r, j], lo[j], hi[j]), BITS[j]) for j in range(9)]
        words[r, 0] = p[0] << 21 | p[1] << 11 | p[2]
        words[r, 2] = p[3] << 21 | p[4] << 11 | p[5]
        words[r, 3] = p[6] << 24 | p[7] << 16 | p[8] << 8 | pack(alpha(sel["opacity"][r, 0]), 8)
    words[:, 1] = rotation_words(sel["rotations"])
    return chunks, words, sh_bytes(sel)


def lerp(lo, hi, code, bits):
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    return lo + code.astype(np.float64) / float((1 << bits) - 1) * (hi - lo)


def logit(code):
    a = np.clip(code.astype(np.float64), 0.5, 254.5) / 255.0
    return np.log(a / (1.0 - a))


def decode(chunks, words, sh, degree):
    """The decoded cloud as float64 arrays BEFORE the one rounding (``f32`` of each is the stored word)."""
    P_out, n = words.shape[0], (degree + 1) ** 2
    rec = chunks[np.arange(P_out) // ROWS]
    w = words.astype(np.uint32)
    centers = np.stack([lerp(rec[:, 0], rec[:, 3], w[:, 0] >> 21, 11), lerp(rec[:, 1], rec[:, 4], (w[:, 0] >> 11) & 1023, 10),
                        lerp(rec[:, 2], rec[:, 5], w[:, 0] & 2047, 11)], axis=1)
    scales = np.stack([lerp(rec[:, 6], rec[:, 9], w[:, 2] >> 21, 11), lerp(rec[:, 7], rec[:, 10], (w[:, 2] >> 11) & 1023, 10)], axis=1)
    k = np.stack([lerp(rec[:, 12 + a], rec[:, 15 + a], (w[:, 3] >> (24 - 8 * a)) & 255, 8) for a in range(3)], axis=1)
    shs = np.zeros((P_out, n, 3))
    shs[:, 0, :] = (k - 0.5) / C0
    if n > 1:
        shs[:, 1:, :] = (((sh.astype(np.float64) + 0.5) / 256.0 - 0.5) * 8.0).reshape(P_out, 3, n - 1).transpose(0, 2, 1)
    L = (w[:, 1] >> 30).astype(np.int64)
    comps = np.stack([((((w[:, 1] >> s) & 1023).astype(np.float64)) / 1023.0 - 0.5) * 1.4142135623730951 for s in (20, 10, 0)], axis=1)
    total = (comps[:, 0] * comps[:, 0] + comps[:, 1] * comps[:, 1]) + comps[:, 2] * comps[:, 2]
    rest = 1.0 - total
    q = np.zeros((P_out, 4))
    np.put_along_axis(q, _OTHERS[L], comps, 1)
    np.put_along_axis(q, L[:, None], np.sqrt(np.where(rest > 0.0, rest, 0.0))[:, None], 1)
    return {"centers": centers, "shs": shs, "opacity": logit(w[:, 3] & 255)[:, None], "scales": scales, "rotations": q}


def splat_encode(c, order, pl):
    """[P_out, 8] uint32: the 32-byte rows as words."""
    sel = {k: c[k][order] for k in FIELDS}
    P_out = order.shape[0]
    rows = np.empty((P_out, 8), np.uint32)
    rows[:, 0:3] = sel["centers"].view(np.uint32)
    with np.errstate(over="ignore"):
        rows[:, 3:5] = f32(np.exp(sel["scales"].astype(np.float64))).view(np.uint32)
    rows[:, 5] = np.float32(pl[1]).view(np.uint32)
    k = np.clip(f32(0.5 + C0 * sel["shs"][:, 0, :].astype(np.float64)).astype(np.float64), 0.0, 1.0)
    p = pack(k, 8)
    rows[:, 6] = p[:, 0] | p[:, 1] << 8 | p[:, 2] << 16 | pack(alpha(sel["opacity"][:, 0]), 8) << 24
    q = sel["rotations"].astype(np.float64)
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    b = np.clip(np.floor(q / n[:, None] * 128.0 + 128.0 + 0.5), 0.0, 255.0).astype(np.uint32)
    rows[:, 7] = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | b[:, 3] << 24
    return rows


def splat_decode(rows):
    """The decoded cloud (SH degree 0) as float64 BEFORE the one rounding; the centres are the stored words themselves."""
    w = rows.astype(np.uint32)
    with np.errstate(divide="ignore"):
        scales = np.log(np.ascontiguousarray(w[:, 3:5]).view(np.float32).astype(np.float64))
    dc = np.stack([(((w[:, 6] >> (8 * a)) & 255).astype(np.float64) / 255.0 - 0.5) / C0 for a in range(3)], axis=1)
    q = np.stack([(((w[:, 7] >> (8 * i)) & 255).astype(np.float64) - 128.0) / 128.0 for i in range(4)], axis=1)
    return {"centers": np.ascontiguousarray(w[:, 0:3]).view(np.float32).astype(np.float64), "shs": dc[:, None, :],
            "opacity": logit(w[:, 6] >> 24)[:, None], "scales": scales, "rotations": q}


CHUNK_PROPERTIES = ("min_x min_y min_z max_x max_y max_z min_scale_x min_scale_y min_scale_z max_scale_x max_scale_y max_scale_z "
                    "min_r min_g min_b max_r max_g max_b").split()


def compressed_ply_bytes(chunks, words, sh):
    P_out, W = words.shape[0], sh.shape[1]
    lines = ["ply", "format binary_little_endian 1.0", f"element chunk {chunks.shape[0]}"] + [f"property float {p}" for p in CHUNK_PROPERTIES]
    lines += [f"element vertex {P_out}"] + [f"property uint packed_{p}" for p in ("position", "rotation", "scale", "color")]
    if W:
        lines += [f"element sh {P_out}"] + [f"property uchar f_rest_{j}" for j in range(W)]
    head = ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")
    return head + chunks.astype("<f4").tobytes() + words.astype("<u4").tobytes() + sh.astype("u1").tobytes()
