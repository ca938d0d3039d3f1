"""`lara_amd.splatpack` on the CPU: the host entries (the per-row functions of csrc/splatpack_ops.h compiled for the host) against the
numpy float64 restatement of csrc/lara_splatpack.h on every case of tests/splatpack_cases.py; the files, their refusals and
``read``'s sniffing; the round-trip bounds that follow from the formats.  Everything that is an IEEE-exact computation is equal as
integers; the alpha byte and ``.splat``'s importance key go through ``exp`` and may differ by one only where the restatement's value
before the rounding lies within 2^-30 of a rounding boundary, for at most 1e-3 of a case's rows (none did at writing:
profiles/splatpack_parity.txt)."""
import os

import numpy as np
import pytest
import torch

from tests import splatpack_cases as C
from tests import splatpack_restate as S

CASES = C.cases()
IDS = [f"{P}-{d}-{kind}" for P, d, kind in CASES]


def _cloud(c):
    from lara_amd import splatio
    return splatio.SurfelCloud(*(torch.from_numpy(c[k].copy()) for k in C.FIELDS))


def _np(t):
    return t.detach().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_restatement_stays_off_the_rounding_boundaries(case):
    """The seeds' own condition: the restatement alone has (almost) no row whose alpha or importance sits on a boundary."""
    k = C.case(*case)
    ok = k["valid"] != 0
    for near in (C.near_boundary(k["alpha_pre"])[ok], C.near_fp32_boundary(k["importance_pre"])[ok]):
        assert near.sum() <= 1e-3 * max(near.size, 1)
        assert near.sum() == 0                           # (what the seeds were chosen for)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_host_entries_equal_the_restatement(hip_lib, case):
    from lara_amd import splatpack as sp
    P, degree, kind = case
    k = C.case(*case)
    cloud = _cloud(k["cloud"])
    valid, box, dropped = sp.bounds(cloud)
    assert np.array_equal(_np(valid), k["valid"]) and int(dropped) == k["dropped"] and np.array_equal(_bits(_np(box)), _bits(k["box"]))
    if kind == "mixed" and P > 13:
        assert k["dropped"] == 6 and k["valid"][[3, 4, 7, 8, 9, 10, 11, 12, 13]].all()          # -0.0, denormals and the edge rows are kept
    mk = sp.morton_keys(cloud, valid, box)
    assert np.array_equal(_np(mk), k["morton_keys"])
    assert np.array_equal(_np(sp.order_of(mk, k["dropped"])), k["order"])
    ik = _np(sp.importance_keys(cloud, valid, C.THICKNESS))
    off_keys = C.exempt_keys(ik, k["importance_keys"], k["importance_pre"], k["valid"])
    # encode takes the restatement's order: a key on a boundary must not move every later row
    chunks, words, sh = sp.encode(cloud, torch.from_numpy(k["order"]), C.THICKNESS)
    w = _bits(_np(words))
    assert np.array_equal(_bits(_np(chunks)), _bits(k["chunks"])) and np.array_equal(_np(sh), k["sh"])
    assert np.array_equal(w[:, :3], k["words"][:, :3]) and np.array_equal(w[:, 3] >> 8, k["words"][:, 3] >> 8)
    off_alpha = C.exempt_bytes(w[:, 3] & 255, k["words"][:, 3] & 255, k["alpha_pre"][k["order"]])
    rows = sp.splat_encode(cloud, torch.from_numpy(k["splat_order"]), C.THICKNESS)
    r = _bits(_np(rows)).reshape(-1, 8)
    assert np.array_equal(r[:, [0, 1, 2, 5, 7]], k["splat"][:, [0, 1, 2, 5, 7]]) and np.array_equal(r[:, 6] & 0xFFFFFF, k["splat"][:, 6] & 0xFFFFFF)
    off_alpha += C.exempt_bytes(r[:, 6] >> 24, k["splat"][:, 6] >> 24, k["alpha_pre"][k["splat_order"]])
    far, off_words = C.spacing_off(r[:, 3:5].copy().view(np.float32), k["splat"][:, 3:5].copy().view(np.float32))
    assert far == 0
    # the decoders, on the restatement's own words
    dec = sp.decode(torch.from_numpy(k["chunks"]), torch.from_numpy(k["words"].view(np.int32)), torch.from_numpy(k["sh"]), degree)
    sdec = sp.splat_decode(torch.from_numpy(k["splat"].view(np.uint8).reshape(-1, 32)))
    for got, want in ((dec, k["decoded"]), (sdec, k["splat_decoded"])):
        for t, name in zip(got, C.FIELDS):
            far, off = C.spacing_off(_np(t), S.f32(want[name]))
            assert far == 0, name
            off_words += off
            assert bool(torch.isfinite(t).all()) or name == "scales"
    print(f"splatpack parity, host entries against the float64 restatement, P {P}, SH degree {degree}, {kind}: alpha bytes that differ "
          f"{off_alpha}, importance keys that differ {off_keys}, fp32 words (exp scales, decoded words) that differ {off_words}")


def test_the_special_rows_pack_as_the_header_says(hip_lib):
    k = C.case(1000, 1, "mixed")
    at = {int(s): i for i, s in enumerate(k["order"])}
    w = k["words"]
    assert w[at[8], 1] >> 30 == 0 and w[at[11], 1] >> 30 == 0          # equal largest components: the smallest index
    assert w[at[9], 1] >> 30 == 1 and (w[at[9], 1] >> 20) & 1023 < 512          # the largest was negative: w's sign flipped
    assert w[at[12], 3] & 255 == 0 and w[at[13], 3] & 255 == 255
    v = S.values(k["cloud"], k["plan"])
    assert v[7, 3] == 20.0 and v[7, 4] == -20.0 and (v[10, 6] > 1.0) and (v[10, 7] < 0.0)
    so = {int(s): i for i, s in enumerate(k["splat_order"])}
    assert list(k["splat"][so[10], 6].reshape(1).view(np.uint8)[:3]) == [255, 0, 255]          # k clamped to [0, 1] in .splat
    imp = S.f32(k["importance_pre"])[k["splat_order"]]
    assert (np.diff(imp.astype(np.float64)) <= 0).all()          # descending importance
    c = C.case(257, 1, "coincident")
    assert (c["words"][:, 0] == 0).all() and np.array_equal(c["order"], np.arange(257))
    assert (c["chunks"][:, :3] == c["chunks"][:, 3:6]).all() and c["chunks"].shape == (2, 18)


@pytest.mark.parametrize("case", [(1000, 3, "mixed"), (257, 1, "mixed"), (256, 0, "mixed")], ids=str)
def test_the_round_trip_bounds_that_follow_from_the_format(hip_lib, case):
    from lara_amd import splatpack as sp
    P, degree, _ = case
    k = C.case(*case)
    packed = sp.pack(_cloud(k["cloud"]), C.THICKNESS)
    got, info = sp.unpack(packed)
    order, rec = _np(packed.order), _np(packed.chunks)[np.arange(packed.n_surfels) // 256].astype(np.float64)
    src = {f: k["cloud"][f][order] for f in C.FIELDS}
    v = S.values(src, k["plan"]).astype(np.float64)
    one = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    for j, (slot, bits, dec) in enumerate(((0, 11, got.centers[:, 0]), (1, 10, got.centers[:, 1]), (2, 11, got.centers[:, 2]),
                                          (6, 11, got.scales[:, 0]), (7, 10, got.scales[:, 1]))):
        d, col = _np(dec).astype(np.float64), v[:, j if j < 3 else j]
        half = (rec[:, slot + 3] - rec[:, slot]) / (2.0 * ((1 << bits) - 1))
        assert (np.abs(d - col) <= half + one(d)).all(), j
    q = src["rotations"].astype(np.float64)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    L = np.argmax(np.abs(q), axis=1)
    q = np.where(np.take_along_axis(q, L[:, None], 1) < 0, -q, q)
    others = np.take_along_axis(np.abs(_np(got.rotations).astype(np.float64) - q), S._OTHERS[L], 1)
    assert (others <= 1.4142135623730951 / 2046 + 1e-7).all()          # (1e-7: the decoded word's own fp32 rounding)
    rest, back = src["shs"][:, 1:, :].astype(np.float64), _np(got.shs)[:, 1:, :].astype(np.float64)
    inside = (rest >= -4.0) & (rest < 4.0)
    assert (degree == 0 or inside.mean() > 0.99) and (np.abs(back - rest)[inside] <= 8.0 / 512).all()
    a = S.alpha(src["opacity"][:, 0])
    assert (np.abs((_np(packed.words).view(np.uint32)[:, 3] & 255) / 255.0 - a) <= 1.0 / 510 + 1e-12).all()
    assert info["dropped"] == k["dropped"] and info["dropped_third_scale"]["min"] == info["dropped_third_scale"]["max"] == float(np.float32(k["plan"][0]))
    assert all(bool(torch.isfinite(t).all()) for t in got.render_args())          # the logit included: refine can take the cloud


# ------------------------------------------------------------------------------------------------------------------ files

@pytest.mark.parametrize("case", [(1000, 3, "mixed"), (257, 1, "mixed"), (255, 0, "mixed"), (300, 1, "all_invalid"), (0, 1, "mixed")], ids=str)
def test_the_files_are_the_restated_bytes_and_read_back_bit_for_bit(hip_lib, tmp_path, case):
    from lara_amd import splatpack as sp
    P, degree, _ = case
    k = C.case(*case)
    cloud = _cloud(k["cloud"])
    packed = sp.pack(cloud, C.THICKNESS)
    ply, splat = str(tmp_path / "a.compressed.ply"), str(tmp_path / "a.splat")
    assert sp.write(ply, cloud, thickness=C.THICKNESS) == os.path.getsize(ply) and sp.write_splat(splat, cloud, C.THICKNESS) == 32 * packed.n_surfels
    data = open(ply, "rb").read()
    if np.array_equal(_bits(_np(packed.words)), k["words"]):
        assert data == S.compressed_ply_bytes(k["chunks"], k["words"], k["sh"])
    head = S.compressed_ply_bytes(k["chunks"], k["words"], k["sh"])
    cut = head.index(b"end_header\n") + 11
    assert data[:cut] == head[:cut] and len(data) == len(head) and data == sp.compressed_ply_bytes(packed)
    back = sp.read_compressed_ply(ply, packed=True)
    for a, b in ((back.chunks, packed.chunks), (back.words, packed.words), (back.sh, packed.sh)):
        assert a.dtype == b.dtype and a.shape == b.shape and _np(a).tobytes() == _np(b).tobytes()
    assert back.sh_degree == degree
    rows = sp.read_splat(splat, rows=True)
    assert _np(rows).tobytes() == sp.splat_bytes(cloud, C.THICKNESS) == open(splat, "rb").read()
    if np.array_equal(_bits(_np(rows)).reshape(-1, 8), k["splat"]):
        assert _np(rows).tobytes() == k["splat"].tobytes()
    for path, deg in ((ply, degree), (splat, 0)):
        got, info = sp.read(path)
        assert got.n_surfels == packed.n_surfels == info["n_surfels"] and got.sh_degree == deg
    want = sp.unpack(packed)[0]
    for a, b in zip(sp.read(ply)[0].render_args(), want.render_args()):
        assert _np(a).tobytes() == _np(b).tobytes()


def test_read_sniffs_and_a_plain_ply_goes_to_splatio(hip_lib, tmp_path):
    from lara_amd import splatio, splatpack as sp
    k = C.case(257, 1, "mixed")
    cloud = _cloud(k["cloud"])
    path = str(tmp_path / "point_cloud.ply")
    assert sp.write(path, cloud) == len(splatio.ply_bytes(cloud)) and open(path, "rb").read() == splatio.ply_bytes(cloud)
    (a, ia), (b, ib) = sp.read(path), splatio.read_ply(path)
    assert ia == ib
    for x, y in zip(a.render_args(), b.render_args()):
        assert _np(x).tobytes() == _np(y).tobytes()
    other = str(tmp_path / "renamed.ply")                              # a compressed PLY under a plain name: found by its first element
    sp.write_compressed_ply(other, cloud, C.THICKNESS)
    assert sp.read(other)[1]["format"] == "compressed"
    with pytest.raises(ValueError, match="format is"):
        sp.write(path, cloud, format="ksplat")


def test_save_surfels_default_route_is_unchanged(hip_lib, tmp_path):
    from lara_amd import evaluate, splatio, splatpack as sp
    k = C.case(256, 3, "plain")
    cloud = _cloud(k["cloud"])
    a, b, c, d = (str(tmp_path / n) for n in ("a.ply", "b.ply", "c.ply", "d.splat"))
    assert evaluate.save_surfels(a, cloud.render_args()) == evaluate.save_surfels(b, cloud.render_args(), format="ply") == cloud.n_surfels
    assert open(a, "rb").read() == open(b, "rb").read() == splatio.ply_bytes(cloud)
    evaluate.save_surfels(c, cloud.render_args(), format="compressed")
    evaluate.save_surfels(d, cloud.render_args(), format="splat", thickness=2e-3)
    assert open(c, "rb").read() == sp.compressed_ply_bytes(cloud, 1e-3) and open(d, "rb").read() == sp.splat_bytes(cloud, 2e-3)


def test_the_readers_refuse_what_would_make_them_guess(hip_lib, tmp_path):
    from lara_amd import splatpack as sp
    k = C.case(257, 1, "mixed")
    data = sp.compressed_ply_bytes(_cloud(k["cloud"]), C.THICKNESS)
    cut = data.index(b"end_header\n") + 11
    head, body = data[:cut].decode("ascii"), data[cut:]
    variants = {
        "short": data[:-1], "long": data + b"\0", "big": (head.replace("binary_little_endian", "binary_big_endian")).encode() + body,
        "ascii": head.replace("binary_little_endian", "ascii").encode() + body,
        "missing": head.replace("property float max_scale_y\n", "").encode() + body,
        "missing_word": head.replace("property uint packed_scale\n", "").encode() + body,
        "kind": head.replace("property uint packed_color", "property float packed_color").encode() + body,
        "sh_width": head.replace("property uchar f_rest_8\n", "").encode() + body,
        "chunks": head.replace("element chunk 1\n", "element chunk 2\n").encode() + body,
    }
    for name, blob in variants.items():
        path = str(tmp_path / (name + ".ply"))
        with open(path, "wb") as f:
            f.write(blob)
        with pytest.raises(ValueError, match=name + r"\.ply"):
            sp.read(path)
    splat = str(tmp_path / "odd.splat")
    with open(splat, "wb") as f:
        f.write(bytes(33))
    with pytest.raises(ValueError, match=r"odd\.splat.*multiple of the 32-byte row"):
        sp.read(splat)
    with pytest.raises(ValueError, match="thickness"):
        sp.pack(_cloud(k["cloud"]), thickness=0.0)


def test_the_entries_refuse_sizes_and_addresses_they_cannot_take(hip_lib):
    """Before any launch or loop: more than 2^27 rows (a key's row bits, the LDS row index), P_out > P, an SH degree outside 0..3, words
    off a 16-byte boundary, a null pointer."""
    from lara_amd import splatpack as sp
    from lara_amd._native import host_array
    t = torch.zeros(64, dtype=torch.float32)
    five, plan = host_array("p", [t] * 5), host_array("d", [0.0, 1.0])
    a = t.data_ptr()
    assert a % 16 == 0
    assert sp._entry("lara_splatpack_workspace_bytes")((1 << 27) + 1) == -1 and sp._entry("lara_splatpack_workspace_bytes")(1 << 27) > 0
    for dev in ("", "_host"):
        tail = (None,) if dev == "" else ()
        assert sp._entry("lara_splatpack_bounds" + dev)(1, (1 << 27) + 1, five, a, a, a, a, *tail) == -1
        assert sp._entry("lara_splatpack_bounds" + dev)(4, 1, five, a, a, a, a, *tail) == -1
        assert sp._entry("lara_splatpack_morton_keys" + dev)(1 << 40, a, a, a, a, *tail) == -1
        assert sp._entry("lara_splatpack_importance_keys" + dev)(None, 1, a, a, a, a, *tail) == -1
        assert sp._entry("lara_splatpack_encode" + dev)(plan, 1, 2, 3, five, a, a, a, a, *tail) == -1          # P_out > P
        assert sp._entry("lara_splatpack_encode" + dev)(plan, 1, 2, 2, five, a, a, a + 4, a, *tail) == -1          # words off 16 bytes
        assert sp._entry("lara_splatpack_encode" + dev)(plan, 1, 2, 2, five, a, a, a, None, *tail) == -1          # no SH array at degree 1
        assert sp._entry("lara_splatpack_decode" + dev)(1, (1 << 27) + 1, a, a, a, five, *tail) == -1
        assert sp._entry("lara_splatpack_splat_encode" + dev)(plan, 0, 2, 2, five, a, a + 8, *tail) == -1
        assert sp._entry("lara_splatpack_splat_decode" + dev)(2, a, None, *tail) == -1
    with pytest.raises(ValueError, match="2\\^27|order is"):
        sp.encode(_cloud(C.case(1, 1, "plain")["cloud"]), torch.zeros(2, dtype=torch.int64))
