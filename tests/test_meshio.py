"""include/lara_meshio.h without a GPU: the header's constants held to the module's, the formatting routines of csrc/fmt9g.h (through
the library's host-only entries) held to Python's own "%.9g" and str(), the cases of tests/meshio_cases.py, the PLY restatement
through read_ply, the header text, and the refusals.  tests/test_meshio_gpu.py holds the kernels to write_obj's bytes and to the
restatement.  Every comparison here is an equality of bytes or bits: the routines are exact, so there is no bar."""
import ctypes

import numpy as np
import pytest
import torch

from lara_amd import mesh, meshio
from tests import meshio_cases as C
from tests import meshio_restate as R

FILL = 0xA5


def test_header_constants_equal_the_modules():
    """The macros of include/lara_meshio.h pinned, equal to the module's, and consistent with one another."""
    from tests import test_abi_cpu as abi
    text = abi.header_texts()["lara_meshio.h"]
    for macro, value in (("BLOCK_LINES", 256), ("MAX_F32_TOKEN", 15), ("MAX_U32_TOKEN", 10), ("MAX_VERTEX_LINE", 98), ("MAX_FACE_LINE", 35),
                         ("PLY_FACE_ROW", 13), ("MAX_VERTICES", 2 ** 31 - 1), ("MAX_TRIANGLES", (2 ** 31 - 1) // 3),
                         ("MAX_INDEX", 2 ** 31 - 2), ("ERR_INDEX", 1)):
        assert f"#define LARA_MESHIO_{macro} {value}\n" in text
    assert (meshio.BLOCK_LINES, meshio.MAX_F32_TOKEN, meshio.MAX_U32_TOKEN, meshio.MAX_VERTEX_LINE, meshio.MAX_FACE_LINE) == (256, 15, 10, 98, 35)
    assert (meshio.PLY_FACE_ROW, meshio.MAX_VERTICES, meshio.MAX_TRIANGLES, meshio.MAX_INDEX) == (13, 2 ** 31 - 1, (2 ** 31 - 1) // 3, 2 ** 31 - 2)
    assert meshio.MAX_VERTEX_LINE == 1 + 6 * (1 + meshio.MAX_F32_TOKEN) + 1 and meshio.MAX_FACE_LINE == 1 + 3 * (1 + meshio.MAX_U32_TOKEN) + 1
    assert 3 * meshio.MAX_TRIANGLES < 2 ** 31 <= 3 * (meshio.MAX_TRIANGLES + 1) and C.MAX_INDEX == meshio.MAX_INDEX


def _format_f32(lib, bits):
    """(tokens as an 'S16' array, lengths) of fp32 bit patterns through the host entry; nothing beyond a length may be written."""
    v = np.ascontiguousarray(bits, np.uint32)
    out = np.full((len(v), 16), FILL, np.uint8)
    n = np.full(len(v), -7, np.int32)
    assert lib.lara_meshio_format_f32_host(len(v), v.ctypes.data, out.ctypes.data, n.ctypes.data) == 0
    assert n.min() >= 1 and n.max() <= meshio.MAX_F32_TOKEN
    beyond = np.arange(16)[None, :] >= n[:, None]
    assert (out[beyond] == FILL).all()
    out[beyond] = 0
    return out.view("S16")[:, 0], n


def _format_u32(lib, values):
    v = np.ascontiguousarray(values, np.uint32)
    out = np.full((len(v), 10), FILL, np.uint8)
    n = np.full(len(v), -7, np.int32)
    assert lib.lara_meshio_format_u32_host(len(v), v.ctypes.data, out.ctypes.data, n.ctypes.data) == 0
    beyond = np.arange(10)[None, :] >= n[:, None]
    assert (out[beyond] == FILL).all()
    out[beyond] = 0
    return out.view("S10")[:, 0], n


def _assert_tokens(got, n, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} tokens differ, the first {got[bad[0]]!r} for {want[bad[0]]!r}"
    assert np.array_equal(n, np.char.str_len(want))


def test_format_f32_equals_percent_9g_on_the_special_values(hip_lib):
    s = C.float_specials()
    got, n = _format_f32(hip_lib, s)
    _assert_tokens(got, n, R.fmt9g_of_bits(s), "special values")
    for b in s[::97]:                                   # the vectorised restatement is the scalar one
        assert R.fmt9g_of_bits([b])[0].decode() == R.fmt9g(np.array(b, np.uint32).view(np.float32))
    one = lambda x: _format_f32(hip_lib, C.bits_of(np.float32(x)).reshape(1))[0][0].decode()
    # the issue's tables, by hand
    assert [one(x) for x in (1234567.875, 1292052.125, 1761752.875)] == ["1234567.88", "1292052.12", "1761752.88"]
    by_bits = lambda b: _format_f32(hip_lib, np.array([b], np.uint32))[0][0].decode()
    assert by_bits(0x19416d9a) == "1e-23" and by_bits(0x56b5e621) == "1e+14"
    assert [by_bits(b) for b in (0x0da24260, 0x0f4ad2f8, 0x10fd87b6, 0x26901d7d)] == ["1e-30", "1e-29", "1e-28", "1e-15"]
    assert one(C.LONGEST) == "-7.77995488e+32" and one(0.0) == "0" and one(-0.0) == "-0" and one(float("inf")) == "inf"
    assert one(float("-inf")) == "-inf" and by_bits(0xffc00000) == "nan" and by_bits(0x7fc00000) == "nan"
    assert one(999999936.0) == "999999936" and one(1e9) == "1e+09" and one(1e-4) == "9.99999975e-05" and one(np.nextafter(np.float32(1e-4), np.float32(1))) == "0.000100000005"
    assert one(1e-45) == "1.40129846e-45" and one(3.4028234663852886e38) == "3.40282347e+38" and one(16777216.0) == "16777216"


def test_format_f32_equals_percent_9g_on_two_million_random_bit_patterns(hip_lib):
    bits = np.random.default_rng(9).integers(0, 2 ** 32, 2_000_000, dtype=np.uint64).astype(np.uint32)
    got, n = _format_f32(hip_lib, bits)
    _assert_tokens(got, n, R.fmt9g_of_bits(bits), "random bit patterns")


def test_format_u32_equals_str(hip_lib):
    rng = np.random.default_rng(10)
    v = np.concatenate([C.index_crossings() + 1, [0, 1, 2 ** 32 - 1, 2 ** 31 - 1, 2 ** 31], rng.integers(0, 2 ** 32, 50_000),
                        rng.integers(0, 10, 50_000) ** rng.integers(1, 10, 50_000)]).astype(np.uint32)
    got, n = _format_u32(hip_lib, v)
    _assert_tokens(got, n, np.array([str(int(x)) for x in v], "S10"), "indices")
    assert n.max() == 10 and n.min() == 1


def test_the_cases_are_what_the_tests_rely_on():
    s = C.float_specials()
    have = set(int(b) for b in s)
    assert s.dtype == np.uint32 and len(have) > 2500
    assert {0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000} <= have
    assert all(int(C.bits_of(np.float32(np.ldexp(1.0, e)))) in have for e in range(-149, 128))
    assert set(C.CARRY_CASES) <= have                                     # rounding that carries into the next power of ten
    f = s.view(np.float32)
    with np.errstate(invalid="ignore"):
        assert (f == np.float32(999999936.0)).any() and (f == np.float32(1e9)).any() and (f == np.float32(1e-4)).any()
        assert (f == np.nextafter(np.float32(1e-4), np.float32(1))).any()      # 0.000100000005: the first float in fixed notation
    tokens = [R.fmt9g(x) for x in f]
    assert max(map(len, tokens)) == 15 == meshio.MAX_F32_TOKEN and "0" in tokens and "-7.77995488e+32" in tokens
    # the ties: exactly representable, exactly half a unit of the ninth digit, and both rounding directions occur
    t = C.ties().view(np.float32).astype(np.float64)
    assert len(t) >= 1000 and np.all((t >= 1e6) & (t < 1e7)) and np.all(t * 8 == np.round(t * 8)) and np.all((t * 8) % 2 == 1)
    hundredths = t * 100
    assert np.all(hundredths - np.floor(hundredths) == 0.5)
    went_up = np.array([float(R.fmt9g(x)) > x for x in t])
    assert 400 < went_up.sum() < len(t) - 400
    even = np.array([int(round(float(R.fmt9g(x)) * 100)) % 2 == 0 for x in t])
    assert even.all()
    assert C.SIZES == [(0, 0), (1, 0), (0, 1), (3, 1), (255, 254), (256, 256), (257, 300), (1000, 2100)]
    v, tr, c = C.widest()
    assert len(v) == 256 == len(tr) and R.fmt9g(v[0, 0]) == "-7.77995488e+32" and int(tr.max()) == 2 ** 31 - 2
    assert len("v" + 6 * (" " + R.fmt9g(v[0, 0])) + "\n") == meshio.MAX_VERTEX_LINE and len("f" + 3 * (" %d" % (tr[0, 0] + 1)) + "\n") == meshio.MAX_FACE_LINE
    v, tr, c = C.narrowest()
    assert c is None and not v.any() and not tr.any() and len(v) > 256
    x = C.index_crossings() + 1
    digits = np.char.str_len(x.astype(str))
    assert set(digits) == set(range(1, 11)) and all((10 ** k - 1 in x) and (10 ** k in x) for k in range(1, 10)) and 2 ** 31 - 1 in x
    sv, st, sc = C.specials_mesh()
    for col in list(sv.T) + list(sc.T):                                   # every special value in every position of a line
        assert set(col.view(np.uint32).tolist()) == have
    e = C.color_edges()
    u = R.color_u8(e)
    flat, uf = e.reshape(-1), u.reshape(-1)
    with np.errstate(invalid="ignore"):
        assert uf[np.isnan(flat)].max() == 0 and uf[flat < 0].max() == 0 and uf[flat > 1].min() == 255
    for k in (0, 127, 254):                                               # the rule steps between the neighbours of (k + 0.5) / 255
        mid = np.float32((k + 0.5) / 255.0)
        lo, hi = np.nextafter(mid, np.float32(-1)), np.nextafter(mid, np.float32(2))
        assert R.color_u8(lo) == k and R.color_u8(hi) == k + 1 and (flat == lo).any() and (flat == mid).any() and (flat == hi).any()
    for nv, nt in C.SIZES:
        mv, mt, mc, mn = C.mesh(nv, nt)
        assert mv.shape == (nv, 3) and mt.shape == (nt, 3) and mc.shape == (nv, 3) and mn.shape == (nv, 3) and mt.dtype == np.int64
        assert nt == 0 or (0 <= mt.min() and mt.max() <= C.MAX_INDEX)


def test_header_text_by_hand():
    assert meshio.ply_header(3, 1) == (b"ply\nformat binary_little_endian 1.0\ncomment lara_amd.meshio\nelement vertex 3\nproperty float x\n"
                                       b"property float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
    assert meshio.ply_header(278260, 556516, normals=True, colors=True) == (
        b"ply\nformat binary_little_endian 1.0\ncomment lara_amd.meshio\nelement vertex 278260\nproperty float x\nproperty float y\n"
        b"property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
        b"property uchar blue\nelement face 556516\nproperty list uchar int vertex_indices\nend_header\n")
    for n in (False, True):
        for c in (False, True):
            assert meshio.ply_header(7, 9, n, c) == R.ply_header(7, 9, n, c) and len(meshio.ply_header(7, 9, n, c)) <= 307


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_restatement_round_trips_through_read_ply(tmp_path, with_normals, with_colors):
    for nv, nt in C.SIZES:
        v, t, c, n = C.mesh(nv, nt)
        if nv:
            v[0] = C.float_specials()[:3].view(np.float32)              # bits survive, a negative zero among them
        data = R.ply_bytes(v, t, c if with_colors else None, n if with_normals else None)
        assert len(data) == len(R.ply_header(nv, nt, with_normals, with_colors)) + nv * (12 + 12 * with_normals + 3 * with_colors) + 13 * nt
        path = tmp_path / f"m{nv}_{nt}.PLY"
        path.write_bytes(data)
        rv, rt, rc = meshio.read_mesh(str(path))
        assert rv.dtype == np.float32 and rv.tobytes() == v.tobytes() and rt.dtype == np.int64 and np.array_equal(rt, t)
        if with_colors:
            assert rc.dtype == np.float32 and np.array_equal(rc, R.color_u8(c).astype(np.float32) / np.float32(255))
        else:
            assert rc is None
    bad = tmp_path / "bad.ply"
    bad.write_bytes(data[:-1])                                           # a byte short
    with pytest.raises(ValueError):
        meshio.read_ply(str(bad))
    bad.write_bytes(data.replace(b"comment lara_amd.meshio\n", b""))     # a header this module does not write
    with pytest.raises(ValueError):
        meshio.read_ply(str(bad))
    bad.write_bytes(data.replace(b"binary_little_endian", b"ascii"))
    with pytest.raises(ValueError):
        meshio.read_ply(str(bad))


def test_read_mesh_dispatches_obj_to_read_obj(tmp_path):
    v, t, c, _ = C.mesh(3, 1)
    t = t % 3
    path = str(tmp_path / "m.OBJ")
    mesh.write_obj(path, v, t, c)
    rv, rt, rc = meshio.read_mesh(path)
    assert rv.tobytes() == v.tobytes() and np.array_equal(rt, t) and rc.tobytes() == c.tobytes()
    with pytest.raises(ValueError):
        meshio.read_mesh(str(tmp_path / "m.stl"))


def test_refusals(hip_lib, tmp_path):
    """Negative sizes, sizes out of range, null pointers and a bad index width come back as LARA2DGS_E_INVALID (-1) from host code,
    before any pointer is used; empty inputs are no-ops; the python layer refuses CPU tensors, unknown extensions and OBJ normals."""
    L = hip_lib
    big_v, big_t = 2 ** 31, (2 ** 31 - 1) // 3 + 1
    assert L.lara_meshio_obj_workspace_bytes(-1, 0) == -1 and L.lara_meshio_obj_workspace_bytes(0, -1) == -1
    assert L.lara_meshio_obj_workspace_bytes(big_v, 0) == -1 and L.lara_meshio_obj_workspace_bytes(0, big_t) == -1
    assert L.lara_meshio_obj_workspace_bytes(0, 0) == 8 and L.lara_meshio_obj_workspace_bytes(257, 256) == 8 * (2 + 1 + 1)
    assert L.lara_meshio_obj_workspace_bytes(big_v - 1, big_t - 1) == 8 * (2 ** 23 + -(-(big_t - 1) // 256) + 1)
    assert L.lara_meshio_obj_lengths(-1, None, None, 0, None, 4, None, None) == -1
    assert L.lara_meshio_obj_lengths(4, None, None, 0, None, 4, None, None) == -1              # null pointers
    assert L.lara_meshio_obj_lengths(0, None, None, 4, None, 4, None, None) == -1
    assert L.lara_meshio_obj_lengths(0, None, None, 4, None, 2, None, None) == -1              # 2-byte indices
    assert L.lara_meshio_obj_lengths(0, None, None, 0, None, 8, None, None) == 0               # an empty mesh: a no-op
    assert L.lara_meshio_obj_emit(big_v, None, None, 0, None, 4, None, None, None) == -1
    assert L.lara_meshio_obj_emit(4, None, None, 4, None, 8, None, None, None) == -1
    assert L.lara_meshio_obj_emit(0, None, None, 0, None, 4, None, None, None) == 0
    assert [L.lara_meshio_ply_body_bytes(1, 0, n, c) for n in (0, 1) for c in (0, 1)] == [12, 15, 24, 27]
    assert L.lara_meshio_ply_body_bytes(10, 4, 1, 1) == 270 + 52 and L.lara_meshio_ply_body_bytes(0, 0, 0, 0) == 0
    assert L.lara_meshio_ply_body_bytes(-1, 4, 0, 0) == -1 and L.lara_meshio_ply_body_bytes(4, big_t, 0, 0) == -1
    assert L.lara_meshio_ply_body_bytes(big_v - 1, big_t - 1, 1, 1) == 27 * (big_v - 1) + 13 * (big_t - 1)      # beyond 2^32: int64
    assert L.lara_meshio_ply_workspace_bytes() == 8
    assert L.lara_meshio_ply_pack(4, None, None, None, 0, None, 4, None, None, None) == -1
    assert L.lara_meshio_ply_pack(0, None, None, None, 4, None, 3, None, None, None) == -1
    assert L.lara_meshio_ply_pack(0, None, None, None, 0, None, 4, None, None, None) == 0
    n = (ctypes.c_int * 1)()
    assert L.lara_meshio_format_f32_host(-1, None, None, None) == -1 and L.lara_meshio_format_f32_host(1, None, None, n) == -1
    assert L.lara_meshio_format_u32_host(-1, None, None, None) == -1 and L.lara_meshio_format_u32_host(1, None, None, n) == -1
    assert L.lara_meshio_format_f32_host(0, None, None, None) == 0 and L.lara_meshio_format_u32_host(0, None, None, None) == 0
    v, t = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int64)
    for fn in (meshio.obj_bytes, meshio.ply_bytes):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(v, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshio.write_mesh(str(tmp_path / "a.obj"), v, t)
    # the format is settled before any tensor is looked at
    with pytest.raises(ValueError, match="extension"):
        meshio.write_mesh(str(tmp_path / "a.stl"), v, t)
    with pytest.raises(ValueError, match="extension"):
        meshio.write_mesh(str(tmp_path / "a"), v, t)
    with pytest.raises(ValueError, match="format"):
        meshio.write_mesh(str(tmp_path / "a.obj"), v, t, format="stl")
    with pytest.raises(ValueError, match="normals"):
        meshio.write_mesh(str(tmp_path / "a.obj"), v, t, normals=v)
    with pytest.raises(ValueError, match="normals"):
        meshio.write_mesh(str(tmp_path / "a.ply"), v, t, normals=v, format="obj")
    assert not list(tmp_path.iterdir())
    from lara_amd.mesh import MeshExtractor
    with pytest.raises(ValueError, match="writer"):
        MeshExtractor.extract(object.__new__(MeshExtractor), str(tmp_path / "a.obj"), None, cams=[], writer="disk")
