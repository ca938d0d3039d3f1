"""lara_amd.meshio on the device: `obj_bytes` against the bytes of the file `mesh.write_obj` writes for the same tensors, `ply_bytes`
against the numpy restatement (tests/meshio_restate.py), byte for byte -- the routines are exact, so every comparison is an equality
and there is no bar --, the raw entry points against guard bytes, the refusal of indices out of range, the files read back, and
`MeshExtractor.extract(writer="device")` against `writer="host"`.  Inputs: tests/meshio_cases.py.  The tally of meshes and bytes
that compared equal goes to test_out/meshio_parity.txt."""
import os

import numpy as np
import pytest
import torch

from tests import meshio_cases as C
from tests import meshio_restate as R

FILL, SLACK, GUARD = 0xA5, 4096, 256
TALLY = {"obj_meshes": 0, "obj_bytes": 0, "ply_meshes": 0, "ply_bytes": 0}


@pytest.fixture(scope="module", autouse=True)
def _write_tally():
    yield
    line = ("meshio: {obj_meshes} OBJ meshes / {obj_bytes} bytes equal to write_obj's files, "
            "{ply_meshes} PLY meshes / {ply_bytes} bytes equal to the restatement").format(**TALLY)
    print("\n" + line)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "test_out"), exist_ok=True)
    with open(os.path.join(root, "test_out", "meshio_parity.txt"), "w") as f:
        f.write(line + "\n")


def _dev(x, dtype=None):
    if x is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def _assert_obj(tmp_path, v, t, c=None, what=""):
    """obj_bytes(v, t, c) == the file write_obj writes for the same tensors; two calls give equal tensors.  Returns the bytes."""
    from lara_amd import mesh, meshio
    path = str(tmp_path / "target.obj")
    mesh.write_obj(path, v, t, c)
    with open(path, "rb") as f:
        want = f.read()
    got = meshio.obj_bytes(v, t, c)
    again = meshio.obj_bytes(v, t, c)
    assert got.dtype == torch.uint8 and got.is_cuda and got.dim() == 1 and torch.equal(got, again)
    got = _host(got)
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        lo = max(0, first - 60)
        raise AssertionError(f"{what}: {len(got)} bytes for {len(want)}; first difference at byte {first}: "
                             f"{got[lo:first + 40]!r} for {want[lo:first + 40]!r}")
    TALLY["obj_meshes"] += 1
    TALLY["obj_bytes"] += len(want)
    return want


def _assert_ply(v, t, c=None, n=None, what=""):
    from lara_amd import meshio
    want = R.ply_bytes(v, t, c, n)
    args = (_dev(v), _dev(t), _dev(c), _dev(n))
    got = meshio.ply_bytes(*args)
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got, meshio.ply_bytes(*args))
    got = _host(got)
    if got != want:
        m = min(len(got), len(want))
        first = next((i for i in range(m) if got[i] != want[i]), m)
        raise AssertionError(f"{what}: {len(got)} bytes for {len(want)}; first difference at byte {first} "
                             f"(the header has {len(R.ply_header(len(v), len(t), n is not None, c is not None))})")
    TALLY["ply_meshes"] += 1
    TALLY["ply_bytes"] += len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("with_colors", [False, True])
def test_obj_bytes_equal_write_obj_at_every_size(hip_lib, tmp_path, with_colors):
    for nv, nt in C.SIZES:
        v, t, c, _ = C.mesh(nv, nt)
        want = _assert_obj(tmp_path, _dev(v), _dev(t), _dev(c) if with_colors else None, what=f"({nv}, {nt})")
        assert want.count(b"\n") == nv + nt and (nv + nt > 0 or want == b"")
        _assert_obj(tmp_path, _dev(v), _dev(t, torch.int32), _dev(c) if with_colors else None, what=f"({nv}, {nt}) int32")


@pytest.mark.gpu
def test_obj_bytes_equal_write_obj_on_the_edges(hip_lib, tmp_path):
    from lara_amd import meshio
    v, t, c = C.specials_mesh()                    # every special value in every position of a line
    _assert_obj(tmp_path, _dev(v), _dev(t), _dev(c), what="specials")
    _assert_obj(tmp_path, _dev(v), _dev(t), None, what="specials, no colours")
    v, t, c = C.widest()                           # a workgroup's LDS span exactly full: 256 x 98 and 256 x 35 bytes
    want = _assert_obj(tmp_path, _dev(v), _dev(t), _dev(c), what="widest")
    assert len(want) == 256 * (meshio.MAX_VERTEX_LINE + meshio.MAX_FACE_LINE)
    v, t, c = C.narrowest()
    want = _assert_obj(tmp_path, _dev(v), _dev(t), None, what="narrowest")
    assert want == b"v 0 0 0\n" * len(v) + b"f 1 1 1\n" * len(t)
    v, t, c = C.crossing_mesh()                    # indices on every digit-count crossing
    for dtype in (torch.int64, torch.int32):
        want = _assert_obj(tmp_path, _dev(v), _dev(t, dtype), None, what=f"crossings {dtype}")
        assert b" 9 " in want and b" 10 " in want and b" 999999999" in want and b" 1000000000" in want and b" 2147483647" in want
    for dtype in (torch.int16, torch.uint8):       # any integer type
        _assert_obj(tmp_path, _dev(v), _dev(t % 100, dtype), None, what=f"{dtype}")
    # fp64 vertices and colours are cast as write_obj casts them
    rng = np.random.default_rng(3)
    v64, c64 = rng.standard_normal((300, 3)) / 3.0, rng.random((300, 3))
    t = rng.integers(0, 300, (500, 3))
    assert not np.array_equal(v64.astype(np.float32).astype(np.float64), v64)
    _assert_obj(tmp_path, _dev(v64), _dev(t), _dev(c64), what="fp64")
    # a non-contiguous vertex view, a non-contiguous triangle view
    wide, tw = _dev(rng.standard_normal((300, 7)).astype(np.float32)), _dev(rng.integers(0, 300, (500, 5)))
    vv, tt = wide[:, 2:5], tw[:, 1:4]
    assert not vv.is_contiguous() and not tt.is_contiguous()
    _assert_obj(tmp_path, vv, tt, wide[:, 4:7], what="views")
    _assert_obj(tmp_path, wide[::2, :3], tt, None, what="strided rows")


@pytest.mark.gpu
@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_bytes_equal_the_restatement(hip_lib, with_normals, with_colors):
    for nv, nt in C.SIZES:
        v, t, c, n = C.mesh(nv, nt)
        _assert_ply(v, t, c if with_colors else None, n if with_normals else None, what=f"({nv}, {nt})")
    v, t, c = C.specials_mesh()                    # bit copies, NaN payloads and negative zeros included
    _assert_ply(v, t.astype(np.int32), c if with_colors else None, v[::-1].copy() if with_normals else None, what="specials")
    v, t, _ = C.crossing_mesh()
    _assert_ply(v, t, v if with_colors else None, v if with_normals else None, what="crossings")


@pytest.mark.gpu
def test_ply_colour_edges(hip_lib):
    from lara_amd import meshio
    e = C.color_edges()
    v = np.zeros_like(e)
    t = np.zeros((1, 3), np.int64)
    _assert_ply(v, t, e, None, what="colour edges")
    _assert_ply(v, t, e, e, what="colour edges with normals")
    got = np.frombuffer(_host(meshio.ply_bytes(_dev(v), _dev(t), _dev(e))), np.uint8)
    rows = got[len(R.ply_header(len(v), 1, False, True)):][: 15 * len(v)].reshape(-1, 15)[:, 12:]
    assert np.array_equal(rows, R.color_u8(e))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(257, 300), (1000, 2100), (3, 1)])
@pytest.mark.parametrize("index_dtype", [torch.int64, torch.int32])
def test_raw_entry_points_write_nothing_beyond_their_bytes(hip_lib, tmp_path, size, index_dtype):
    """The emit and pack entries, given an output 4096 bytes longer than needed and pre-filled with 0xA5, at an address that is no
    multiple of 16, leave every byte beyond the total (and in front of the first) untouched; so do the workspaces' guard bytes."""
    from lara_amd import _native, mesh
    nv, nt = size
    vn, tn, cn, nn = C.mesh(nv, nt)
    dev = torch.device("cuda:0")
    v, t, c, n = _dev(vn), _dev(tn, index_dtype), _dev(cn), _dev(nn)
    ib = t.element_size()
    path = str(tmp_path / "target.obj")
    mesh.write_obj(path, v, t, c)
    with open(path, "rb") as f:
        want = f.read()
    nbytes = _native.query("lara_meshio_obj_workspace_bytes", nv, nt)
    nb = nbytes // 8 - 1
    assert nb == -(-nv // 256) + -(-nt // 256)
    guarded = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    ws = guarded[GUARD:GUARD + nbytes].view(torch.int64)
    _native.call("lara_meshio_obj_lengths", dev, nv, v, c, nt, t, ib, ws)
    totals = ws[:nb].clone()
    assert int(ws[nb]) == 0 and int(totals.sum()) == len(want)
    assert bool((guarded[:GUARD] == FILL).all()) and bool((guarded[GUARD + nbytes:] == FILL).all())
    offsets = torch.cumsum(totals, 0) - totals
    for lead in (0, 5):                          # an aligned start, and a head that is not
        out = torch.full((lead + len(want) + SLACK,), FILL, dtype=torch.uint8, device=dev)
        _native.call("lara_meshio_obj_emit", dev, nv, v, c, nt, t, ib, offsets, out.data_ptr() + lead)
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert host[lead:lead + len(want)].tobytes() == want
        assert (host[:lead] == FILL).all() and (host[lead + len(want):] == FILL).all()
    # PLY: the body alone, 27-byte rows and 12-byte rows
    for cc, nrm, col in ((c, n, cn), (None, None, None)):
        body = R.ply_bytes(vn, tn, col, None if nrm is None else nn)[len(R.ply_header(nv, nt, nrm is not None, col is not None)):]
        assert len(body) == _native.query("lara_meshio_ply_body_bytes", nv, nt, int(nrm is not None), int(col is not None))
        pw = torch.full((8 + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        for lead in (0, 7):
            out = torch.full((lead + len(body) + SLACK,), FILL, dtype=torch.uint8, device=dev)
            _native.call("lara_meshio_ply_pack", dev, nv, v, nrm, cc, nt, t, ib, out.data_ptr() + lead, pw[GUARD:GUARD + 8])
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            assert host[lead:lead + len(body)].tobytes() == body
            assert (host[:lead] == FILL).all() and (host[lead + len(body):] == FILL).all()
        hp = pw.cpu().numpy()
        assert (hp[:GUARD] == FILL).all() and (hp[GUARD + 8:] == FILL).all() and not hp[GUARD:GUARD + 8].any()


@pytest.mark.gpu
def test_an_index_out_of_range_raises_and_no_file_appears(hip_lib, tmp_path):
    from lara_amd import meshio
    v, t, c, _ = C.mesh(257, 300)
    v, c = _dev(v), _dev(c)
    for bad, dtype, row in ((-1, torch.int64, 0), (2 ** 31 - 1, torch.int64, 299), (2 ** 40, torch.int64, 256), (-1, torch.int32, 255),
                            (2 ** 31 - 1, torch.int32, 17)):
        tt = t.copy()
        tt[row, 1] = bad
        tt = _dev(tt, dtype)
        with pytest.raises(RuntimeError, match="outside"):
            meshio.obj_bytes(v, tt, c)
        with pytest.raises(RuntimeError, match="outside"):
            meshio.ply_bytes(v, tt, c)
        for name in ("bad.obj", "bad.ply"):
            with pytest.raises(RuntimeError, match="outside"):
                meshio.write_mesh(str(tmp_path / "sub" / name), v, tt, c)
    assert not list(tmp_path.iterdir())
    t[0, 0] = 2 ** 31 - 2                            # the largest index that is in range
    assert meshio.obj_bytes(v, _dev(t), c).numel() > 0 and meshio.ply_bytes(v, _dev(t), c).numel() > 0
    with pytest.raises(ValueError, match="integer"):
        meshio.obj_bytes(v, _dev(t).float(), c)


@pytest.mark.gpu
def test_written_files_read_back_bit_exact(hip_lib, tmp_path):
    from lara_amd import mesh, meshio
    vn, tn, cn, nn = C.mesh(1000, 2100)
    v, t, c, n = _dev(vn), _dev(tn), _dev(cn), _dev(nn)
    for name, fmt in (("a.obj", None), ("b.OBJ", None), ("deep/er/c.ply", None), ("d.PLY", None), ("e.dat", "ply"), ("f.ply", "obj")):
        path = str(tmp_path / name)
        is_ply = (fmt or name.rsplit(".", 1)[1].lower()) == "ply"
        wrote = meshio.write_mesh(path, v, t, c, n if is_ply else None, format=fmt)
        assert wrote == os.path.getsize(path)
        with open(path, "rb") as f:
            data = f.read()
        if is_ply:
            assert data == R.ply_bytes(vn, tn, cn, nn)
            rv, rt, rc = meshio.read_ply(path)
            assert rc.tobytes() == (R.color_u8(cn).astype(np.float32) / np.float32(255)).tobytes()
        else:
            assert data == _host(meshio.obj_bytes(v, t, c))
            rv, rt, rc = mesh.read_obj(path)
            assert rc.tobytes() == cn.tobytes()
        assert rv.tobytes() == vn.tobytes() and np.array_equal(rt, tn)
        if fmt is None:
            mv, mt, mc = meshio.read_mesh(path)
            assert mv.tobytes() == rv.tobytes() and np.array_equal(mt, rt) and mc.tobytes() == rc.tobytes()
    assert meshio.write_mesh(str(tmp_path / "empty.obj"), v[:0], t[:0]) == 0 and os.path.getsize(str(tmp_path / "empty.obj")) == 0
    assert meshio.write_mesh(str(tmp_path / "empty.ply"), v[:0], t[:0]) == len(R.ply_header(0, 0, False, False))
    ev, et, ec = meshio.read_ply(str(tmp_path / "empty.ply"))
    assert ev.shape == (0, 3) and et.shape == (0, 3) and ec is None


@pytest.mark.gpu
def test_mesh_extractor_device_writer(hip_lib, tmp_path):
    """On the scene and cameras of tests/test_meshclean_gpu.py's own extractor test: writer="device" writes the bytes writer="host"
    writes; a .ply path gives a PLY that reads back as the returned mesh; the default call is the host writer."""
    from lara_amd import meshio
    from lara_amd.mesh import MeshExtractor, write_obj
    from lara_amd.renderer import Renderer
    from tests.test_meshclean_gpu import AABB, _scene_params, _turntable
    params, cams = _scene_params(), _turntable()
    ex = MeshExtractor(params, Renderer(sh_degree=1, white_background=True), AABB)
    read = lambda p: open(p, "rb").read()
    host, default, device, ply = (str(tmp_path / n) for n in ("host.obj", "default.obj", "device.obj", "mesh.ply"))
    ex.timings = []
    v, t, c = ex.extract(host, None, cams=cams)      # the default call: the host writer, write_obj's bytes as before
    host_marks = [name for name, _ in ex.timings]
    assert t.shape[0] > 5000
    ex.timings = []
    dv, dt, dc = ex.extract(device, None, cams=cams, writer="device")
    assert [name for name, _ in ex.timings] == host_marks and host_marks[-1] == "write_obj"
    ex.timings = None
    assert torch.equal(dv, v) and torch.equal(dt, t) and torch.equal(dc, c)
    assert read(device) == read(host)
    TALLY["obj_meshes"] += 1
    TALLY["obj_bytes"] += os.path.getsize(host)
    write_obj(default, v, t, c)
    assert read(default) == read(host)
    pv, pt, pc = ex.extract(ply, None, cams=cams, writer="device")
    rv, rt, rc = meshio.read_ply(ply)
    assert rv.tobytes() == pv.cpu().numpy().tobytes() and np.array_equal(rt, pt.cpu().numpy())
    assert np.array_equal(rc, R.color_u8(pc.cpu().numpy()).astype(np.float32) / np.float32(255))
    assert read(ply) == R.ply_bytes(pv.cpu().numpy(), pt.cpu().numpy(), pc.cpu().numpy())
    TALLY["ply_meshes"] += 1
    TALLY["ply_bytes"] += os.path.getsize(ply)
