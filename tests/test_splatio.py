"""`lara_amd.splatio` on CPU tensors, held to the numpy restatement of the layout (tests/splatio_restate.py): the written bytes
equal the restatement's for every SH degree and P in {0, 1, 257}; a round trip returns every tensor's bits, NaN payloads,
infinities, -0.0 and denormals included; the channel-major rule of ``f_rest`` (and a file in the other order does NOT read back
equal); the reader's tolerance (permuted properties, no normals, extra properties, comments, a 3DGS-style file) and each of its
refusals; ``from_render_pkg`` / ``scene_item`` / ``gs_params``; ``select``; ``concatenate``; ``evaluate.save_surfels``; and that
nothing on the default routes imports the module."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lara_amd import splatio
from tests import splatio_cases as C
from tests import splatio_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(c, device="cpu"):
    return splatio.SurfelCloud(*(torch.from_numpy(c[k].copy()).to(device) for k in C.FIELDS))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(cloud, c):
    """Every tensor of ``cloud`` holds the words of the arrays ``c``."""
    for k, t in zip(C.FIELDS, cloud.render_args()):
        want = torch.from_numpy(c[k].view(np.int32).copy())
        assert t.dtype == torch.float32 and t.shape == want.shape and torch.equal(_bits(t.cpu()), want), k
    return True


def _put(tmp_path, data, name="f.ply"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


# ------------------------------------------------------------------------------------------------------------------ writing

@pytest.mark.parametrize("thickness", [None, 0.003])
@pytest.mark.parametrize("P", [0, 1, 257])
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_ply_bytes_equal_the_restatement(degree, P, thickness):
    c = C.cloud(P, degree, seed=1, special=True)
    got = splatio.ply_bytes(_cloud(c), thickness)
    assert isinstance(got, bytes)
    want = R.file_bytes(c, thickness)
    head = splatio.ply_header(P, degree, thickness is not None)
    assert head == R.header(P, degree, thickness is not None) == got[:len(head)]
    n_props = 3 + 3 + 3 * (degree + 1) ** 2 + 1 + (2 if thickness is None else 3) + 4
    assert len(got) == len(head) + 4 * n_props * P
    assert got == want


def test_write_ply_writes_ply_bytes_and_p0_writes_the_header_alone(tmp_path):
    c = C.cloud(257, 1, seed=2, special=True)
    p = tmp_path / "sub" / "point_cloud.ply"
    n = splatio.write_ply(str(p), _cloud(c), thickness=0.01)
    assert p.read_bytes() == splatio.ply_bytes(_cloud(c), 0.01) and n == p.stat().st_size
    n = splatio.write_ply(str(p), _cloud(C.cloud(0, 2)))
    assert p.read_bytes() == splatio.ply_header(0, 2) and n == len(splatio.ply_header(0, 2))
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            splatio.ply_bytes(_cloud(c), bad)
    with pytest.raises(ValueError):
        splatio.ply_header(4, 4)


def test_the_cloud_refuses_other_shapes_and_types():
    c = C.cloud(5, 1)
    t = {k: torch.from_numpy(c[k]) for k in C.FIELDS}
    with pytest.raises(ValueError):
        splatio.SurfelCloud(t["centers"], t["shs"][:, :3], t["opacity"], t["scales"], t["rotations"])          # 3 coefficients
    with pytest.raises(ValueError):
        splatio.SurfelCloud(t["centers"], t["shs"], t["opacity"][:4], t["scales"], t["rotations"])
    with pytest.raises(ValueError):
        splatio.SurfelCloud(t["centers"].double(), t["shs"], t["opacity"], t["scales"], t["rotations"])
    ok = splatio.SurfelCloud(t["centers"].requires_grad_(True), t["shs"], t["opacity"], t["scales"], t["rotations"])
    assert ok.n_surfels == 5 and ok.sh_degree == 1 and not ok.centers.requires_grad


# ------------------------------------------------------------------------------------------------------------------ round trip

@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_round_trip_returns_every_bit(tmp_path, degree):
    c = C.cloud(257, degree, seed=4, special=True)
    for k in C.FIELDS:          # the seeds are there: two NaN payloads, both infinities, -0.0 and denormals in every field
        w = set(c[k].view(np.uint32).reshape(-1).tolist())
        assert set(C.SPECIAL_WORDS.tolist()) <= w, k
    p = str(tmp_path / "c.ply")
    splatio.write_ply(p, _cloud(c))
    back, info = splatio.read_ply(p)
    assert _same_bits(back, c)
    assert (back.n_surfels, back.sh_degree) == (257, degree) == (info["n_surfels"], info["sh_degree"])
    assert info["dropped_third_scale"] is None and info["skipped_properties"] == ["nx", "ny", "nz"]
    assert info["comments"] == ["comment lara_amd.splatio"]


def test_round_trip_with_thickness_returns_two_scales_and_reports_the_third(tmp_path):
    c = C.cloud(257, 1, seed=5, special=True)
    p = str(tmp_path / "c.ply")
    splatio.write_ply(p, _cloud(c), thickness=0.003)
    back, info = splatio.read_ply(p)
    assert _same_bits(back, c) and back.scales.shape == (257, 2)
    third = float(np.float32(math.log(0.003)))
    assert info["dropped_third_scale"] == {"min": third, "max": third}


def test_round_trip_of_an_empty_cloud(tmp_path):
    p = str(tmp_path / "c.ply")
    splatio.write_ply(p, _cloud(C.cloud(0, 3)), thickness=1.0)
    back, info = splatio.read_ply(p)
    assert back.n_surfels == 0 and back.sh_degree == 3 and back.shs.shape == (0, 16, 3)
    assert info["dropped_third_scale"] == {"min": None, "max": None}


# ------------------------------------------------------------------------------------------------------------------ channel-major

def test_f_rest_is_channel_major(tmp_path):
    P, degree, n = 7, 2, 9
    c = C.numbered(P, degree)
    data = splatio.ply_bytes(_cloud(c))
    names = R.property_names(degree)
    rows = np.frombuffer(data, np.dtype([(a, "<f4") for a in names]), P, len(R.header(P, degree)))
    for ch in range(3):
        assert np.array_equal(rows["f_dc_%d" % ch], 100.0 * np.arange(P) + ch)
        for k in range(n - 1):
            assert np.array_equal(rows["f_rest_%d" % (ch * (n - 1) + k)], 100.0 * np.arange(P) + 10 * (1 + k) + ch)
    assert np.array_equal(rows["f_rest_1"], 100.0 * np.arange(P) + 20)            # the second coefficient of RED, not green
    back, _ = splatio.read_ply(_put(tmp_path, data))
    assert _same_bits(back, c)
    # the OTHER flatten (coefficient-major) is a different file and loads as different coefficients
    other = R.file_bytes(c, order="coefficient")
    assert other != data and len(other) == len(data)
    wrong, _ = splatio.read_ply(_put(tmp_path, other, "other.ply"))
    assert not torch.equal(_bits(wrong.shs), torch.from_numpy(c["shs"].view(np.int32).copy()))
    assert torch.equal(_bits(wrong.shs[:, 0]), torch.from_numpy(c["shs"][:, 0].copy().view(np.int32)))          # (the DC is not in question)


# ------------------------------------------------------------------------------------------------------------------ reader tolerance

def test_reader_finds_properties_by_name_and_skips_the_rest(tmp_path):
    P, degree = 257, 1
    c = C.cloud(P, degree, seed=6, special=True)
    col = R.columns(c)
    g = np.random.default_rng(0)
    names = [a for a in R.property_names(degree) if a not in ("nx", "ny", "nz")]
    props = [(names[i], "float") for i in g.permutation(len(names))]
    props.insert(3, ("label", "uchar"))
    props.insert(11, ("confidence", "double"))
    col["label"], col["confidence"] = g.integers(0, 256, P).astype(np.uint8), g.normal(size=P)
    data = R.custom_file(props, col, P, extra_header=["comment made by a test", "obj_info anything at all", "comment  "])
    back, info = splatio.read_ply(_put(tmp_path, data))
    assert _same_bits(back, c)
    assert info["skipped_properties"] == ["label", "confidence"] and info["dropped_third_scale"] is None
    assert len(info["comments"]) == 3
    # a trailing element is allowed when it has no rows (a list property in it included)
    data = R.custom_file(props, col, P, after=["element face 0", "property list uchar int vertex_indices"])
    assert _same_bits(splatio.read_ply(_put(tmp_path, data))[0], c)


def test_reader_loads_a_3dgs_style_file(tmp_path):
    """Three scales, degree 3, the order of the 3DGS ``save_ply`` (the same as this module's, with scale_2)."""
    P, degree = 33, 3
    c = C.cloud(P, degree, seed=7)
    col = R.columns(c)
    s2 = np.linspace(-9.0, -4.0, P).astype(np.float32)
    col["scale_2"] = R.words(s2)
    names = R.property_names(degree, third_scale=True)
    assert len(names) == 62          # 3 + 3 + 3 + 45 + 1 + 3 + 4: the 3DGS row
    data = R.custom_file([(a, "float") for a in names], col, P)
    back, info = splatio.read_ply(_put(tmp_path, data))
    assert _same_bits(back, c) and back.sh_degree == 3
    assert info["dropped_third_scale"] == {"min": -9.0, "max": -4.0}


# ------------------------------------------------------------------------------------------------------------------ refusals

def _minimal(P=2, degree=0):
    c = C.cloud(P, degree, seed=8)
    return [(a, "float") for a in R.property_names(degree)], R.columns(c), P


def _refusal_files():
    props, col, P = _minimal()
    good = R.custom_file(props, col, P)
    files = {
        "ascii": R.custom_file(props, col, P, fmt="ascii 1.0"),
        "big-endian": R.custom_file(props, col, P, fmt="binary_big_endian 1.0"),
        "list property": R.custom_file(props, col, 0, after=["property list uchar int neighbours"]),
        "missing opacity": R.custom_file([p for p in props if p[0] != "opacity"], col, P),
        "missing rot_3": R.custom_file([p for p in props if p[0] != "rot_3"], col, P),
        "missing f_dc_1": R.custom_file([p for p in props if p[0] != "f_dc_1"], col, P),
        "element before vertex": R.custom_file(props, col, P, before=["element camera 0", "property float fx"]),
        "no vertex element": good.replace(b"element vertex", b"element points"),
        "body one byte short": good[:-1],
        "body one byte long": good + b"\0",
        "body one row short": good[:-4 * len(props)],
        "count does not fit: negative": good.replace(b"element vertex 2", b"element vertex -2"),
        "count does not fit: fraction": good.replace(b"element vertex 2", b"element vertex 2.0"),
        "count does not fit: too large": good.replace(b"element vertex 2", b"element vertex 3"),
        "count does not fit: too small": good.replace(b"element vertex 2", b"element vertex 1"),
        "rows in a trailing element": R.custom_file(props, col, P, after=["element face 1", "property int a"]) + b"\0\0\0\0",
        "f_rest count": R.custom_file(props + [("f_rest_0", "float"), ("f_rest_1", "float"), ("f_rest_2", "float")],
                                      dict(col, f_rest_0=col["x"], f_rest_1=col["x"], f_rest_2=col["x"]), P),
        "double x": R.custom_file([(a, "double" if a == "x" else t) for a, t in props], dict(col, x=np.zeros(P)), P),
        "a property twice": R.custom_file(props + [("w", "float")], dict(col, w=col["x"]), P).replace(b"float w\n", b"float x\n"),
        "no end_header": good.replace(b"end_header\n", b""),
        "not a ply": b"plx" + good[3:],
        "no format line": good.replace(b"format binary_little_endian 1.0\n", b""),
    }
    return good, files


def test_the_minimal_file_of_the_refusals_loads(tmp_path):
    good, _ = _refusal_files()
    cloud, _ = splatio.read_ply(_put(tmp_path, good))
    assert cloud.n_surfels == 2 and cloud.sh_degree == 0


@pytest.mark.parametrize("key", sorted(_refusal_files()[1]))
def test_reader_refuses(tmp_path, key):
    path = _put(tmp_path, _refusal_files()[1][key], "refused.ply")
    with pytest.raises(ValueError) as e:
        splatio.read_ply(path)
    assert "refused.ply" in str(e.value)          # the error names the file


# ------------------------------------------------------------------------------------------------------------------ render_pkg

def _tuples(P=257, keep=100, seed=9, degree=1):
    """(coarse 5-tuple, fine 6-tuple) as network.py:483 and :515 build them, and the fine subset as arrays."""
    c = C.cloud(P, degree, seed=seed, special=True)
    t = {k: torch.from_numpy(c[k].copy()) for k in C.FIELDS}
    g = torch.Generator().manual_seed(seed)
    mask = torch.zeros(P, dtype=torch.bool)
    mask[torch.randperm(P, generator=g)[:keep]] = True
    shs_fine = t["shs"][mask] + 1.0
    coarse = (t["centers"], t["shs"], t["opacity"], t["scales"], t["rotations"])
    fine = (t["centers"][mask], shs_fine, t["opacity"], t["scales"], t["rotations"], mask)
    m = mask.numpy()
    sub = {"centers": c["centers"][m], "shs": shs_fine.numpy(), "opacity": c["opacity"][m], "scales": c["scales"][m],
           "rotations": c["rotations"][m]}
    return c, coarse, fine, sub


def test_from_render_pkg_takes_the_coarse_and_the_fine_tuple():
    c, coarse, fine, sub = _tuples()
    a = splatio.SurfelCloud.from_render_pkg(coarse)
    assert a.n_surfels == 257 and _same_bits(a, c)
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(a.render_args(), coarse))          # taken as it is
    b = splatio.SurfelCloud.from_render_pkg(fine)
    assert b.n_surfels == 100 and _same_bits(b, sub)
    with pytest.raises(ValueError):
        splatio.SurfelCloud.from_render_pkg(coarse[:4])
    # gs_params() into the indexing MeshExtractor.extract does (lara_amd/mesh.py: `_opacity[mask]` ...)
    _centers, _shs, _opacity, _scaling, _rotation, mask = b.gs_params()
    assert mask.dtype == torch.bool and mask.shape == (100,) and bool(mask.all())
    got = splatio.SurfelCloud(_centers, _shs, _opacity[mask], _scaling[mask], _rotation[mask])
    assert _same_bits(got, sub)
    assert [t.data_ptr() for t in b.render_args()] == [t.data_ptr() for t in (_centers, _shs, _opacity, _scaling, _rotation)]


def test_scene_item_follows_the_list_order_of_the_network():
    _, c0, f0, _ = _tuples(seed=10)
    _, c1, f1, _ = _tuples(seed=11)
    pkg = [c0, f0, c1, f1]
    assert splatio.scene_item(pkg, 0) is f0 and splatio.scene_item(pkg, 1) is f1
    assert splatio.scene_item(pkg, 0, stage="coarse") is c0 and splatio.scene_item(pkg, 1, "coarse") is c1
    pkg = [c0, c1]                                                       # a step without the fine stage
    assert splatio.scene_item(pkg, 0, "coarse", with_fine=False) is c0 and splatio.scene_item(pkg, 1, "coarse", with_fine=False) is c1
    for args in ((pkg, 0, "fine", False), (pkg, 2, "coarse", False), ([c0, f0, c1, f1], 2), ([c0, f0], -1), (pkg, 0, "medium"),
                 (pkg, 0, "fine", True), ([c0, f0, c1], 0)):
        with pytest.raises(ValueError):
            splatio.scene_item(*args)


def test_save_surfels_writes_what_the_module_writes(tmp_path):
    from lara_amd import evaluate
    _, coarse, fine, sub = _tuples()
    p = str(tmp_path / "out" / "point_cloud.ply")
    assert evaluate.save_surfels(p, fine) == 100
    assert open(p, "rb").read() == R.file_bytes(sub)
    n = evaluate.save_surfels(p, coarse, min_opacity=0.05, thickness=0.002)
    cloud = splatio.SurfelCloud.from_render_pkg(coarse)
    kept, idx = splatio.select(cloud, min_opacity=0.05)
    assert n == kept.n_surfels == idx.numel() and 0 < n < 257
    assert open(p, "rb").read() == splatio.ply_bytes(kept, 0.002)


# ------------------------------------------------------------------------------------------------------------------ select

def _select_cloud():
    """12 rows whose opacity and centre sit on, just above and just below the thresholds, with NaN rows."""
    c = C.cloud(12, 1, seed=12)
    x = np.float32(-1.25)
    s = torch.sigmoid(torch.tensor(x)).item()                          # the fp32 sigmoid the module compares
    thr = float(s)
    above = np.nextafter(np.float32(thr), np.float32(1))
    lo, hi = np.float32(-0.25), np.float32(0.375)
    c["centers"][:] = 0.0
    c["opacity"][:] = 3.0
    c["opacity"][1] = x                                                 # sigmoid == thr: `>` drops it
    c["opacity"][2] = np.nan
    c["opacity"][3] = -np.inf                                           # sigmoid 0
    c["opacity"][4] = np.inf                                            # sigmoid 1
    c["centers"][5] = (lo, hi, lo)                                      # on the box: `<=` keeps it
    c["centers"][6] = (np.nextafter(lo, np.float32(-1)), 0, 0)          # one ulp outside
    c["centers"][7] = (0, np.nextafter(hi, np.float32(1)), 0)
    c["centers"][8] = (0, np.nan, 0)
    c["centers"][9] = (0, 0, np.inf)
    c["centers"][10] = (-0.0, 0, 0)
    c["opacity"][11], c["centers"][11] = np.nan, (np.nan, 0, 0)
    return c, thr, float(above), ([float(lo)] * 3, [float(hi)] * 3)


def _rows(c, idx):
    return {k: c[k][idx] for k in C.FIELDS}


def test_select_keeps_rows_in_order_with_exact_edges():
    c, thr, above, box = _select_cloud()
    cloud = _cloud(c)
    every, idx = splatio.select(cloud)                                  # no filter: NaN rows stay
    assert idx.dtype == torch.int64 and idx.tolist() == list(range(12)) and _same_bits(every, c)
    got, idx = splatio.select(cloud, min_opacity=thr)
    assert idx.tolist() == [0, 4, 5, 6, 7, 8, 9, 10] and _same_bits(got, _rows(c, idx.numpy()))
    assert 1 in splatio.select(cloud, min_opacity=float(np.nextafter(np.float32(thr), np.float32(0))))[1].tolist()
    assert 1 not in splatio.select(cloud, min_opacity=above)[1].tolist()
    got, idx = splatio.select(cloud, aabb=box)
    assert idx.tolist() == [0, 1, 2, 3, 4, 5, 10] and _same_bits(got, _rows(c, idx.numpy()))
    got, idx = splatio.select(cloud, min_opacity=thr, aabb=torch.tensor(box))
    assert idx.tolist() == [0, 4, 5, 10] and _same_bits(got, _rows(c, idx.numpy()))
    got, idx = splatio.select(cloud, min_opacity=1.0)                   # sigmoid(inf) = 1 is not > 1: nothing passes
    assert idx.numel() == 0 and idx.dtype == torch.int64 and got.n_surfels == 0 and got.shs.shape == (0, 4, 3)
    assert splatio.ply_bytes(got) == splatio.ply_header(0, 1)
    c2 = C.cloud(257, 2, seed=13)
    got, idx = splatio.select(_cloud(c2), min_opacity=0.1, aabb=([-0.4, -0.5, -0.5], [0.5, 0.3, 0.5]))
    want = np.nonzero((1.0 / (1.0 + np.exp(-c2["opacity"][:, 0].astype(np.float64))) > 0.1 + 1e-6) & (c2["centers"][:, 0] >= -0.4)
                      & (c2["centers"][:, 1] <= 0.3))[0]
    assert 0 < idx.numel() < 257 and bool((idx[1:] > idx[:-1]).all()) and set(want.tolist()) <= set(idx.tolist())
    assert _same_bits(got, _rows(c2, idx.numpy()))


# ------------------------------------------------------------------------------------------------------------------ concatenate

def test_concatenate_keeps_the_order_and_refuses_mixed_degrees():
    a, b, e = C.cloud(5, 1, seed=14, special=True), C.cloud(257, 1, seed=15, special=True), C.cloud(0, 1)
    got = splatio.concatenate([_cloud(a), _cloud(e), _cloud(b), _cloud(a)])
    assert got.n_surfels == 267 and _same_bits(got, {k: np.concatenate([a[k], b[k], a[k]]) for k in C.FIELDS})
    with pytest.raises(ValueError):
        splatio.concatenate([_cloud(a), _cloud(C.cloud(5, 2))])
    with pytest.raises(ValueError):
        splatio.concatenate([])


# ------------------------------------------------------------------------------------------------------------------ hygiene

def test_the_default_routes_do_not_import_splatio():
    code = ("import sys, lara_amd, lara_amd.evaluate, lara_amd.pipeline; "
            "sys.exit(1 if 'lara_amd.splatio' in sys.modules else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
