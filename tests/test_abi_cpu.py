"""The C-ABI library builds for gfx950 without a GPU, loads, and exports every symbol that
the headers under include/ declare; the Python copy of the ABI (lara_amd/_native.py) agrees with the headers, function by
function and struct by struct.  No compute calls here (no GPU)."""
import ctypes
import os
import re

import pytest

from lara_amd import _native, rasterizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the headers, read as what they are: plain C with one prototype style ----------------------------------------------------
_C_KINDS = {"int": "i", "int32_t": "i", "uint32_t": "i", "int64_t": "l", "float": "f", "double": "d"}
_STRUCT_RE = r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;"


def _c_kind(decl):
    """Kind of a C type without its declarator's name: 'p' any pointer or array parameter, 'i' int / int32_t, 'l' int64_t,
    'f' float, 'd' double; anything else (a struct by value) is returned as written."""
    decl = " ".join(decl.replace("const", " ").split())
    return "p" if "*" in decl or "[" in decl else _C_KINDS.get(decl, decl)


def header_texts(include_dir=None):
    include_dir = include_dir or os.path.join(ROOT, "include")
    texts = {}
    for hdr in sorted(os.listdir(include_dir)):
        if hdr.endswith(".h"):
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(include_dir, hdr)).read(), flags=re.S)
            texts[hdr] = re.sub(r"//[^\n]*", "", text)
    return texts


def header_functions_by_file(include_dir=None):
    """{header file name: {name: (return kind, [parameter kinds])}} of every prototype: return 'i' / 'l' / 'z' (const char *)."""
    by_file = {}
    for hdr, text in header_texts(include_dir).items():
        out = by_file[hdr] = {}
        text = re.sub(_STRUCT_RE, "", text, flags=re.S)
        text = re.sub(r"^\s*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
        for stmt in text.split(";"):
            m = re.match(r"[\s}]*((?:const\s+)?\w+[\s*]+)(lara2dgs_\w+|lara_\w+)\s*\((.*)\)\s*$", stmt, flags=re.S)
            if m is None:
                assert not re.search(r"\blara\w*\s*\(", stmt), f"a prototype this parser does not read: {stmt!r}"
                continue
            ret, name, params = m.group(1), m.group(2), " ".join(m.group(3).split())
            kinds = []
            if params not in ("", "void"):
                for p in params.split(","):
                    d = re.match(r"(.*?)(\w+)\s*(\[[^\]]*\])?$", p.strip())
                    kinds.append(_c_kind(d.group(1) + (d.group(3) or "")))
            assert not any(name in fns for fns in by_file.values()), f"{name} is declared twice"
            out[name] = ("z" if "char" in ret else _c_kind(ret), kinds)
    return by_file


def header_functions(include_dir=None):
    """{name: (return kind, [parameter kinds])} over all headers."""
    return {name: sig for fns in header_functions_by_file(include_dir).values() for name, sig in fns.items()}


def header_structs(include_dir=None):
    """{typedef name: [(field, kind)]}; an array field's kind carries its length, e.g. 'l[4]' (macros resolved)."""
    out = {}
    for text in header_texts(include_dir).values():
        macros = dict(re.findall(r"#define\s+(\w+)\s+\(?(-?\d+)\)?\s", text))
        for m in re.finditer(_STRUCT_RE, text, flags=re.S):
            fields = []
            for stmt in m.group(1).split(";"):
                names = [d.strip() for d in " ".join(stmt.split()).split(",")]
                if names == [""]:
                    continue
                first = re.match(r"(.*?)(\w+)\s*(?:\[(\w+)\])?$", names[0])
                base = first.group(1).replace("*", " ")
                decls = [(first.group(1), first.group(2), first.group(3))]
                for more in names[1:]:                       # `int64_t a, b, c;`
                    d = re.match(r"(\**)\s*(\w+)\s*(?:\[(\w+)\])?$", more)
                    decls.append((base + d.group(1), d.group(2), d.group(3)))
                for ctype, field, length in decls:
                    fields.append((field, _c_kind(ctype) + (f"[{int(macros.get(length, length))}]" if length else "")))
            out[m.group(2)] = fields
    return out


def _ctypes_kind(t):
    """The same kinds for a ctypes type of the binding."""
    if isinstance(t, type) and issubclass(t, ctypes.Array):
        return f"{_ctypes_kind(t._type_)}[{t._length_}]"
    if isinstance(t, type) and issubclass(t, ctypes.Structure):
        return {cls: name for name, cls in _native.STRUCTS.items()}[t]
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents"):
        return "p"
    return {ctypes.c_int: "i", ctypes.c_int32: "i", ctypes.c_int64: "l", ctypes.c_float: "f", ctypes.c_double: "d"}[t]


def declared_functions():
    return sorted(header_functions())


def table_mismatches(include_dir=None):
    """Every disagreement between the signature table and the headers, as text."""
    declared, bad = header_functions(include_dir), []
    bad += [f"{n}: declared in a header, no row in the table" for n in sorted(set(declared) - set(_native._SIGS))]
    bad += [f"{n}: a row in the table, declared in no header" for n in sorted(set(_native._SIGS) - set(declared))]
    for name in sorted(set(declared) & set(_native._SIGS)):
        restype, argtypes, _ = _native._SIGS[name]
        ret = "z" if restype is ctypes.c_char_p else _ctypes_kind(restype)
        kinds = [_ctypes_kind(t) for t in argtypes]
        if (ret, kinds) != declared[name]:
            bad.append(f"{name}: header {declared[name]}, table {(ret, kinds)}")
    return bad


def test_signature_table_equals_the_headers():
    """Every function the headers declare has a row, every row a declaration, and they agree in the return type and, position by
    position, in the kind of every parameter (pointer / int32 / int64 / float)."""
    assert table_mismatches() == []             # (first: it names the function, the count below only counts)
    assert len(header_functions()) == len(_native._SIGS) == 196


# how many functions each header declares: a function that moves between headers, or a header that appears or goes, shows here
FUNCTIONS_PER_HEADER = {
    "lara2dgs.h": 16, "lara_batchfinish.h": 2, "lara_coarsedec.h": 3, "lara_depthsurface.h": 8, "lara_eval.h": 3, "lara_featvol.h": 3,
    "lara_finedec.h": 8, "lara_groupattn.h": 20, "lara_loss.h": 6, "lara_lpips.h": 4, "lara_meshalign.h": 3, "lara_meshbvh.h": 6, "lara_meshclean.h": 6,
    "lara_meshdist.h": 7, "lara_meshio.h": 8, "lara_meshmetrics.h": 7, "lara_meshray.h": 6, "lara_meshrender.h": 3,
    "lara_meshsign.h": 6, "lara_meshsimplify.h": 12, "lara_meshtexture.h": 7, "lara_meshtopo.h": 12, "lara_meshwind.h": 6,
    "lara_pointfeat.h": 7, "lara_rays.h": 1, "lara_splatadam.h": 2, "lara_splatdensify.h": 7, "lara_splatxform.h": 2,
    "lara_surface.h": 6, "lara_tsdf.h": 4, "lara_vit.h": 5,
}


def test_each_header_declares_its_pinned_number_of_functions():
    assert {hdr: len(fns) for hdr, fns in header_functions_by_file().items()} == FUNCTIONS_PER_HEADER
    assert sum(FUNCTIONS_PER_HEADER.values()) == 196
    assert [d for d in os.listdir(os.path.join(ROOT, "include")) if not d.endswith(".h")] == [], "include/ is flat"


def test_stream_flag_follows_the_prototype():
    """The helper appends the stream exactly where the prototype ends in `void *stream`."""
    seen = 0
    for text in header_texts().values():
        for name, params in re.findall(r"\b(lara2dgs_\w+|lara_\w+)\s*\(([^()]*)\)\s*;", text):
            assert _native._SIGS[name][2] == bool(re.search(r"void\s*\*\s*stream\s*$", params)), name
            seen += 1
    assert seen == 196


def test_a_changed_prototype_fails_the_table_check(tmp_path):
    """The check has teeth: a header that gains, loses or reorders a parameter disagrees with the table."""
    import shutil
    src = open(os.path.join(ROOT, "include", "lara_rays.h")).read()
    proto = re.search(r"int lara_build_rays_out\((.*?)\);", src, flags=re.S)
    params = [p.strip() for p in " ".join(proto.group(1).split()).split(",")]
    variants = {"gains": params[:1] + ["int32_t extra"] + params[1:], "loses": params[:2] + params[3:],
                "reorders": params[:3] + [params[4], params[3]] + params[5:]}
    for what, ps in variants.items():
        inc = tmp_path / what
        shutil.copytree(os.path.join(ROOT, "include"), inc)
        (inc / "lara_rays.h").write_text(src.replace(proto.group(0), f"int lara_build_rays_out({', '.join(ps)});"))
        assert [m for m in table_mismatches(str(inc)) if m.startswith("lara_build_rays_out:")], what


def test_struct_mirrors_equal_the_header_structs():
    """Every struct a header defines is mirrored once, with the header's field names in the header's order and the same kind
    (and array length) field by field."""
    structs = header_structs()
    assert sorted(structs) == sorted(_native.STRUCTS) and len(structs) == 13
    for name, cls in _native.STRUCTS.items():
        assert [(f, _ctypes_kind(t)) for f, t in cls._fields_] == structs[name], name
    assert structs["lara_lpips_net"][1] == ("layers", f"lara_lpips_layer[{_native.LPIPS_MAX_LAYERS}]")


def test_a_mistyped_table_row_fails_when_it_is_parsed():
    for row in ("i lara_x(q)", "i lara_x(s p)", "x lara_x(i)", "i lara_x(i*)", "i lara_x(i) extra", "i lara_x(i)\ni lara_x(i)"):
        with pytest.raises(ValueError):
            _native._parse_signatures(row)
    assert _native._parse_signatures("l lara_x(i*2 View s)")["lara_x"][1:] == (
        [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_native.View), ctypes.c_void_p], True)


# ---- the call helper, against a stand-in library object ---------------------------------------------------------------------
class _FakeLibrary:
    """Stands in for the loaded library: records what each function is called with and answers `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        if name == "lara2dgs_error_string":
            return lambda rc: b"invalid argument"
        if name == "lara2dgs_last_hip_error":
            return lambda: 7
        return lambda *a: (self.calls.append((name, a)), self.rc)[1]


@pytest.fixture
def fake_library(monkeypatch):
    import contextlib
    import torch

    class FakeStream:
        cuda_stream = 0x5EED

    lib = _FakeLibrary()
    lib.entered = []
    monkeypatch.setattr(torch.cuda, "device", lambda dev: (lib.entered.append(dev), contextlib.nullcontext())[1])
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: FakeStream())
    monkeypatch.setattr(_native, "_handle", lib)
    return lib


def test_call_passes_tensors_none_and_the_stream(fake_library):
    import torch
    t, u = torch.zeros(4), torch.zeros(3, dtype=torch.uint8)
    view = _native.ImageView()
    # a prototype that ends in `void *stream`: the stream is appended, the device entered; a tensor arrives as its data_ptr(),
    # None as NULL, a raw address as it is
    _native.call("lara2dgs_mark_visible", "dev0", 5, t, None, t.data_ptr() + 8, u)
    assert fake_library.calls.pop() == ("lara2dgs_mark_visible", (5, t.data_ptr(), None, t.data_ptr() + 8, u.data_ptr(), 0x5EED))
    assert fake_library.entered == ["dev0"]
    # one that does not: nothing is appended; ints, floats and struct instances pass through as they are
    layout = _native.GradLayout()
    _native.call("lara2dgs_get_grad_layout", None, 1, 2, 3, 4, 5, 6, layout)
    assert fake_library.calls.pop() == ("lara2dgs_get_grad_layout", (1, 2, 3, 4, 5, 6, layout))
    _native.call("lara_lpips_forward", "dev0", None, 1, 2, 3, view, view, 2.0, -1.0, t, u)
    name, args = fake_library.calls.pop()
    assert args[4] is view and args[6:8] == (2.0, -1.0) and args[-1] == 0x5EED and len(args) == 11
    # a miscounted argument list never reaches the library
    with pytest.raises(TypeError, match="lara2dgs_mark_visible takes 6 arguments, got 5"):
        _native.call("lara2dgs_mark_visible", "dev0", 5, t, None, t)
    with pytest.raises(TypeError, match="lara2dgs_state_bytes takes 5 arguments, got 6"):
        _native.query("lara2dgs_state_bytes", 8, 16, 16, 1024, 0, 0)
    assert fake_library.calls == []


def test_call_and_query_raise_with_the_called_functions_own_name(fake_library):
    import torch
    fake_library.rc = -1
    with pytest.raises(RuntimeError, match=r"lara_amd: lara_voxel_rows failed: invalid argument \(hipError 7\)"):
        _native.call("lara_voxel_rows", "dev0", 1, 4, torch.zeros(1), None, None, 0)
    with pytest.raises(RuntimeError, match=r"lara_amd: lara_point_feats_workspace_bytes failed: invalid argument \(hipError 7\)"):
        _native.query("lara_point_feats_workspace_bytes", 4, 8, 8)
    with pytest.raises(ValueError, match="too small"):
        _native.query("lara_ms_ssim_workspace_floats", 1, 3, 8, 8, error=ValueError("too small"))
    fake_library.rc = 4096
    assert _native.query("lara_point_feats_workspace_bytes", 4, 8, 8) == 4096


def test_call_on_picks_the_device_entry_or_its_host_twin(fake_library):
    import torch
    t = torch.zeros(4)
    cuda, args = torch.device("cuda", 0), (t, t, None, None, 1, 2, 3, 4, t, t, None)
    # a GPU device: the entry itself, on that device, the stream appended
    _native.call_on("lara_batch_finish", cuda, *args)
    p = t.data_ptr()
    assert fake_library.calls.pop() == ("lara_batch_finish", (p, p, None, None, 1, 2, 3, 4, p, p, None, 0x5EED))
    assert fake_library.entered == [cuda]
    # the host: `<name>_host`, no stream, no device entered
    _native.call_on("lara_batch_finish", torch.device("cpu"), *args)
    assert fake_library.calls.pop() == ("lara_batch_finish_host", (p, p, None, None, 1, 2, 3, 4, p, p, None))
    assert fake_library.entered == [cuda] and fake_library.calls == []
    # a failed call carries the name of the function that was called
    fake_library.rc = -1
    with pytest.raises(RuntimeError, match=r"lara_amd: lara_batch_finish_host failed: invalid argument"):
        _native.call_on("lara_batch_finish", torch.device("cpu"), *args)


def test_no_cpu_path_check():
    import torch
    for t in (torch.zeros(1), torch.device("cpu")):
        with pytest.raises(RuntimeError, match=r"tensors must live on an MI355X \(HIP\) device; there is no CPU path"):
            _native.require_device(t)
    _native.require_device(torch.device("cuda", 0))


def test_header_declares_the_three_reference_entry_points():
    names = declared_functions()
    for must in ("lara2dgs_forward", "lara2dgs_backward", "lara2dgs_mark_visible"):
        assert must in names


def test_library_exports_every_declared_symbol(hip_lib):
    for name in declared_functions():
        assert hasattr(hip_lib, name), f"{name} declared in a header but not exported"
    assert hip_lib.lara2dgs_abi_version() == rasterizer.ABI_VERSION


def test_block_save_offsets_follow_the_save_area(hip_lib):
    """lara_groupblock_save_offsets (host code only): eleven increasing, 256-byte aligned offsets inside
    lara_groupblock_save_bytes; a wrong count or an unsupported shape is refused."""
    fn = hip_lib.lara_groupblock_save_offsets
    for scenes, R in ((1, 4), (3, 6), (4, 32)):
        M = scenes * R ** 3
        offs = (ctypes.c_int64 * 11)()
        assert fn(scenes, R, offs, 11) == 0
        o = list(offs)
        assert o[0] == 0 and o == sorted(set(o)) and all(v % 256 == 0 for v in o)
        sizes = [M * 512] * 4 + [M * 1024, M * 512, M * 1024, M * 1024, M * 1024, M * 512 + 512, M * 8]   # xn1 q kv o x1 xn2 z h x2 xn3 stats
        assert all(b - a >= n for a, b, n in zip(o, o[1:] + [hip_lib.lara_groupblock_save_bytes(scenes, R)], sizes))
    for bad in ((1, 4, 10), (1, 4, 12), (1, 5, 11), (1, 2, 11), (-1, 4, 11)):
        assert fn(bad[0], bad[1], offs, bad[2]) == -1
    assert fn(1, 4, None, 11) == -1


def test_vit_save_offsets_follow_the_save_area(hip_lib):
    """lara_vit_save_offsets (host code only): patches, xfin, stf, the first block's base, the block stride and the twelve
    per-block offsets -- increasing, 256-byte aligned, every region inside lara_vit_save_bytes with room for what the header
    says it holds; bad dims, a null array or a wrong count are refused."""
    fn = hip_lib.lara_vit_save_offsets

    def dims(N, views, H, W, C, F, depth, heads=None):
        d = _native.VitDims()
        d.N, d.views, d.H, d.W, d.C, d.F, d.depth, d.eps = N, views, H, W, C, F, depth, 1e-6
        d.heads = C // 64 if heads is None else heads
        return d
    rup = lambda v, m: (v + m - 1) // m * m
    offs = (ctypes.c_int64 * 17)()
    for case in ((1, 1, 16, 16, 64, 64, 1), (3, 1, 64, 128, 128, 192, 1), (2, 2, 112, 144, 320, 1280, 2), (3, 1, 128, 128, 1024, 256, 1),
                 (16, 4, 512, 512, 768, 3072, 12)):
        N, _, H, W, C, F, depth = case
        d = dims(*case)
        assert fn(ctypes.byref(d), offs, 17) == 0
        o = list(offs)
        total = hip_lib.lara_vit_save_bytes(ctypes.byref(d))
        T = 1 + (H // 16) * (W // 16)
        M, Mp, Tp, NH, Pp = N * T, rup(N * T, 128), rup(T, 64), N * C // 64, rup(N * (T - 1), 128)
        assert all(v % 256 == 0 for v in o)
        head, base, stride, blk = o[:3], o[3], o[4], o[5:]
        assert head[0] == 0 and head == sorted(set(head)) and blk[0] == 0 and blk == sorted(set(blk))
        assert base + depth * stride == total
        sizes = [Pp * 768 * 2, M * C * 4, M * 8]                                                    # patches xfin stf
        assert all(b - a >= n for a, b, n in zip(head, head[1:] + [base], sizes))
        hd = NH * Tp * 64 * 2
        sizes = [M * C * 4, Mp * C * 2, M * 8, hd, hd, hd, Mp * C * 2, NH * Tp * 4, M * C * 4, Mp * C * 2, M * 8, Mp * F * 2]
        assert all(b - a >= n for a, b, n in zip(blk, blk[1:] + [stride], sizes))                   # xin .. h
    good = (1, 1, 16, 16, 64, 64, 1)
    for n in (16, 18, 0, -1):
        assert fn(ctypes.byref(dims(*good)), offs, n) == -1
    assert fn(ctypes.byref(dims(*good)), None, 17) == -1 and fn(None, offs, 17) == -1
    for bad in ((0, 1, 16, 16, 64, 64, 1), (3, 2, 16, 16, 64, 64, 1), (1, 1, 24, 16, 64, 64, 1), (1, 1, 16, 16, 96, 64, 1),
                (1, 1, 16, 16, 1088, 64, 1), (1, 1, 16, 16, 64, 32, 1), (1, 1, 16, 16, 64, 64, 0), (1, 1, 16, 16, 64, 64, 65)):
        assert fn(ctypes.byref(dims(*bad)), offs, 17) == -1, bad
    assert fn(ctypes.byref(dims(*good, heads=2)), offs, 17) == -1


def test_sizes_and_layout_are_consistent(hip_lib):
    P, H, W = 524288, 512, 512
    cap = rasterizer.binning_capacity(P)
    L = rasterizer.StateLayout()
    assert hip_lib.lara2dgs_get_state_layout(P, H, W, cap, 0, ctypes.byref(L)) == 0
    assert L.total == hip_lib.lara2dgs_state_bytes(P, H, W, cap, 0)
    offs = [L.header, L.geom, L.point_list, L.ranges, L.final_T, L.n_contrib, L.total]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    assert L.point_list - L.geom >= P * 80 and L.ranges - L.point_list >= cap * 4
    assert hip_lib.lara2dgs_scratch_bytes(P, H, W, cap, 0) >= cap * 8
    assert hip_lib.lara2dgs_state_bytes(-1, H, W, cap, 0) < 0


def test_forward_only_state_is_the_lists_and_the_surfel_records(hip_lib):
    """A forward-only call (inference: evaluation.py:129, tools/meshExtractor.py:85) keeps nothing for a backward: every
    section only the backward reads has size 0, the sections the forward's own kernels use keep their offsets."""
    P, H, W = 524288, 512, 512
    cap = rasterizer.binning_capacity(P)
    full, short = rasterizer.StateLayout(), rasterizer.StateLayout()
    assert hip_lib.lara2dgs_get_state_layout(P, H, W, cap, 0, ctypes.byref(full)) == 0
    assert hip_lib.lara2dgs_get_state_layout(P, H, W, cap, 1, ctypes.byref(short)) == 0
    for name in ("header", "geom", "cullbox", "point_list", "ranges", "tile_order", "pair_base"):
        assert getattr(full, name) == getattr(short, name), name
    backward_only = ("pair_base", "pair_pos", "final_T", "n_contrib", "seg_base", "seg_cnt", "bwd_order", "bwd_items", "ckpt",
                     "pair_mask", "tile_maxc", "seg_cost")
    assert all(getattr(short, n) == short.total for n in backward_only)
    assert short.total == hip_lib.lara2dgs_state_bytes(P, H, W, cap, 1)
    assert short.total < 0.4 * full.total and short.total >= P * 96 + cap * 4        # 67 MB of 182 at LaRa's sizes
    assert hip_lib.lara2dgs_scratch_bytes(P, H, W, cap, 1) < 0.2 * hip_lib.lara2dgs_scratch_bytes(P, H, W, cap, 0)
    assert hip_lib.lara2dgs_scratch_bytes(P, H, W, cap, 1) >= P * 16 + cap * 8


def test_backward_refuses_a_forward_only_view(hip_lib):
    v = rasterizer._View()
    v.P, v.image_height, v.image_width, v.sh_degree, v.forward_only = 8, 16, 16, 1, 1
    dummy = ctypes.c_void_p(4096)        # (never dereferenced: the argument check comes first)
    v.bg = v.viewmatrix = v.projmatrix = v.campos = 4096
    assert hip_lib.lara2dgs_backward(ctypes.byref(v), *([dummy] * 20)) == -1
    views = (rasterizer._View * 2)(v, v)
    assert hip_lib.lara2dgs_backward_views(2, views, *([dummy] * 10), 256, dummy, 256, dummy, dummy) == -1


def test_invalid_arguments_return_error_codes_not_crashes(hip_lib):
    v = rasterizer._View()
    v.P, v.image_height, v.image_width, v.sh_degree = 8, 16, 16, 7   # bad degree, null matrices
    rc = hip_lib.lara2dgs_forward(ctypes.byref(v), *([None] * 13))
    assert rc == -1 and hip_lib.lara2dgs_error_string(rc) == b"invalid argument"
    assert hip_lib.lara2dgs_mark_visible(4, None, None, None, None, None) == -1


def test_library_exports_no_setters(hip_lib):
    """the library keeps no global state.  Rounds 2-4 shipped three process-wide setters (view lanes,
    forward split, per-view launches) for A/B runs; they are gone with the paths they selected."""
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", rasterizer.LIB_PATH], capture_output=True, text=True).stdout
    assert "lara2dgs_forward_views" in syms
    names = [l.split()[-1] for l in syms.splitlines() if "lara" in l]
    assert not [n for n in names if "_set_" in n.replace("l2d_set_hip_error", "")], syms
    # ... with ONE documented exception: the per-kernel event log bench.py's roofline leg switches on (include/lara2dgs.h says
    # so); any other exported name that reads like a switch fails here
    switches = [n for n in names if re.search(r"_(enable|disable|configure|option|mode)\b|_(enable|disable)_", n)]
    assert switches == ["lara2dgs_profile_enable"], switches


def test_operator_refuses_cpu_tensors_and_has_no_fallback(hip_lib):
    import torch
    from tests.helpers import small_scene, raster_settings
    from lara_amd import GaussianRasterizer
    act, cams = small_scene(grid=4, size=32)
    rs = raster_settings(cams[0], (1, 1, 1), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianRasterizer(rs)(means3D=act["means3D"], means2D=None, opacities=act["opacities"],
                               shs=act["shs"], scales=act["scales"], rotations=act["rotations"])


def test_product_path_never_imports_the_oracle():
    for pkg in ("lara_amd", "diff_surfel_rasterization"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, pkg)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp")):
                    src = open(os.path.join(dirpath, f)).read()
                    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                    assert "surfel_oracle" not in src, f


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    """No CPU fallback anywhere: without liblara2dgs.so every entry point raises (on the GPU box that means a failed
    build is visible at the first call, not a silent torch path)."""
    import pytest
    import lara_amd.rasterizer as rz
    monkeypatch.setattr(rz, "LIB_PATH", str(tmp_path / "liblara2dgs.so"))
    monkeypatch.setattr(rz, "_lib", None, raising=False)
    with pytest.raises(RuntimeError, match="HIP library not found"):
        rz.load_library()


def test_buffer_sizes_are_quantised_in_the_surfel_count(hip_lib):
    """The fine pass renders a subset whose size changes every step; buffers sized from the exact count would be a new
    allocation size per call.  Sizes come from the count rounded up, and a buffer sized for the rounded count holds the
    exact one."""
    from lara_amd import rasterizer
    assert rasterizer._sizing_P(261600) == rasterizer._sizing_P(262144) == rasterizer._sizing_P(262700) == 294912
    assert rasterizer._sizing_P(524288) == 557056 and rasterizer._sizing_P(0) == 1024 and rasterizer._sizing_P(1500) == 2048
    assert rasterizer._sizing_P(32768) == 32768 and rasterizer._sizing_P(32769) == 98304 and rasterizer._sizing_P(98305) == 163840
    for P in (1, 1023, 32768, 32769, 70000, 98304, 262100, 524288):
        q = rasterizer._sizing_P(P)
        cap = rasterizer.binning_capacity(P)
        assert q >= P and cap == rasterizer.binning_capacity(q)
        for fo in (0, 1):
            assert hip_lib.lara2dgs_state_bytes(q, 512, 512, cap, fo) >= hip_lib.lara2dgs_state_bytes(P, 512, 512, cap, fo)
            assert hip_lib.lara2dgs_scratch_bytes(q, 512, 512, cap, fo) >= hip_lib.lara2dgs_scratch_bytes(P, 512, 512, cap, fo)


def test_capacity_policy_follows_the_measured_pair_counts(monkeypatch):
    """Host logic of the workspace policy (rasterizer.py): capacities sit on the grid {2^k, 1.5 * 2^k}, start from
    LARA2DGS_DUP_FACTOR pairs per (quantised) surfel, and follow twice the largest count of the size class's last `_HISTORY`
    calls -- a window: a spike ages out and the capacity comes back down (round 5 kept a high-water mark for the life of the
    process)."""
    import torch
    from lara_amd import rasterizer as rz
    monkeypatch.delenv("LARA2DGS_DUP_FACTOR", raising=False)
    rz.reset_capacity_history()
    assert [rz._cap_grid(n) for n in (1, 1 << 20, (1 << 20) + 1, 3 << 19, (3 << 19) + 1, 3_090_000, 1 << 40)] == \
        [1 << 20, 1 << 20, 3 << 19, 3 << 19, 1 << 21, 3 << 20, 0xFFFFFFFF]
    dev = torch.device("cuda", 0)
    P, H, W = 524288, 512, 512
    b = rz._bucket(dev, P, H, W)
    assert b == (0, 557056, 512, 512) == rz._bucket(dev, 524000, H, W)
    assert rz.binning_capacity(P) == rz.binning_capacity(P, H, W, dev) == 3 << 20      # 4 x 557 056 -> 3 Mi
    rz.note_pair_count(b, 1_545_000)                                # LaRa's init distribution
    assert rz.binning_capacity(P, H, W, dev) == 3 << 20
    rz.note_pair_count(b, 4_600_000)                                # surfels e x larger
    assert rz.binning_capacity(P, H, W, dev) == 3 << 22
    assert rz.binning_capacity(P, 1024, 1024, dev) == 3 << 20      # another size class: its own history
    rep = rz.capacity_report()
    assert rep[b] == {"D_max": 4_600_000, "calls": 2, "capacity": 3 << 22, "longest_list": 0} and "reruns" in rep
    for _ in range(rz._HISTORY - 1):                                # the spike is still inside the window ...
        rz.note_pair_count(b, 1_545_000)
    assert rz.binning_capacity(P, H, W, dev) == 3 << 22
    rz.note_pair_count(b, 1_545_000)                                # ... and now it is not
    assert rz.binning_capacity(P, H, W, dev) == 3 << 20 and rz.capacity_report()[b]["calls"] == rz._HISTORY
    monkeypatch.setenv("LARA2DGS_DUP_FACTOR", "16")
    assert rz.binning_capacity(P) == 3 << 22
    rz.reset_capacity_history()


def test_a_forward_that_does_not_fit_is_repeated_before_the_operator_returns(monkeypatch):
    """Host logic of `_run_forward` (no GPU: the enqueue, the pinned words and the event are stand-ins): the forward goes out at
    the capacity the class's history asks for; the counts the scan kernel would have stored are read; an overflow repeats the SAME
    forward at twice the count it reported -- before anything is returned -- and every count lands in the history."""
    import numpy as np
    import torch
    from lara_amd import rasterizer as rz
    monkeypatch.delenv("LARA2DGS_DUP_FACTOR", raising=False)
    rz.reset_capacity_history()

    class FakeCounts:
        def __init__(self, n):
            self.np = np.zeros((max(n, 16), 4), dtype=np.uint32)
            self.ptr = 0xABC0

    class FakeEvent:
        def record(self): pass
        def query(self): return True

    fake = FakeCounts(8)
    monkeypatch.setattr(rz, "_counts", lambda n: fake)
    monkeypatch.setattr(torch.cuda, "Event", FakeEvent)
    bucket = (0, 557056, 512, 512)
    D_per_view = [1_500_000, 7_000_000, 1_400_000]        # view 1 outgrows the 3 Mi pairs a new class starts from
    calls = []

    def enqueue(cap, counts_ptr):
        assert counts_ptr == fake.ptr and not fake.np[:3, 3].any(), "the ready words are cleared before every launch"
        calls.append(cap)
        for i, D in enumerate(D_per_view):                 # what tile_scan stores
            fake.np[i] = (D, int(D > cap), 4000, 1)
        return "state%d" % len(calls), (lambda: None), ("sb", "qb")

    reruns = rz._reruns
    state, cap, extra, D = rz._run_forward(bucket, 3, enqueue)
    assert calls == [3 << 20, 1 << 24] and cap == 1 << 24 and state == "state2" and extra == ("sb", "qb") and D == 7_000_000      # 2 x 7 M on the grid
    assert rz._reruns == reruns + 1 and list(rz._hist[bucket]) == [7_000_000, 7_000_000]
    # the next call of the class starts where this one ended: no repeat
    calls.clear()
    state, cap, _, _ = rz._run_forward(bucket, 3, enqueue)
    assert calls == [1 << 24] and rz._reruns == reruns + 1
    # beyond the 32-bit pair index there is nothing to repeat with: the one way a call can still fail, and it says so
    D_per_view[1] = 0xFFFFFFF0

    def enqueue_huge(cap, counts_ptr):
        for i, D in enumerate(D_per_view):
            fake.np[i] = (D, 1, 4000, 1)
        return "s", (lambda: None), None
    monkeypatch.setattr(rz, "_next_capacity", lambda b: 0xFFFFFFFF)
    with pytest.raises(RuntimeError, match="32-bit pair index"):
        rz._run_forward(bucket, 3, enqueue_huge)
    rz.reset_capacity_history()


# ---- the HIP layer's one launch-and-check path (lara_amd/csrc/launch.h), checked on the sources as text -------------------------

CSRC = os.path.join(ROOT, "lara_amd", "csrc")
LAUNCH_HEADER = "launch.h"
# launches kept outside the shared helper on purpose: (file, reason); at most five
LAUNCH_ALLOW_LIST = ()
# every profile label and how often it is written: the first argument of L2D_PROF, of the labeled launch L2D_LAUNCH and of
# vit.hip's VT_PROF alias.  tools/* and tests/test_pipeline.py read profiles by these names.  (gb_ln2, gb_ln3, gb_mlp1, gb_mlp2 and the
# second gbb_dx_conv / gbb_dx_mlp, third and fourth gbb_ln_bwd were written in preprocessor branches no shipped build compiled; they
# left with those branches.)
PROFILE_LABELS = {
    "activate_bwd": 1, "activate_fwd": 1, "build_rays": 1, "bwd_order": 1, "coarse_decoder_bwd": 1,
    "coarse_decoder_fwd": 1, "composite_bwd": 1, "composite_bwd_color": 1, "composite_fwd": 1,
    "composite_fwd_only": 1, "eval_quantize": 1, "eval_scores": 1, "featvol_grad_transpose": 1, "featvol_index": 1,
    "featvol_linear": 2, "featvol_modln": 1, "featvol_param_grads": 1, "featvol_sample_tokens": 1,
    "featvol_sample_volume": 1, "featvol_token_bwd": 1, "fine_decoder_bwd": 1, "fine_decoder_fwd": 1,
    "fine_decoder_wgrad": 1, "fine_ln_bwd": 1, "fine_ln_fwd": 1, "ga_fused": 1, "ga_gemm_kv": 1, "gb_conv3d": 2,
    "gb_mlp_fused": 1, "gbb_dw_conv": 1, "gbb_dw_linear": 1,
    "gbb_dx_attn": 1, "gbb_dx_conv": 1, "gbb_dx_mlp": 1, "gbb_ln_bwd": 2, "gbb_recompute": 1, "gbt_forward": 1,
    "loss_terms_bwd": 1, "loss_terms_fwd": 1, "lpips_conv2d": 1, "lpips_forward": 1, "lpips_maxpool": 1,
    "mesh_area_finish": 1, "mesh_cluster_stats": 1, "mesh_compact_rows": 1, "mesh_crop": 1, "mesh_edge_insert": 1,
    "mesh_edge_owner": 1, "mesh_hook": 1, "mesh_jump": 1, "mesh_keep_clusters": 1, "mesh_remap": 1, "ms_ssim_bwd": 1,
    "ms_ssim_fwd": 1, "point_feats_bwd": 1, "point_feats_fwd": 1, "point_feats_pack": 2, "preprocess_bwd": 1,
    "preprocess_bwd_views": 1, "preprocess_fwd": 1, "preprocess_fwd_views": 1, "scatter": 1, "subset_compact": 1,
    "subset_pair_base": 1, "surface_bwd": 1, "surface_fwd": 1, "take_rows_bwd": 1, "take_rows_fwd": 1, "tile_scan": 2,
    "tile_sort": 1, "tsdf_integrate": 1, "tsdf_integrate_blocks": 1, "tsdf_mesh_count": 1, "tsdf_mesh_emit": 1,
    "tsdf_touch": 1, "vit_attention": 11, "vit_elementwise": 25, "vit_layernorm": 9, "vit_products": 14,
    "voxel_rows_bwd": 1, "voxel_rows_fwd": 1, "vt_deconv": 1, "vt_ln": 1, "vtb_head": 1,
}


def _csrc_sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                out[name] = f.read()
    return out


def _first_argument(text, i):
    """text[i:] up to the first comma or closing bracket at depth 0 (string literals skipped)."""
    depth, j = 0, i
    while True:
        c = text[j]
        if c == '"':
            j = text.index('"', j + 1)
        elif c in "([{":
            depth += 1
        elif c in ")]}":
            if depth == 0:
                break
            depth -= 1
        elif c == "," and depth == 0:
            break
        j += 1
    return text[i:j]


def _profile_labels(sources):
    labels = {}
    for text in sources.values():
        for m in re.finditer(r"\b(?:L2D_PROF|VT_PROF|L2D_LAUNCH)\(", text):
            for lit in re.findall(r'"([^"]*)"', _first_argument(text, m.end())):
                labels[lit] = labels.get(lit, 0) + 1
    return labels


def test_launch_failures_go_through_the_one_checked_path():
    src = _csrc_sources()
    assert len(LAUNCH_ALLOW_LIST) <= 5
    allowed = {f for f, _ in LAUNCH_ALLOW_LIST}
    # (a) the status is produced by the shared helpers alone; abi.hip only names it in lara2dgs_error_string
    holders = sorted(n for n, t in src.items() if "LARA2DGS_E_LAUNCH" in t)
    assert holders == ["abi.hip", LAUNCH_HEADER], holders
    abi = src["abi.hip"]
    start = abi.index("lara2dgs_error_string")
    body = abi[start:abi.index("\n}", start)]
    assert abi.count("LARA2DGS_E_LAUNCH") == 1 and "case LARA2DGS_E_LAUNCH:" in body
    # (b) kernels are launched inside the shared helper only
    for token in ("hipLaunchKernelGGL", "<<<"):
        where = sorted(n for n, t in src.items() if token in t and n != LAUNCH_HEADER and n not in allowed)
        assert where == [], (token, where)
    assert "hipLaunchKernelGGL" in src[LAUNCH_HEADER]
    # (c) and the launch error is read there only
    assert sorted(n for n, t in src.items() if "hipGetLastError" in t) == [LAUNCH_HEADER]
    # (d) the profile labels are the ones the tools know, each as often as before
    assert _profile_labels(src) == PROFILE_LABELS
