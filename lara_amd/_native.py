"""The one ctypes binding of ``liblara2dgs.so``: the loader, the mirrors of the header structs, the signature of every function
the headers under ``include/`` declare, and the checked call the modules of this package go through.

The headers are the contract; ``SIGNATURES`` and the ``Structure`` classes below are its Python copy, and
``tests/test_abi_cpu.py`` holds one against the other (names, order, kinds) without the library or a device.  A new entry point
is declared in a header and gets one row here.

PyTorch only owns memory and the stream.  There is no CPU path and no fallback: without the library, or with tensors that are
not on the GPU, the callers raise.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LARA2DGS_LIB: another build of the same library -- kernel A/B experiments, `make -C lara_amd/csrc VARIANT=<tag> EXTRA=...`; never a CPU path)
LIB_PATH = os.environ.get("LARA2DGS_LIB") or os.path.join(_HERE, "liblara2dgs.so")
ABI_VERSION = 10

_vp, _i32, _i64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float


def _struct(name, *groups):
    """A ``ctypes.Structure`` from (ctype, "field names") groups in declaration order."""
    return type(name, (ctypes.Structure,), {"_fields_": [(n, t) for t, names in groups for n in names.split()]})


_BLOCK_FIELDS = "ln1_w ln1_b wq wkv wo ln2_w ln2_b w1 b1 w2 b2 ln3_w ln3_b wconv"

# include/lara2dgs.h
View = _struct("View", (_i32, "P sh_degree sh_coeffs image_height image_width"), (_f32, "tanfovx tanfovy scale_modifier"),
               (_i32, "prefiltered debug forward_only"), (_i64, "capacity"), (_vp, "bg viewmatrix projmatrix campos counts_out"))
StateLayout = _struct("StateLayout", (_i64, "header geom cullbox point_list ranges tile_order pair_base pair_pos final_T n_contrib "
                                            "seg_base seg_cnt bwd_order bwd_items ckpt pair_mask tile_maxc seg_cost total"))
Subset = _struct("Subset", (_vp, "coarse_state"), (_i64, "coarse_state_stride coarse_capacity"),
                 (_i32, "coarse_P coarse_forward_only"), (_vp, "inv"))
GradLayout = _struct("GradLayout", (_i64, "means3D means2D shs colors opacities scales rotations transmat total"))
# include/lara_featvol.h
FeatvolDims = _struct("FeatvolDims", (_i32, "B V C E h w R img_w img_h"), (_f32, "eps"), (_i64 * 4, "x_stride"))
# include/lara_groupattn.h
BlockWeights = _struct("BlockWeights", (_vp, _BLOCK_FIELDS), (_f32, "eps"))
BlockWeightsT = _struct("BlockWeightsT", (_vp, "wq_t wkv_t wo_t w1_t w2_t wconv_t"))
BlockGrads = _struct("BlockGrads", (_vp, _BLOCK_FIELDS))
# include/lara_loss.h (element strides)
ImageView = _struct("ImageView", (_vp, "p"), (_i64, "sN sC sY sV sX"), (_i32, "Wv"))
# include/lara_lpips.h
LPIPS_MAX_LAYERS, LPIPS_TAPS = 16, 5
LpipsLayer = _struct("LpipsLayer", (_vp, "w bias"), (_i32, "cin cout k stride pad pool_k pool_s tap"))
LpipsNet = _struct("LpipsNet", (_i32, "n_layers"), (LpipsLayer * LPIPS_MAX_LAYERS, "layers"), (_vp * LPIPS_TAPS, "lin"),
                   (_f32 * 3, "shift"), (_f32 * 3, "scale"))
# include/lara_pointfeat.h
RowsItem = _struct("RowsItem", (_vp, "src dst"), (_i32, "width"))
# include/lara_vit.h
VitDims = _struct("VitDims", (_i32, "N views H W C heads F depth"), (_f32, "eps"), (_i64 * 5, "img_stride"))

STRUCTS = {"lara2dgs_view": View, "lara2dgs_state_layout": StateLayout, "lara2dgs_subset": Subset,
           "lara2dgs_grad_layout": GradLayout, "lara_featvol_dims": FeatvolDims, "lara_groupblock_weights": BlockWeights,
           "lara_groupblock_weights_t": BlockWeightsT, "lara_groupblock_grads": BlockGrads, "lara_image_view": ImageView,
           "lara_lpips_layer": LpipsLayer, "lara_lpips_net": LpipsNet, "lara_rows_item": RowsItem, "lara_vit_dims": VitDims}

# One row per declared function: `<return> <name>(<parameters>)`.  Returns: i = int / int32_t, l = int64_t, z = const char *.
# Parameters: i = int32_t / int, l = int64_t, f = float, d = double, p = any pointer (device memory, or a host array where the header says
# so), s = the trailing `void *stream`, a struct's name = a pointer to that struct (an instance is passed by reference, an
# array of them as it is); `x*N` repeats x N times.
SIGNATURES = """
# include/lara2dgs.h
i lara2dgs_abi_version()
z lara2dgs_error_string(i)
i lara2dgs_last_hip_error()
l lara2dgs_state_bytes(i*3 l i)
l lara2dgs_scratch_bytes(i*3 l i)
i lara2dgs_get_state_layout(i*3 l i StateLayout)
i lara2dgs_forward(View p*12 s)
i lara2dgs_backward(View p*19 s)
i lara2dgs_forward_views(i View p*11 l p l s)
i lara2dgs_forward_views_subset(i View p*11 l p l Subset s)
i lara2dgs_get_grad_layout(i*6 GradLayout)
i lara2dgs_backward_views(i View p*10 l p l p s)
i lara2dgs_mark_visible(i p*4 s)
i lara2dgs_profile_enable(i)
i lara2dgs_selftest(i p p s)
i lara2dgs_profile_collect(p i p i)
# include/lara_batchfinish.h
i lara_batch_finish(p*4 l*4 p*3 s)
i lara_batch_finish_host(p*4 l*4 p*3)
# include/lara_coarsedec.h
l lara_coarse_decoder_padded_rows(l)
i lara_coarse_decoder_forward(i*3 p*7 f f p*5 s)
i lara_coarse_decoder_backward(i*3 p*19 s)
# include/lara_depthsurface.h
l lara_depthsurface_backproject_workspace_bytes(i*3)
i lara_depthsurface_backproject_count(i*3 p p i i f p p s)
i lara_depthsurface_backproject_emit(i*3 p p i i f p p i p f p*4 s)
l lara_depthsurface_thin_workspace_bytes(i i)
i lara_depthsurface_thin(i p p f i p*5 s)
i lara_depthsurface_observe(i p i*3 p p i f p p f i p s)
l lara_depthsurface_reduce_workspace_bytes(i)
i lara_depthsurface_reduce(i i p*5 i p*3 s)
# include/lara_eval.h
l lara_eval_workspace_doubles(i*6)
i lara_eval_scores(i*3 ImageView ImageView p i*3 p*3 i i p*3 s)
i lara_eval_quantize_frames(i*3 l l p*5 s)
# include/lara_featvol.h
l lara_featvol_workspace_bytes(FeatvolDims)
i lara_featvol_forward(FeatvolDims p*10 i p p s)
i lara_featvol_backward(FeatvolDims p*10 i p*7 s)
# include/lara_finedec.h
i lara_fine_decoder_forward(i p*8 s)
i lara_fine_decoder_backward(i p*14 s)
i lara_fine_wgrad_floats()
l lara_fine_wgrad_workspace_bytes(i)
i lara_fine_decoder_wgrad(i p*8 s)
i lara_fine_ln_blocks(i)
i lara_fine_ln_forward(i p*3 f p p s)
i lara_fine_ln_backward(i p*6 s)
# include/lara_groupattn.h
l lara_groupattn_workspace_bytes(i)
i lara_groupattn_forward(i i p*4 f p*5 s)
l lara_groupblock_workspace_bytes(i i)
i lara_groupblock_forward(i*3 p p BlockWeights p s)
i lara_voltrans_head_forward(i i p*3 f p p i p p s)
i lara_tokens_from_volume(i*3 p p s)
i lara_volume_from_tokens(i*3 p p s)
i lara_gemm_nt_bf16(i*3 p*3 i s)
i lara_batched_transpose(i*3 p p i s)
l lara_groupblock_backward_workspace_bytes(i i)
l lara_groupblock_save_bytes(i i)
i lara_groupblock_forward_train(i*3 p*3 BlockWeights p s)
i lara_groupblock_backward(i*3 p p BlockWeights BlockWeightsT p*3 BlockGrads i p i p s)
l lara_voltrans_head_backward_workspace_bytes(i*3)
i lara_voltrans_head_backward(i i p*3 f p i p*7 s)
i lara_groupblock_save_offsets(i i p i)
l lara_gemm_tn_workspace_bytes()
i lara_gemm_tn_bf16(i*3 p*4 s)
i lara_layernorm256_backward(i p*3 f p*5 s)
i lara_groupattn_core_backward(i p*5 s)
# include/lara_loss.h
l lara_loss_partial_floats(l)
i lara_loss_terms_forward(i*4 p*9 s)
i lara_loss_terms_backward(i*4 p*12 s)
l lara_ms_ssim_workspace_floats(i*4)
i lara_ms_ssim_forward(i*4 ImageView ImageView p*3 s)
i lara_ms_ssim_backward(i*4 ImageView ImageView p p ImageView p s)
# include/lara_lpips.h
l lara_lpips_workspace_bytes(LpipsNet i*3)
i lara_lpips_forward(LpipsNet i*3 ImageView ImageView f f p p s)
i lara_lpips_conv2d(i*9 p*4 s)
i lara_lpips_maxpool(i*6 p p s)
# include/lara_meshalign.h
i lara_meshalign_transform(i p*3 d p p s)
l lara_meshalign_accumulate_workspace_bytes(i)
i lara_meshalign_accumulate(i*3 p*6 f p*3 s)
# include/lara_meshbvh.h
l lara_meshbvh_bytes(i)
i lara_meshbvh_layout(i p)
i lara_meshbvh_keys(i i p*3 s)
i lara_meshbvh_build(i i p*3 s)
i lara_meshbvh_query(i p*5 s)
i lara_meshbvh_box_bound_host(l p*3)
# include/lara_meshclean.h
i lara_mesh_crop(l l p*5 s)
i lara_mesh_compact_rows(l i p*4 s)
i lara_mesh_cluster_labels(l p l p*6 s)
i lara_mesh_cluster_stats(l l p*4 l p*5 s)
i lara_mesh_keep_clusters(l l p*7 s)
i lara_mesh_remap(l l p*4 s)
# include/lara_meshdist.h
i lara_meshdist_grid_resolution(i)
l lara_meshdist_grid_bytes(i)
i lara_meshdist_build(i i p*3 s)
l lara_meshdist_query_workspace_bytes(i)
i lara_meshdist_query(i p*7 s)
i lara_meshdist_face_normals(i i p*3 s)
i lara_meshdist_point_triangle_host(l p*4)
# include/lara_meshio.h
l lara_meshio_obj_workspace_bytes(l l)
i lara_meshio_obj_lengths(l p p l p i p s)
i lara_meshio_obj_emit(l p p l p i p p s)
l lara_meshio_ply_body_bytes(l l i i)
l lara_meshio_ply_workspace_bytes()
i lara_meshio_ply_pack(l p*3 l p i p p s)
i lara_meshio_format_f32_host(l p*3)
i lara_meshio_format_u32_host(l p*3)
# include/lara_meshmetrics.h
l lara_meshmetrics_sample_workspace_bytes(i)
i lara_meshmetrics_sample_surface(i i p p i i p*6 s)
i lara_meshmetrics_grid_resolution(i)
l lara_meshmetrics_nearest_workspace_bytes(i i)
i lara_meshmetrics_nearest(i i p*6 s)
l lara_meshmetrics_reduce_workspace_bytes(i)
i lara_meshmetrics_reduce(i i p*4 i p*3 s)
# include/lara_meshray.h
i lara_meshray_cast(i p*8 s)
i lara_meshray_cast_other_order(i p*8 s)
i lara_meshray_occluded(i p*6 s)
i lara_meshray_visible(i p p i p f p p s)
i lara_meshray_raytri_host(l p*8)
i lara_meshray_box_entry_host(l p*6)
# include/lara_meshrender.h
l lara_meshrender_workspace_bytes(i*5)
i lara_meshrender_section_offsets(i*5 p)
i lara_meshrender_views(i*5 p*6 f p i p*7 s)
# include/lara_meshsign.h
i lara_meshsign_rows(i p i p*3 s)
i lara_meshsign_vote(i i p p i p*4 s)
i lara_meshsign_counts(i p*5 s)
i lara_meshsign_volume(p p s)
i lara_meshsign_cross_host(l p*6)
i lara_meshsign_rows_host(i p i l p*3)
# include/lara_meshsimplify.h
l lara_meshsimplify_cells_workspace_bytes(l)
i lara_meshsimplify_cells(l p f p*5 s)
i lara_meshsimplify_clusters(l p*5 s)
l lara_meshsimplify_triangles_workspace_bytes(l)
i lara_meshsimplify_triangles(l*3 p*8 s)
i lara_meshsimplify_corner_keys(l l p*5 s)
i lara_meshsimplify_bucket_count(l l p p s)
l lara_meshsimplify_bucket_workspace_bytes(l l)
i lara_meshsimplify_bucket_fill(l l p*4 s)
i lara_meshsimplify_sums(l*3 p*7 i p*3 s)
i lara_meshsimplify_solve(l l i p*4 f p*4 s)
i lara_meshsimplify_vertex_map(l l p*4 s)
# include/lara_meshtexture.h
i lara_meshtexture_atlas_size(i*3 p)
i lara_meshtexture_texels(i*4 p*5 s)
i lara_meshtexture_texels_host(i*4 p*5)
i lara_meshtexture_bake(i*4 p*5 i*3 p*5 f f i*3 p f*3 p*3 s)
i lara_meshtexture_bake_host(i*4 p*5 i*3 p*5 f f i*3 p f*3 p*3)
i lara_meshtexture_sample(i*3 l p*3 i f*3 p s)
i lara_meshtexture_sample_host(i*3 l p*3 i f*3 p)
# include/lara_meshtopo.h
i lara_meshtopo_halfedge_keys(i i p*3 s)
i lara_meshtopo_edge_heads(l p p s)
i lara_meshtopo_edge_rows(l l p*10 s)
i lara_meshtopo_report(i i l p*6 s)
i lara_meshtopo_boundary_vertices(i l p*3 s)
i lara_meshtopo_pair_keys(l p p s)
i lara_meshtopo_corner_keys(i i p p s)
i lara_meshtopo_csr(i l p i p p s)
i lara_meshtopo_vertex_normals(i p*4 i p p s)
i lara_meshtopo_smooth_pass(i p*4 d p s)
i lara_meshtopo_normals_host(i p*4 i p p)
i lara_meshtopo_smooth_host(i p*4 d p)
# include/lara_meshwind.h
l lara_meshwind_moments_bytes(i)
i lara_meshwind_moments(i p p s)
i lara_meshwind_rows(i p*3 d p*3 s)
i lara_meshwind_classify(i p d d p*4 s)
i lara_meshwind_solid_host(l p*3)
i lara_meshwind_brute_host(i p l p p)
# include/lara_pointfeat.h
l lara_point_feats_workspace_bytes(i*3)
i lara_point_feats_forward(i*4 p*9 s)
i lara_point_feats_backward(i*4 p*13 s)
i lara_point_feats_forward_concat(i*5 p*9 s)
i lara_point_feats_backward_concat(i*5 p*13 s)
i lara_take_rows(i p i RowsItem i s)
i lara_voxel_rows(i i p*3 i s)
# include/lara_rays.h
i lara_build_rays_out(i*3 f p*3 s)
# include/lara_splatadam.h
i lara_splatadam_step(p i l p*20 p i p s)
i lara_splatadam_step_host(p i l p*20 p i p)
# include/lara_splatdensify.h
i lara_splatdensify_accumulate(l i p*5 s)
i lara_splatdensify_accumulate_host(l i p*5)
l lara_splatdensify_workspace_bytes(l)
i lara_splatdensify_decide(p l p*9 s)
i lara_splatdensify_decide_host(p l p*9)
i lara_splatdensify_apply(p i l*3 p*7 s)
i lara_splatdensify_apply_host(p i l*3 p*7)
# include/lara_splatxform.h
i lara_splatxform_apply(p i l p*10 l l s)
i lara_splatxform_apply_host(p i l p*10 l l)
# include/lara_surface.h
i lara_surface_maps_forward(i i p*4 f p*6 s)
i lara_surface_maps_backward(i i p*4 f p*8 s)
i lara_activate_gaussians_forward(l p*6 s)
i lara_activate_gaussians_backward(l p*9 s)
i lara_surface_maps_forward_views(i*3 p*4 f p*6 s)
i lara_surface_maps_backward_views(i*3 p*4 f p*8 s)
# include/lara_tsdf.h
i lara_tsdf_integrate(i p f f i*3 p*8 s)
i lara_tsdf_integrate_blocks(i p f f i*4 p*11 s)
i lara_tsdf_mesh_count(i p f p*5 s)
i lara_tsdf_mesh_emit(i p f p*9 s)
# include/lara_vit.h
l lara_vit_workspace_bytes(VitDims i)
l lara_vit_save_bytes(VitDims)
i lara_vit_save_offsets(VitDims p i)
i lara_vit_forward(VitDims p*5 s)
i lara_vit_backward(VitDims p*5 s)
"""

_RETURNS = {"i": ctypes.c_int, "l": _i64, "z": ctypes.c_char_p}
_PARAMS = {"i": _i32, "l": _i64, "f": _f32, "d": ctypes.c_double, "p": _vp, "s": _vp,
           **{cls.__name__: ctypes.POINTER(cls) for cls in STRUCTS.values()}}


def _parse_signatures(text):
    """{name: (restype, [argtypes], ends in the stream?)}; a row that does not parse is an error here, at import."""
    table = {}
    for row in text.splitlines():
        row = row.strip()
        if not row or row.startswith("#"):
            continue
        m = re.fullmatch(r"(\w) (\w+)\(([^()]*)\)", row)
        if m is None or m.group(1) not in _RETURNS or m.group(2) in table:
            raise ValueError(f"lara_amd: bad or repeated signature row {row!r}")
        kinds = []
        for token in m.group(3).split():
            t = re.fullmatch(r"(\w+)(?:\*(\d+))?", token)
            if t is None or t.group(1) not in _PARAMS:
                raise ValueError(f"lara_amd: unknown parameter {token!r} in {row!r}")
            kinds += [t.group(1)] * int(t.group(2) or 1)
        if "s" in kinds[:-1]:
            raise ValueError(f"lara_amd: the stream is the last parameter, in {row!r}")
        table[m.group(2)] = (_RETURNS[m.group(1)], [_PARAMS[k] for k in kinds], kinds[-1:] == ["s"])
    return table


_SIGS = _parse_signatures(SIGNATURES)
_handle = None          # the loaded library ...
_handle_path = None     # ... and the path it was loaded from


def load_library(path=None):
    """Load liblara2dgs.so (built by ``__graft_entry__.build()`` / ``make -C lara_amd/csrc``), once, with every signature of
    ``SIGNATURES`` applied.  ``path``: ``rasterizer.load_library`` passes its own ``LIB_PATH``, which callers may have pointed
    elsewhere; the cached handle answers only for the path it was loaded from."""
    global _handle, _handle_path
    if _handle is not None and path in (None, _handle_path):
        return _handle
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"lara_amd: HIP library not found at {path}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C lara_amd/csrc`. "
            "There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes, _) in _SIGS.items():
        fn = getattr(lib, name)         # (a row without a symbol behind it fails here, not at the first call)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.lara2dgs_abi_version() != ABI_VERSION:
        raise RuntimeError("lara_amd: liblara2dgs.so ABI version mismatch; rebuild the library")
    _handle, _handle_path = lib, path
    return lib


def check(rc: int, what: str):
    if rc != 0:
        lib = load_library()
        raise RuntimeError(f"lara_amd: {what} failed: {lib.lara2dgs_error_string(rc).decode()} "
                           f"(hipError {lib.lara2dgs_last_hip_error()})")


def current_stream(device):
    """The hipStream_t of ``device``'s current torch stream, as the integer the library takes."""
    return torch.cuda.current_stream(device).cuda_stream


def call(name: str, device, *args):
    """``name(*args[, stream])`` on ``device`` (None: a host-only function), checked.  A tensor goes as its ``data_ptr()``,
    None as NULL; ints (raw addresses among them), floats, struct instances and host arrays go as they are; the device's
    current stream is appended where the prototype ends in ``void *stream``.  Nothing is copied, cast or made contiguous."""
    lib = load_library()
    _, argtypes, has_stream = _SIGS[name]
    with torch.cuda.device(device) if device is not None else contextlib.nullcontext():
        a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
        if has_stream:
            a.append(current_stream(device))
        if len(a) != len(argtypes):      # (ctypes lets extra arguments of a cdecl function through)
            raise TypeError(f"lara_amd: {name} takes {len(argtypes)} arguments, got {len(a)}")
        rc = getattr(lib, name)(*a)
    if rc != 0:
        check(rc, name)


def call_on(name: str, device, *args):
    """``call`` of the entry ``name`` for tensors on the GPU ``device``, of its host twin ``<name>_host`` (the same function
    compiled for the CPU, no stream) for tensors on the host."""
    if device.type == "cuda":
        call(name, device, *args)
    else:
        call(name + "_host", None, *args)


def query(name: str, *args, error=None) -> int:
    """A ``*_bytes`` / ``*_floats`` / ``*_blocks`` / ``*_rows`` query (host code).  A negative answer raises like a failed
    call, or raises ``error`` where the caller has a better message for sizes the library refuses."""
    if len(args) != len(_SIGS[name][1]):
        raise TypeError(f"lara_amd: {name} takes {len(_SIGS[name][1])} arguments, got {len(args)}")
    n = int(getattr(load_library(), name)(*args))
    if n < 0:
        if error is not None:
            raise error
        check(n, name)
    return n


def pointers(*tensors):
    """The addresses of ``tensors`` (None: NULL), for a direct call of a function of the loaded library."""
    return [None if t is None else t.data_ptr() for t in tensors]


def require_device(t):
    """The one "no CPU path" check: ``t`` is a tensor or a ``torch.device``."""
    if not (t.is_cuda if isinstance(t, torch.Tensor) else t.type == "cuda"):
        raise RuntimeError("lara_amd: tensors must live on an MI355X (HIP) device; there is no CPU path")


def rows3(x, device, what: str, module: str) -> torch.Tensor:
    """``x`` as the [N,3] fp32 contiguous tensor on ``device`` a kernel takes (detached); any other shape raises."""
    x = x.detach().to(device, torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f"lara_amd.{module}: expected {what} [N,3]")
    return x


def host_array(kind: str, values):
    """A host array a 'p' parameter takes: ``kind`` 'i' int32, 'l' int64, 'f' float, 'd' double, 'p' device addresses (of
    tensors); ``values`` the elements, or a length for a zeroed output array."""
    ctype = {"i": _i32, "l": _i64, "f": _f32, "d": ctypes.c_double, "p": _vp}[kind]
    if isinstance(values, int):
        return (ctype * values)()
    if kind == "p":
        values = [t.data_ptr() for t in values]
    return (ctype * len(values))(*values)


def char_buffer(nbytes: int):
    return ctypes.create_string_buffer(nbytes)


# ---- byte buffers -----------------------------------------------------------------------------------------------------------
_GUARD = 1 << 16   # poison mode: guard bytes on either side of a buffer
_guards = []       # poison mode: [(whole allocation, payload bytes)] handed out since the last check_poison_guards()


def _poison_mode() -> bool:
    return os.environ.get("LARA2DGS_POISON_BUFFERS") == "1"


def alloc_bytes(n: int, device: torch.device) -> torch.Tensor:
    """A state / scratch / workspace buffer.  LARA2DGS_POISON_BUFFERS=1 (tests / debugging): the buffer sits between two 64 KB
    guard zones and everything is filled with 0xFF bytes (NaN as floats, 4 G as counts) before the library sees it -- a kernel
    that reads a field before it is written, or beyond either end, then fails loudly instead of living off whatever the caching
    allocator left around, and `check_poison_guards()` finds a write beyond either end."""
    if not _poison_mode():
        return torch.empty(n, dtype=torch.uint8, device=device)
    whole = torch.empty(n + 2 * _GUARD, dtype=torch.uint8, device=device)
    whole.fill_(255)
    _guards.append((whole, n))
    return whole[_GUARD:_GUARD + n]


class StreamWorkspace:
    """One module's workspace: a byte tensor per (device index, current stream), grown on demand.  Two calls on one stream
    share it in stream order; a module whose call runs another module's call while it holds its own keeps an instance of its own."""

    def __init__(self):
        self._buffers = {}

    def __call__(self, dev, nbytes):
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        ws = self._buffers.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._buffers[key] = alloc_bytes(nbytes, dev)
        return ws


def check_poison_guards() -> list:
    """Poison mode: the payload sizes of the buffers handed out since the last call whose guard zones no longer read 0xFF
    (i.e. some kernel wrote outside the buffer); synchronises the device."""
    torch.cuda.synchronize()
    bad = [n for whole, n in _guards
           if not bool((whole[:_GUARD] == 255).all()) or not bool((whole[_GUARD + n:] == 255).all())]
    _guards.clear()
    return bad
