"""`lara_amd.dataset.finish_images` on the GPU (csrc/batchfinish.hip): the kernel's words equal the host entry's words -- the same
per-pixel function compiled for the CPU, which tests/test_batchfinish.py holds to the numpy restatement and to the reference's items
-- on every shape of tests/batchfinish_cases.py (single pixels, short quads, odd rows, either side of one workgroup's span, shapes
that send one half the wide way and the other pixel by pixel), with inputs and outputs at storage offsets that force the per-pixel
path, in the rgb-only form, into sentinel-filled outputs with guard rows; a batch whose word indices pass 2^31; then raw fixture
batches through `on_device` against `collate_to_device` of the reference's float items."""
import functools

import numpy as np
import pytest
import torch

from lara_amd import dataset as D
from tests import batchfinish_cases as C
from tests import batchfinish_restate as S
from tests.test_batchfinish import FX, FX_RAW, TAGS, fixture_items

pytestmark = pytest.mark.gpu
GUARD = 64                                   # elements of sentinel after every output
SENTINEL_F, SENTINEL_B = -12345.0, 0xEE


@functools.lru_cache(maxsize=None)
def _case(i):
    """(the batch, the host entry's outputs) of shape i, computed once."""
    b = C.batch(C.SHAPES[i], seed=i)
    host = D.finish_images(*(torch.from_numpy(b[k]) for k in ("rgba", "bg", "n_u8", "rot")))
    return b, host


def _at_offset(a, nbytes, device):
    """``a`` on the device as a contiguous view that starts ``nbytes`` into its allocation."""
    t = torch.from_numpy(a)
    raw = torch.empty(t.numel() * t.element_size() + nbytes, dtype=torch.uint8, device=device)
    assert raw.data_ptr() % 256 == 0
    view = raw[nbytes:].view(t.dtype).view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == nbytes % 16
    return view


def _output(shape, dtype, nbytes, device):
    """A sentinel-filled allocation and its view of ``shape`` that starts ``nbytes`` in and has GUARD elements after it."""
    n = int(np.prod(shape))
    size = torch.empty(0, dtype=dtype).element_size()
    assert nbytes % size == 0
    whole = torch.full((nbytes // size + n + GUARD,), SENTINEL_F if dtype == torch.float32 else SENTINEL_B, dtype=dtype, device=device)
    return whole, whole[nbytes // size:nbytes // size + n].view(shape)


def _untouched(whole, nbytes, n):
    lead = nbytes // whole.element_size()
    fill = SENTINEL_F if whole.dtype == torch.float32 else SENTINEL_B
    return bool((whole[:lead] == fill).all()) and bool((whole[lead + n:] == fill).all())


def _run(i, *, normals=True, in_offset=0, out_offset=0, device="cuda"):
    b, host = _case(i)
    B, V, H, W = C.SHAPES[i]
    dev = torch.device(device, 0)
    rgba, bg = _at_offset(b["rgba"], in_offset, dev), torch.from_numpy(b["bg"]).to(dev)
    n_u8 = _at_offset(b["n_u8"], in_offset, dev) if normals else None
    rot = torch.from_numpy(b["rot"]).to(dev) if normals else None
    outs = [_output((B, V, H, W, 3), torch.float32, 4 * out_offset, dev), _output((B, V, H, W), torch.uint8, out_offset, dev),
            _output((B, H, V * W, 3), torch.float32, 4 * out_offset, dev) if normals else (None, None)]
    D._finish_into(rgba, bg, n_u8, rot, *(view for _, view in outs))
    torch.cuda.synchronize()
    what = f"{C.SHAPES[i]} normals={normals} in+{in_offset} out+{out_offset}"
    for (whole, view), want, lead in zip(outs, host, (4 * out_offset, out_offset, 4 * out_offset)):
        if view is None:
            continue
        got = view.cpu()
        g, w = (got.view(torch.int32), want.view(torch.int32)) if got.dtype == torch.float32 else (got, want)
        assert torch.equal(g, w), (what, int((g != w).sum()), torch.nonzero(g != w)[:4].tolist())
        assert _untouched(whole, lead, view.numel()), (what, "a guard word was written")


@pytest.mark.parametrize("i", range(len(C.SHAPES)), ids=["x".join(map(str, s)) for s in C.SHAPES])
def test_the_kernels_words_equal_the_host_entrys(hip_lib, i):
    """Each shape with normals and in the rgb-only form, into sentinel-filled outputs with guard rows after them."""
    _run(i)
    _run(i, normals=False)


@pytest.mark.parametrize("offset", (1, 4, 16))
def test_views_at_storage_offsets_store_the_same_words(hip_lib, offset):
    """Inputs that start 1, 4 and 16 bytes into their allocation (1: both halves pixel by pixel; 4: the colour pixel by pixel, the
    normals wide; 16: both wide again), and outputs that start one element in (every store pixel by pixel), on shapes that would
    otherwise go wide."""
    for i in (4, 5, 6, 8, 11, 15):
        assert (C.SHAPES[i][2] * C.SHAPES[i][3]) % 4 == 0
        _run(i, in_offset=offset)
        _run(i, in_offset=offset, out_offset=1)
        _run(i, normals=False, in_offset=offset, out_offset=3)


def test_finish_images_allocates_its_outputs_on_the_inputs_device(hip_lib):
    # (on the default stream, on purpose: with a torch.cuda.Stream() created here, the unprotected half of
    # tests/test_stream_safety_gpu.py's race, which runs later in the same process, no longer lost its rows in the one run that had it)
    b, host = _case(15)
    args = [torch.from_numpy(b[k]).cuda() for k in ("rgba", "bg", "n_u8", "rot")]
    got = D.finish_images(*args)
    torch.cuda.synchronize()
    for g, w in zip(got, host):
        assert g.is_cuda and g.shape == w.shape and g.dtype == w.dtype
        assert torch.equal(g.cpu().view(torch.uint8), w.view(torch.uint8))
    rgb, msk, nrm = D.finish_images(args[0], args[1])
    assert nrm is None and torch.equal(rgb.cpu().view(torch.int32), host[0].view(torch.int32)) and torch.equal(msk.cpu(), host[1])
    with pytest.raises(ValueError, match="lara_amd.dataset: bg_color lies on cpu"):
        D.finish_images(args[0], torch.from_numpy(b["bg"]))


def test_word_indices_past_2_to_the_31_land_where_they_belong(hip_lib):
    """B V H W = 343 x 8 x 512 x 512 pixels: fewer than 2^31 pixels, more than 2^31 fp32 words in tar_rgb and tar_nrm.  The per-pixel
    function has no memory between pixels, so the first and the last scene are held to the host entry on those two scenes alone; a
    32-bit offset anywhere would put the last scene's words elsewhere."""
    B, V, H, W = 343, 8, 512, 512
    assert B * V * H * W < 2 ** 31 < 3 * (B - 1) * V * H * W
    free, _ = torch.cuda.mem_get_info()
    need = B * V * H * W * (4 + 3 + 12 + 1 + 12)
    if free < need + (2 << 30):
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} free")
    g = torch.Generator(device="cuda").manual_seed(5)
    rgba = torch.randint(0, 256, (B, V, H, W, 4), dtype=torch.uint8, device="cuda", generator=g)
    n_u8 = torch.randint(0, 256, (B, V, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    bg = torch.rand(B, V, 3, device="cuda", generator=g)
    rot = torch.randn(B, 3, 3, device="cuda", generator=g)
    rgb, msk, nrm = D.finish_images(rgba, bg, n_u8, rot)
    torch.cuda.synchronize()
    for b in (0, B - 1):
        want = D.finish_images(rgba[b:b + 1].cpu(), bg[b:b + 1].cpu(), n_u8[b:b + 1].cpu(), rot[b:b + 1].cpu())
        for got, w in zip((rgb, msk, nrm), want):
            assert torch.equal(got[b:b + 1].cpu().view(torch.uint8), w.view(torch.uint8)), b
    del rgba, n_u8, rgb, msk, nrm
    torch.cuda.empty_cache()


def test_raw_batches_through_on_device_equal_the_float_batches(hip_lib):
    """The end-to-end check of test_on_device_finishes_cpu_collated_batches for raw items: the reference class's items under
    `raw_views` (loader_raw_ref.npz), CPU-collated and finished by `on_device`, against `collate_to_device` of its float items
    (loader_ref.npz): tar_rgb and tar_msk equal, tar_nrm within 8 u sum_k |n_k R[j][k]|, the rays and every other tensor equal, the
    same keys."""
    fx, raw = np.load(FX), np.load(FX_RAW)
    for tag in TAGS:
        items, refs = list(fixture_items(raw, tag).values()), list(fixture_items(fx, tag).values())
        got = list(D.on_device([D.collate_cpu(items)], "cuda"))[0]
        want = D.collate_to_device(refs)
        assert set(got) == set(want), tag
        for k in want:
            if k == "tar_nrm" or not torch.is_tensor(want[k]):
                continue
            assert got[k].is_cuda and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (tag, k)
        assert got["meta"]["scene"] == want["meta"]["scene"]
        n_u8 = np.stack([it["tar_nrm_u8"] for it in items])
        rot = np.stack([it["transform_mats"][0, :3, :3] for it in items])
        err = np.abs(got["tar_nrm"].cpu().numpy().astype(np.float64) - want["tar_nrm"].cpu().numpy().astype(np.float64))
        assert got["tar_nrm"].shape == want["tar_nrm"].shape and (err <= S.normal_bound(n_u8, rot)).all(), tag
        again = D.collate_to_device(items)                                         # raw items straight through collate_to_device
        assert all(torch.equal(again[k], got[k]) for k in got if torch.is_tensor(got[k])), tag
