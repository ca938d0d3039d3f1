"""The image half of `lara_amd.dataset` without a GPU: `finish_images` through ``lara_batch_finish_host`` (the per-pixel function of
csrc/batchfinish_ops.h compiled for the CPU) held to the numpy float32 restatement (tests/batchfinish_restate.py) word for word --
every (colour, alpha) pair under six backgrounds, every normal code under 16 matrices -- and to the REFERENCE class's own items
(tests/golden/loader_ref.npz): colour and mask as integers, normals within the bound two orders of a 3-term fp32 sum allow.
`raw_views`: the class's items under it (tests/golden/loader_raw_ref.npz, tests/golden/make_loader_raw_fixture.py) against its items
without it, the hook's mechanics on a stand-in class, a DataLoader with two workers.  The refusals, the binding, the stand-alone
sanitizer program."""
import os
import pickle
import random
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from lara_amd import dataset as D
from tests import batchfinish_restate as S
from tests.helpers_store import make_store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "loader_ref.npz")
FX_RAW = os.path.join(ROOT, "tests", "golden", "loader_raw_ref.npz")
TAGS = ("train4", "test4", "test1")
IMAGE_KEYS = ("tar_rgb", "tar_msk", "tar_nrm", "tar_nrm_u8")


def _t(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _same_words(got, want, what=""):
    got, want = S.words(got.numpy() if torch.is_tensor(got) else got), S.words(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def fixture_items(fx, tag):
    """{index: item} of one configuration of a loader fixture."""
    n = int(fx[f"{tag}.len"])
    items = {}
    for index in (0, n - 1):
        pre = f"{tag}.{index}."
        it = {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}
        scene, view = str(it.pop("scene")), it.pop("tar_view").tolist()
        it["meta"] = {"scene": scene, "tar_view": view, "frame_id": 0, "tar_h": 32, "tar_w": 32}
        it["fovx"], it["fovy"] = it["fovx"][()], it["fovy"][()]
        items[index] = it
    return items


# ------------------------------------------------------------------------------------------------------------------ the arithmetic

BACKGROUNDS = (0.0, 0.5, 1.0, 0.2, 250.0, -0.0)


def test_every_colour_and_alpha_composites_to_the_restated_words(hip_lib):
    """All 256 x 256 (c, a): channel 0 carries c against a, channels 1 and 2 the same pairs in two other arrangements; each of the six
    backgrounds is the colour of one view, and a seventh view has three different channels."""
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    plane = np.stack([c, c[::-1], (c.astype(np.int64) * 7 + 3).astype(np.uint8), a], axis=-1)
    V = len(BACKGROUNDS) + 1
    rgba = np.broadcast_to(plane, (1, V, 256, 256, 4)).copy()
    bg = np.array([[b, b, b] for b in BACKGROUNDS] + [[0.25, 3.0, -1.5]], np.float32)[None]
    assert np.signbit(bg[0, 5]).all()
    rgb, msk, nrm = D.finish_images(*_t(rgba, bg))
    want_rgb, want_msk = S.colour(rgba, bg)
    assert nrm is None and rgb.dtype == torch.float32 and msk.dtype == torch.uint8
    _same_words(rgb, want_rgb, "rgb")
    _same_words(msk, want_msk, "msk")
    assert set(np.unique(want_msk)) == {0, 1} and (want_msk == (a > 0)).all()
    # the restatement's own footing: opaque pixels are c / 255 whatever the background, clear ones the background's words
    assert np.array_equal(want_rgb[0, 4, :, 255, 0], np.arange(256, dtype=np.float32) / np.float32(255))
    assert np.array_equal(want_rgb[0, 3, :, 0, 1].view(np.uint32), np.full(256, np.float32(0.2).view(np.uint32)))


def _seeded_matrices(n=16):
    g = np.random.default_rng(23)
    return np.concatenate([g.normal(size=(n - 2, 3, 3)), g.normal(size=(1, 3, 3)) * 1e4, g.normal(size=(1, 3, 3)) * 1e-4]).astype(np.float32)


def test_every_normal_code_rotates_to_the_restated_words(hip_lib):
    """16 scenes, each with its own seeded 3x3 (no rotations: any finite matrix), 3 views of 16 x 16: channel 0 walks all 256 codes,
    channels 1 and 2 are seeded, so every code meets every column of every matrix."""
    R = _seeded_matrices()
    g = np.random.default_rng(29)
    B, V, H, W = len(R), 3, 16, 16
    n_u8 = g.integers(0, 256, (B, V, H, W, 3), dtype=np.uint8)
    codes = np.arange(256, dtype=np.uint8).reshape(H, W)
    n_u8[:, 0, :, :, 0], n_u8[:, 1, :, :, 1], n_u8[:, 2, :, :, 2] = codes, codes.T, codes[::-1]
    rgba = g.integers(0, 256, (B, V, H, W, 4), dtype=np.uint8)
    bg = g.random((B, V, 3)).astype(np.float32)
    rgb, msk, nrm = D.finish_images(*_t(rgba, bg, n_u8, R))
    assert nrm.shape == (B, H, V * W, 3)
    _same_words(nrm, S.normals(n_u8, R), "nrm")
    _same_words(rgb, S.colour(rgba, bg)[0], "rgb beside normals")
    _same_words(msk, S.colour(rgba, bg)[1], "msk beside normals")


def test_the_identity_leaves_the_decoded_normals(hip_lib):
    g = np.random.default_rng(31)
    B, V, H, W = 2, 3, 16, 16
    n_u8 = g.integers(0, 256, (B, V, H, W, 3), dtype=np.uint8)
    n_u8[0, 0, :, :, 0] = np.arange(256, dtype=np.uint8).reshape(H, W)
    rgba = np.zeros((B, V, H, W, 4), np.uint8)
    R = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3)).copy()
    nrm = D.finish_images(*_t(rgba, np.ones((B, V, 3), np.float32), n_u8, R))[2].numpy()
    decoded = n_u8.astype(np.float32) / np.float32(255.0) * np.float32(2) - np.float32(1.0)       # gobjverse.py:138, as written there
    assert np.array_equal(nrm, decoded.transpose(0, 2, 1, 3, 4).reshape(B, H, V * W, 3))
    assert np.array_equal(nrm.reshape(B, H, V, W, 3)[1, 5, 2, 7], decoded[1, 2, 5, 7])             # pixel (b, v, h, w) lies at [b, h, v W + w]


# ------------------------------------------------------------------------------------------------------------------ the reference's items

def test_the_stored_arrays_finish_to_the_reference_items(hip_lib):
    """All six fixture items: the raw arrays of the store at the item's own views, its own bg_color and transform_mats -> the
    class's tar_rgb and tar_msk as integers, its tar_nrm within 8 u sum_k |n_k R[j][k]| (numpy's matmul sums in its own order)."""
    fx, store = np.load(FX), make_store(seed=5)
    worst = 0.0
    for tag in TAGS:
        for index, it in fixture_items(fx, tag).items():
            scene = store[it["meta"]["scene"]]
            rgba = np.stack([scene[f"image_{v}"] for v in it["meta"]["tar_view"]])[None]
            n_u8 = np.stack([scene[f"normal_{v}"] for v in it["meta"]["tar_view"]])[None]
            rot = it["transform_mats"][0, :3, :3][None]
            rgb, msk, nrm = D.finish_images(*_t(rgba, it["bg_color"][None], n_u8, rot))
            _same_words(rgb[0], it["tar_rgb"], f"{tag}.{index} tar_rgb")
            _same_words(msk[0], it["tar_msk"], f"{tag}.{index} tar_msk")
            assert nrm[0].shape == it["tar_nrm"].shape == (32, len(it["meta"]["tar_view"]) * 32, 3)
            bound = S.normal_bound(n_u8, rot)[0]
            assert (bound > 0).all()
            ratio = float((np.abs(nrm[0].numpy().astype(np.float64) - it["tar_nrm"].astype(np.float64)) / bound).max())
            print(f"{tag}.{index}: max |tar_nrm - reference| / bound = {ratio:.3f}")
            worst = max(worst, ratio)
    print(f"worst ratio over the six items: {worst:.3f} (measured at writing: 0.42)")
    assert worst <= 1.0


def test_raw_views_items_are_the_reference_items_with_the_stored_images():
    """loader_raw_ref.npz: the reference class under `raw_views`, same store, seeds and configurations as loader_ref.npz."""
    fx, raw, store = np.load(FX), np.load(FX_RAW), make_store(seed=5)
    for tag in TAGS:
        assert int(raw[f"{tag}.len"]) == int(fx[f"{tag}.len"])
        for (index, it), ref in zip(fixture_items(raw, tag).items(), fixture_items(fx, tag).values()):
            assert set(it) | set(D.RAY_KEYS) | {"tar_nrm"} == set(ref) | {"tar_nrm_u8"}, tag
            assert it["meta"] == ref["meta"]
            for k, v in ref.items():
                if k in IMAGE_KEYS or k in D.RAY_KEYS or k == "meta":
                    continue
                assert it[k].dtype == np.asarray(v).dtype, k
                np.testing.assert_array_equal(np.asarray(it[k]), v, err_msg=f"{tag}.{index}.{k}")
            scene, views = store[ref["meta"]["scene"]], ref["meta"]["tar_view"]
            assert it["tar_rgb"].dtype == np.uint8 and it["tar_rgb"].shape == (len(views), 32, 32, 4)
            assert np.array_equal(it["tar_rgb"], np.stack([scene[f"image_{v}"] for v in views]))
            assert it["tar_nrm_u8"].dtype == np.uint8 and np.array_equal(it["tar_nrm_u8"], np.stack([scene[f"normal_{v}"] for v in views]))
            assert it["tar_msk"].dtype == np.uint8 and it["tar_msk"].size == 0 and "tar_nrm" not in it


# ------------------------------------------------------------------------------------------------------------------ the hook

class StandIn(torch.utils.data.Dataset):
    """The parts of the reference class the hook rests on, and no more: ``cfg.load_normal`` read in ``__getitem__``, ``read_image``
    called as a method with (scene, view, bg_color, scene name), the views stacked, ``metas`` indexed by scene name."""

    def __init__(self, cfg, store):
        self.cfg, self.metas, self.names = cfg, store, sorted(store.keys())

    def __len__(self):
        return len(self.names)

    def read_image(self, scene, view_idx, bg_color, scene_name):
        img = np.array(scene[f"image_{view_idx}"]).astype(np.float32)
        return img[..., :3], (np.array(scene[f"normal_{view_idx}"]).astype(np.float32) if self.cfg.load_normal else None), img[..., 3]

    def __getitem__(self, index):
        name = self.names[index]
        views = [random.randrange(10) for _ in range(3)]
        parts = [self.read_image(self.metas[name], v, np.ones(3, np.float32), name) for v in views]
        ret = {"tar_rgb": np.stack([p[0] for p in parts]), "tar_msk": np.stack([p[2] for p in parts]), "drawn": np.float32(random.random()),
               "transform_mats": np.eye(4, dtype=np.float32)[None], "meta": {"scene": name, "tar_view": views, "data_root": self.cfg.data_root}}
        if self.cfg.load_normal:
            ret["tar_nrm"] = np.stack([p[1] for p in parts]).reshape(32, -1, 3)
        return ret


@pytest.mark.parametrize("load_normal", (True, False))
def test_the_hook_leaves_the_cfg_alone_and_the_wrapper_pickles(load_normal):
    store = make_store(seed=3, n_scenes=3)
    cfg = types.SimpleNamespace(data_root="mem", load_normal=load_normal, extra=[1, 2])
    before = dict(vars(cfg))
    other = StandIn(cfg, store)
    ds = D.raw_views(StandIn(cfg, store))
    assert vars(cfg) == before and cfg.load_normal is load_normal                  # the caller's object is as it was
    assert ds.ds.cfg.load_normal is False and ds.ds.cfg.data_root == "mem" and ds.ds.cfg.extra is cfg.extra
    with pytest.raises(AttributeError):
        ds.ds.cfg.missing
    assert len(ds) == 3 and "read_image" not in vars(other) and StandIn.read_image is type(ds.ds).read_image
    random.seed(7)
    plain = other[1]
    random.seed(7)
    it = ds[1]
    assert it["meta"] == plain["meta"] and it["drawn"] == plain["drawn"]           # same draws, and the forwarded cfg was read
    views = it["meta"]["tar_view"]
    assert it["tar_rgb"].dtype == np.uint8 and np.array_equal(it["tar_rgb"], np.stack([store[it["meta"]["scene"]][f"image_{v}"] for v in views]))
    assert it["tar_msk"].dtype == np.uint8 and it["tar_msk"].size == 0 and "tar_nrm" not in it
    if load_normal:
        assert np.array_equal(it["tar_nrm_u8"], np.stack([store[it["meta"]["scene"]][f"normal_{v}"] for v in views]))
    else:
        assert "tar_nrm_u8" not in it
    again = pickle.loads(pickle.dumps(ds))
    random.seed(7)
    back = again[1]
    assert back["meta"] == it["meta"] and np.array_equal(back["tar_rgb"], it["tar_rgb"]) and again.ds.cfg.load_normal is False
    assert D.raw_views(ds.ds).load_normal is load_normal                           # taken over twice: the cfg view does not nest
    assert vars(cfg) == before


def test_raw_items_go_through_dataloader_workers_and_collate_cpu():
    """A real DataLoader with two worker processes over `raw_views` of the stand-in class: the uint8 arrays are default-collated as
    they are, the ray keys are dropped."""
    store = make_store(seed=3, n_scenes=4)
    cfg = types.SimpleNamespace(data_root="mem", load_normal=True)

    ds = D.raw_views(StandIn(cfg, store))
    loader = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=2, collate_fn=D.collate_cpu)
    batches = list(loader)
    assert len(batches) == 2
    for i, b in enumerate(batches):
        assert b["tar_rgb"].dtype == torch.uint8 and b["tar_rgb"].shape == (2, 3, 32, 32, 4) and not b["tar_rgb"].is_cuda
        assert b["tar_nrm_u8"].dtype == torch.uint8 and b["tar_nrm_u8"].shape == (2, 3, 32, 32, 3)
        assert b["tar_msk"].dtype == torch.uint8 and b["tar_msk"].shape == (2, 3, 0) and "tar_nrm" not in b
        for j in range(2):
            scene = store[b["meta"]["scene"][j]]
            views = [int(v[j]) for v in b["meta"]["tar_view"]]
            assert np.array_equal(b["tar_rgb"][j].numpy(), np.stack([scene[f"image_{v}"] for v in views]))
            assert np.array_equal(b["tar_nrm_u8"][j].numpy(), np.stack([scene[f"normal_{v}"] for v in views]))


def test_collate_cpu_of_fixture_items_raw_and_float():
    """Raw fixture items collate with their uint8 arrays; the float items collate to what they did (the ray keys dropped)."""
    fx, raw = np.load(FX), np.load(FX_RAW)
    items, refs = list(fixture_items(raw, "test4").values()), list(fixture_items(fx, "test4").values())
    a, b = D.collate_cpu(items), D.collate_cpu(refs)
    assert a["tar_rgb"].dtype == torch.uint8 and a["tar_rgb"].shape == (2, 8, 32, 32, 4) and a["tar_nrm_u8"].shape == (2, 8, 32, 32, 3)
    assert set(a) - {"tar_nrm_u8"} == set(b) - {"tar_nrm"} and not set(a) & set(D.RAY_KEYS)
    want = torch.utils.data.default_collate([{k: v for k, v in it.items() if k not in D.RAY_KEYS} for it in refs])
    assert set(b) == set(want) and all(torch.equal(b[k], want[k]) for k in b if torch.is_tensor(b[k]))
    for k in ("tar_c2w", "tar_w2c", "tar_ixt", "transform_mats", "bg_color", "near_far", "fovx", "fovy"):
        assert torch.equal(a[k], b[k]), k


def test_finish_on_device_finishes_raw_batches_on_the_host_too(hip_lib, monkeypatch):
    """`finish_on_device` with device="cpu" (the host entry; the ray kernel is stood in for: it has no host form): a raw batch comes
    out with the float batch's image tensors, the float batch as it went in."""
    from lara_amd import batch as batch_mod
    monkeypatch.setattr(batch_mod, "build_rays", lambda c2w, ixt, H, W, scale: torch.zeros(c2w.shape[0], max(int(H * scale), 1), max(int(W * scale), 1), 6))
    fx, raw = np.load(FX), np.load(FX_RAW)
    for tag in TAGS:
        items, refs = list(fixture_items(raw, tag).values()), list(fixture_items(fx, tag).values())
        got, want = D.finish_on_device(D.collate_cpu(items), "cpu"), D.finish_on_device(D.collate_cpu(refs), "cpu")
        assert set(got) == set(want), tag
        assert torch.equal(got["tar_rgb"], want["tar_rgb"]) and torch.equal(got["tar_msk"], want["tar_msk"]), tag
        assert got["tar_nrm"].shape == want["tar_nrm"].shape and got["tar_nrm"].dtype == torch.float32
        n_u8 = np.stack([it["tar_nrm_u8"] for it in items])
        rot = np.stack([it["transform_mats"][0, :3, :3] for it in items])
        assert (np.abs(got["tar_nrm"].numpy().astype(np.float64) - want["tar_nrm"].numpy().astype(np.float64)) <= S.normal_bound(n_u8, rot)).all()
        plain = D.collate_cpu(refs)
        assert all(torch.equal(want[k], plain[k]) for k in plain if torch.is_tensor(plain[k])), tag      # float batches: untouched


# ------------------------------------------------------------------------------------------------------------------ refusals, binding

def test_finish_images_refuses_by_the_arguments_name(hip_lib):
    B, V, H, W = 2, 3, 4, 4
    rgba = torch.zeros(B, V, H, W, 4, dtype=torch.uint8)
    bg = torch.ones(B, V, 3)
    n_u8 = torch.zeros(B, V, H, W, 3, dtype=torch.uint8)
    rot = torch.eye(3).repeat(B, 1, 1)
    D.finish_images(rgba, bg, n_u8, rot)
    bad = [
        ("rgba", dict(rgba=rgba.float())), ("rgba", dict(rgba=rgba[..., :3].contiguous())), ("rgba", dict(rgba=rgba[0])),
        ("rgba", dict(rgba=rgba.numpy())), ("rgba", dict(rgba=torch.zeros(B, V, H, 2 * W, 4, dtype=torch.uint8)[:, :, :, ::2])),
        ("bg_color", dict(bg_color=bg.double())), ("bg_color", dict(bg_color=bg[:, :2].contiguous())), ("bg_color", dict(bg_color=bg[0])),
        ("bg_color", dict(bg_color=torch.ones(B, 3, V).transpose(1, 2))),
        ("normals_u8", dict(normals_u8=n_u8.float())), ("normals_u8", dict(normals_u8=n_u8[:, :, :, :2].contiguous())),
        ("normals_u8", dict(normals_u8=torch.zeros(B, V, W, H, 3, dtype=torch.uint8).transpose(2, 3))),
        ("normals_u8", dict(normals_u8=None)), ("rot", dict(rot=None)),
        ("rot", dict(rot=rot.double())), ("rot", dict(rot=torch.eye(4).repeat(B, 1, 1))), ("rot", dict(rot=rot[:1])),
        ("rot", dict(rot=torch.eye(4).repeat(B, 1, 1)[:, :3, :3])),
    ]
    for name, change in bad:
        kw = dict(rgba=rgba, bg_color=bg, normals_u8=n_u8, rot=rot)
        kw.update(change)
        with pytest.raises(ValueError, match=rf"lara_amd\.dataset: {name} "):
            D.finish_images(**kw)
    for name in ("bg_color", "normals_u8", "rot"):                                 # mixed devices (no device is touched: a meta tensor)
        kw = dict(rgba=rgba, bg_color=bg, normals_u8=n_u8, rot=rot)
        kw[name] = kw[name].to("meta")
        with pytest.raises(ValueError, match=rf"lara_amd\.dataset: {name} lies on meta"):
            D.finish_images(**kw)
    # a contiguous view at a storage offset is no refusal
    shifted = torch.zeros(rgba.numel() + 1, dtype=torch.uint8)[1:].view(rgba.shape)
    assert torch.equal(D.finish_images(shifted, bg)[0], D.finish_images(rgba, bg)[0])


def test_an_empty_batch_launches_nothing(hip_lib, monkeypatch):
    for through in ("call_on", "call"):
        monkeypatch.setattr(D._native, through, lambda name, *a: pytest.fail(f"{name} was called for an empty batch"))
    for shape in ((0, 8, 4, 4), (2, 0, 4, 4), (2, 8, 0, 4), (2, 8, 4, 0)):
        B, V, H, W = shape
        rgb, msk, nrm = D.finish_images(torch.zeros(*shape, 4, dtype=torch.uint8), torch.ones(B, V, 3),
                                        torch.zeros(*shape, 3, dtype=torch.uint8), torch.eye(3).repeat(B, 1, 1))
        assert rgb.shape == (*shape, 3) and msk.shape == shape and nrm.shape == (B, H, V * W, 3)


def test_the_entry_points_refuse_bad_arguments(hip_lib):
    B, V, H, W = 1, 2, 2, 2
    bufs = [np.zeros((B, V, H, W, 4), np.uint8), np.ones((B, V, 3), np.float32), np.zeros((B, V, H, W, 3), np.uint8),
            np.eye(3, dtype=np.float32)[None].copy(), np.zeros((B, V, H, W, 3), np.float32), np.zeros((B, V, H, W), np.uint8),
            np.zeros((B, H, V * W, 3), np.float32)]
    p = [b.ctypes.data for b in bufs]
    host, dev = hip_lib.lara_batch_finish_host, hip_lib.lara_batch_finish
    assert host(*p[:4], B, V, H, W, *p[4:]) == 0
    assert host(p[0], p[1], None, None, B, V, H, W, p[4], p[5], None) == 0             # the rgb-only form
    for fn, tail in ((host, ()), (dev, (None,))):          # (the device entry refuses before it touches a device)
        for k in (0, 1, 4, 5):
            q = list(p)
            q[k] = None
            assert fn(*q[:4], B, V, H, W, *q[4:], *tail) == -1, k
        for gone in ((2,), (3,), (6,), (2, 3), (2, 6), (3, 6)):
            q = [None if k in gone else v for k, v in enumerate(p)]
            assert fn(*q[:4], B, V, H, W, *q[4:], *tail) == -1, gone
        for dims in ((-1, V, H, W), (B, -1, H, W), (B, V, -1, W), (B, V, H, -1), (2 ** 31, 1, 1, 1), (2 ** 16, 2 ** 15, 1, 1),
                     (2 ** 40, 2 ** 40, 1, 1), (1, 2 ** 11, 2 ** 10, 2 ** 10)):
            assert fn(*p[:4], *dims, *p[4:], *tail) == -1, dims
        for dims in ((0, V, H, W), (B, V, H, 0)):
            assert fn(*[None] * 4, *dims, *[None] * 3, *tail) == 0                     # empty: nothing to do, no pointer looked at
    with pytest.raises(ValueError, match="lara_amd.dataset: rgba holds"):
        D._finish_into(torch.zeros(1, dtype=torch.uint8).expand(2 ** 16, 2 ** 15, 1, 1, 4), None, None, None, None, None, None)


def test_the_modules_binding_equals_the_headers_prototypes(hip_lib):
    """The header lies under include/ and its two functions are rows of ``_native.SIGNATURES`` (tests/test_abi_cpu.py holds the rows
    to the prototypes, kind by kind): the library exports both, the stream is on the device entry alone, the unit is built with
    -ffp-contract=off."""
    from lara_amd import _native
    from tests.test_abi_cpu import header_functions_by_file
    names = ["lara_batch_finish", "lara_batch_finish_host"]
    assert sorted(header_functions_by_file()["lara_batchfinish.h"]) == names
    assert set(names) <= set(_native._SIGS) and all(hasattr(hip_lib, n) for n in names)
    assert [_native._SIGS[n][2] for n in names] == [True, False]                                  # the stream, on the device entry alone
    text = open(os.path.join(ROOT, "lara_amd", "csrc", "Makefile")).read()
    assert "FLAGS_batchfinish := -ffp-contract=off\n" in text and " batchfinish " in text.split("OBJS")[1].splitlines()[0]


# ------------------------------------------------------------------------------------------------------------------ the hostcheck

def test_the_stand_alone_host_program_ends_without_a_report():
    """csrc/batchfinish_ops.h and the host entry's loop as a stand-alone program under AddressSanitizer and UBSan (nothing loaded
    into python, no device): 0 words off the restatement, exit code 0, no report."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "batchfinish_hostcheck.py")], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "words off the restatement 0" in run.stdout and "sanitizer reports: none" in run.stdout, run.stdout
