"""The DINO image encoder on the MI355X (lara_amd.dino, include/lara_vit.h) against the restatement (tests/dino_restate.py, pinned
by the transformers fixture) and against itself.

Weights are seeded so that attention is peaked (q / k weights of std sqrt(3 / C): logits of std ~ 3), so a softmax error cannot
hide behind near-uniform rows.  Budget: every output and every parameter gradient is within twice the restatement's own autocast
error (restatement under bf16 autocast vs the restatement in fp32) plus 1e-3 of the largest entry, as in `test_groupatt.py`.
Everything the kernels compute twice -- runs, image strides, the inference and the training forward -- is bitwise."""
import pytest
import torch

from tests.dino_restate import RestatedViT, fixture_grads, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _seed(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            r = torch.randn(p.shape, generator=g)
            if n.endswith("qkv.weight"):
                v = r * (3.0 / p.shape[1]) ** 0.5
            elif n == "patch_embed.proj.weight":
                v = r * 768 ** -0.5
            elif p.dim() == 2 and "blocks" in n:
                v = r * p.shape[1] ** -0.5
            elif "norm" in n and n.endswith("weight"):
                v = 1 + 0.1 * r
            elif n == "pos_embed":
                v = 0.5 * r
            elif n == "cls_token":
                v = r
            else:
                v = 0.1 * r
            p.copy_(v)
    return m


def _models(C, depth, heads, seed=0):
    from lara_amd.dino import DinoViT
    ours = DinoViT(embed_dim=C, depth=depth, num_heads=heads).to(DEV)
    _seed(ours, seed)
    ref = RestatedViT(C, depth, heads, 4 * C).to(DEV)
    ref.load_state_dict(ours.state_dict())
    return ours, ref


def _run(model, images, gout, autocast=False):
    model.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = model(images)
    (out.float() * gout).sum().backward()
    return out.detach().float(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _within_budget(got, bf, f32, what):
    bar = 2 * (bf - f32).abs().max() + 1e-3 * f32.abs().max()
    err = (got - f32).abs().max()
    assert err <= bar, f"{what}: |hip - fp32| {err:.3e} > budget {bar:.3e} (autocast error {(bf - f32).abs().max():.3e})"


def _against_restatement(C, depth, heads, N, H, W, seed=0):
    ours, ref = _models(C, depth, heads, seed)
    g = torch.Generator().manual_seed(seed + 1)
    images = torch.rand(N, 3, H, W, generator=g).to(DEV)
    gout = torch.randn(N, (H // 16) * (W // 16), C, generator=g).to(DEV)
    o, gr = _run(ours, images, gout)
    ob, gb = _run(ref, images, gout, autocast=True)
    of, gf = _run(ref, images, gout)
    _within_budget(o, ob, of, "tokens")
    for n in gf:
        _within_budget(gr[n], gb[n], gf[n], n)
    return ours, images, gout, o, gr


def test_fixture_parity_on_the_device():
    from lara_amd.dino import DinoViT
    f, images, m, gout = load_fixture(DEV)
    C, depth, heads, F_, H, W = (int(v) for v in f["config"])
    ours = DinoViT(embed_dim=C, depth=depth, num_heads=heads, mlp_ratio=F_ / C, img_size=(H, W)).to(DEV)
    ours.load_state_dict(m.state_dict())
    out, grads = _run(ours, images, gout)
    ref = torch.from_numpy(f["out"]).to(DEV)
    assert (out - ref).abs().max() <= 3e-2 * ref.abs().max()
    for n, got, exp in fixture_grads(f, grads):
        err = (got - exp).abs().max() / exp.abs().max()
        assert err <= 5e-2, f"{n}: rel err {err:.2e}"


@pytest.fixture(scope="module")
def full_size():
    """ViT-B/16 on 16 images of 512^2 (LaRa's default: 4 scenes x 4 views), 12 blocks, 1025 tokens."""
    return _against_restatement(768, 12, 12, 16, 512, 512)


def test_full_size_against_the_restatement(full_size):
    assert full_size[3].shape == (16, 1024, 768)


@pytest.mark.parametrize("H,W", [(224, 224), (48, 80)])
def test_vit_small_and_token_counts_that_fill_no_tile(H, W):
    _against_restatement(384, 4, 6, 3, H, W, seed=2)


def test_two_runs_are_bitwise(full_size):
    ours, images, gout, o, gr = full_size
    o2, gr2 = _run(ours, images, gout)
    assert torch.equal(o, o2)
    for n in gr:
        assert torch.equal(gr[n], gr2[n]), n


def test_inference_form_equals_the_training_forward(full_size):
    ours, images, _, o, _ = full_size
    with torch.no_grad():
        o1 = ours(images)
    with torch.inference_mode():
        o2 = ours(images)
    assert torch.equal(o1, o) and torch.equal(o2, o)


def test_strided_tar_rgb_equals_a_contiguous_copy():
    ours, _ = _models(384, 2, 6, seed=3)
    g = torch.Generator().manual_seed(4)
    rgb = torch.rand(2, 6, 64, 96, 3, generator=g).to(DEV)          # [B, V, H, W, 3]; the encoder reads views 0..3 in place
    batch = {"tar_rgb": rgb}
    feats = ours.image_features(batch, 4)
    assert feats.shape == (8, 384, 4, 6) and feats.permute(0, 2, 3, 1).is_contiguous()
    copy = rgb[:, :4].reshape(8, 64, 96, 3).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(feats.permute(0, 2, 3, 1).reshape(8, 24, 384), ours(copy))
    gout = torch.randn(8, 384, 4, 6, generator=g).to(DEV)
    ours.zero_grad()
    (ours.image_features(batch, 4) * gout).sum().backward()
    ga = [p.grad.clone() for p in ours.parameters()]
    ours.zero_grad()
    (ours(copy) * gout.flatten(2).transpose(1, 2)).sum().backward()
    for a, p in zip(ga, ours.parameters()):
        assert torch.equal(a, p.grad)


def test_pipeline_from_images():
    from lara_amd.featvol import FeatureVolume
    from lara_amd.pipeline import lara_loss
    from tests.test_pipeline import _small_problem
    pipe, batch, _ = _small_problem(DEV)
    pipe.fine_mask = "plain"
    pipe.n_streams = 1        # one stream: this test creates no HIP streams of its own (test_stream_safety_gpu.py counts on the mapping)
    pipe.feat_volume = FeatureVolume(C=768, E=32, R=2).to(DEV)
    ours, ref = _models(768, 2, 12, seed=5)
    pipe.image_encoder = ours

    def step(make, model, with_fine):
        pipe.zero_grad()
        model.zero_grad()
        out = make(with_fine)
        lara_loss(batch, out, ms_ssim=False)[0].backward()
        pipe.join_streams()
        return out, [p.grad.clone() for p in model.parameters()]

    o1, g1 = step(lambda wf: pipe.forward_from_images(batch, wf), ours, True)
    o2, g2 = step(lambda wf: pipe.forward_from_image_features(batch, ours.image_features(batch, 4), wf), ours, True)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)

    def restated(autocast):
        def make(wf):
            B, _, H, W, _ = batch["tar_rgb"].shape
            imgs = batch["tar_rgb"][:, :4].reshape(B * 4, H, W, 3).permute(0, 3, 1, 2)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                tok = ref(imgs)
            return pipe.forward_from_image_features(batch, tok.float().transpose(1, 2).reshape(B * 4, 768, H // 16, W // 16), wf)
        return make

    # against the same step fed the restatement's tokens (coarse stage only: the fine stage's mask is a threshold)
    oh, gh = step(lambda wf: pipe.forward_from_images(batch, wf), ours, False)
    ob, gb = step(restated(True), ref, False)
    of, gf = step(restated(False), ref, False)
    for k in oh:
        if torch.is_tensor(oh[k]) and oh[k].is_floating_point():
            _within_budget(oh[k].float(), ob[k].float(), of[k].float(), k)
    for (n, _), a, b, c in zip(ours.named_parameters(), gh, gb, gf):
        _within_budget(a, b, c, n)
