"""The volume transformer block and head, stage by stage, against the bf16-faithful fp64 reference
(oracle/voltrans_bf16.py: fp64 arithmetic, rounded to bf16 exactly where the kernels round).

CPU tests (no mark): the reference with its roundings off IS the fp32 restatement of oracle/voltrans_ref.py (values and
autograd gradients); its rounding markers agree bit for bit with torch's bf16 cast; and the yardstick N of the backward bar
measures bf16 noise at every case (1e-3 <= N <= 5e-2).

GPU tests, at shapes (scenes, R, cond_dim) that reach what the multiples-of-128 shapes of the other files never do:
    (1, 4, 800)  M = 64    the smallest legal volume, every voxel on the boundary, one partial tile everywhere
    (1, 6, 800)  M = 216   ragged against 64 / 128 / 256 rows, G = 27 (odd, 27 mod 4 = 3), interior voxels
    (3, 6, 96)   M = 648   two full 256-row tiles + 136, scene boundaries inside tiles, 3 K tiles in the K|V product
    (2, 4, 32)   M = 128   one K tile

(a) forward, teacher-forced: every saved stage is recomputed in fp64 from the DEVICE's saved inputs of that stage and must
    satisfy, for every element (no exemptions),
        bf16 stages   |got - ref| <= ulp_bf16(ref) + A           fp32 stages   |got - ref| <= 4 A + 2^-23 |ref|
    with ref the unrounded fp64 value and A the fp32 accumulation bound K 2^-24 (|a| . |b|) of the stage's product (a 256-term
    bound on both moments for a LayerNorm).  Three stages carry a named extra term in A:
      o      P = bf16(softmax) is rounded on the device but not saved.  Where the fp64 P lies within the fp32 softmax's own
             error (4 A_score + 2^-23 |s - max| + 16 * 2^-24, relative: both exponentials' arguments, v_exp_f32, the four-term
             sum, the reciprocal and the product) of a rounding tie, the device may round it the other way: A gains
             ulp_bf16(P) |v| for those P.
      h      is gelu of the fp32, unrounded pre-activation (not of the saved bf16 z): the reference takes the pre-activation
             from the device's xn2, and A = 1.13 A_z (the largest slope of gelu) + |z| (1.5e-7 + 8 * 2^-24): the
             Abramowitz-Stegun erf the kernel uses (|error| <= 1.5e-7) and its v_exp / v_rcp.
      out    (head) xn = bf16(norm(x)) is not saved: the same tie term as for P, ulp_bf16(xn) |wdeconv|.
    `lara_groupblock_forward` (in place) gives x_out bit for bit at every case.
(b) backward of one block against the reference's autograd evaluated on the device's saved forward: g, dcond / dK|dV and all
    fourteen parameter gradients, through every branch of the interface (accumulation into pre-filled buffers, dkv != NULL with
    a sentinel beside it, saved = NULL, chained, bit-reproducibility).
(c) the head, forward and backward, Cout in {16, 80}.

The backward bar.  Per tensor, N = ||faithful - unrounded||_2 / ||unrounded||_2 (the bf16 noise itself, from the reference
alone) and E = ||device - faithful||_2 / ||unrounded||_2; the test asserts E <= BAR * N with one BAR for all tensors and cases.
Every E, N and ratio (also in the max-norm) goes to voltrans_stage_errors.json, written the way test_raster_parity_gpu.py
writes its contributor log, into the directory LARA2DGS_TEST_OUT names: set it to the directory the run's logs are collected
from (default: test_out/ in the repository root, kept out of git).
Measured on an MI355X (first clean run, all four cases, block and head): the largest E / N is 0.126 (dln1_b, dln1_w at
(3, 6, 96); 0.10 - 0.12 for g, dkv, dwkv, dcond at the two small-cond_dim cases, <= 0.064 at cond_dim 800, <= 0.008 for the
head).  Twice that is 0.252, above the 0.25 the bar may not exceed: BAR = 0.25, i.e. 1.98 x the measured maximum.
The ratio grows along the backward chain in every case (wconv, ln3, b2: < 0.001; w2 0.0004 - 0.018; w1, b1 0.002 - 0.07;
ln2 0.02 - 0.09; dkv, wkv, dcond 0.05 - 0.11; ln1, g 0.03 - 0.13): a deviation far below an ulp in front of a bf16 rounding
(gb3, dzb, tmpb, gb2, dob, dq, dkv) comes out as a few elements rounded the other way, each a whole ulp, so every rounding
point multiplies what reached it.  The scratch stages themselves, read from the workspace in a scratch run (E / N and the
number of elements that differ from the reference), in chain order gb3, dzb, gb2, dob, dq:
    (1, 4, 800)  0.0008 (4 of 16 k)   0.0020   0.019   0.039   0.044
    (1, 6, 800)  0.0067 (16 of 55 k)  0.017    0.034   0.054   0.046
    (3, 6, 96)   0.023  (48 of 166 k) 0.034    0.063   0.106   0.093
    (2, 4, 32)   0.034  (5 of 33 k)   0.075    0.091   0.106   0.078
The first departure is gb3, the first rounding of the chain, behind the 6912-term transposed convolution and norm3's backward:
a handful of elements (<= 3e-4 of them) rounded the other way; what follows grows from there and no later stage jumps.  In the
max-norm the largest ratio is 0.57 (g at (3, 6, 96); 0.43 - 0.56 for dkv at every case): one element rounded the other way
is a whole bf16 ulp, as large as the largest noise term itself, so the max-norm is recorded and held to a second, separate
bar of 1.0 (a device deviation may not exceed the largest rounding-noise term), not to BAR.  Forward: the worst |diff| / limit is 0.500 for the
bf16 stages (half an ulp: the correctly rounded value) and 0.002 / 0.096 for the fp32 stages of the block / the head.

What these cases found: lara_groupblock_backward and lara_voltrans_head_backward returned LARA2DGS_E_INVALID for an odd
number of voxel groups (R = 6: M = 216 and the 108 key rows are no multiples of 16, which the direct weight-gradient kernel
required although the header promises any even R >= 4); the kernel now masks the rows of a last partial 16-row slice.
"""
import ctypes
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from lara_amd._native import load_library
from oracle import voltrans_bf16 as vb
from oracle.voltrans_ref import build_modules, restated_block, restated_cond, restated_voltrans

DEV = "cuda:0"
U = 2.0 ** -24
CASES = [(1, 4, 800), (1, 6, 800), (3, 6, 96), (2, 4, 32)]
COUTS = [16, 80]
# One bar for all tensors and cases: twice the largest E / N of the first clean run (2 x 0.126), capped at 0.25.
BAR = 0.25
BAR_MAX = 1.0      # max-norm: see the module docstring
STAGES = ("xn1", "q", "kv", "o", "x1", "xn2", "z", "h", "x2", "xn3", "stats")
_LOG = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    if not _LOG:
        return
    out = os.environ.get("LARA2DGS_TEST_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_out")
    os.makedirs(out, exist_ok=True)
    ratios = [v["ratio_l2"] for v in _LOG.values()]
    with open(os.path.join(out, "voltrans_stage_errors.json"), "w") as f:
        json.dump({"bar": BAR, "max_ratio_l2": max(ratios), "max_ratio_max": max(v["ratio_max"] for v in _LOG.values()),
                   "tensors": _LOG}, f, indent=1)


# ---------------------------------------------------------------------------------------------- inputs (seeded, shared)

def _perturbed_modules(seed, R):
    m = build_modules(seed, R, 1)
    g = torch.Generator().manual_seed(seed + 100)
    blk = m["layers"][0]
    with torch.no_grad():
        for ln in (blk["norm1"], blk["norm2"], blk["norm3"], m["norm"]):
            ln.weight.add_(0.3 * torch.randn(256, generator=g))
            ln.bias.add_(0.2 * torch.randn(256, generator=g))
        # the convolution branch as strong as the skip beside it: at the default initialisation (0.58 of the skip) the sums over
        # rows behind it (ln3_b, b2) carry bf16 noise of 0.9e-3 .. 1.0e-3 of their size, at the edge of what the yardstick accepts
        blk["cnn"].weight.mul_(2.0)
    return m


@functools.lru_cache(maxsize=None)
def case_inputs(scenes, R, cond_dim, seed=0):
    """x_in is NOT pos_embed: random rows whose mean and scale vary per row, so that LayerNorm statistics matter."""
    seed = seed + 7 * scenes + 13 * R + cond_dim
    m = _perturbed_modules(seed, R)
    g = torch.Generator().manual_seed(seed + 1)
    M = scenes * R ** 3
    x = torch.randn(M, 256, generator=g) * (0.5 + 1.5 * torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    cond = torch.randn(M // 2, cond_dim, generator=g).to(torch.bfloat16)
    g_out = torch.randn(M, 256, generator=g)
    douts = {c: torch.randn(scenes, 2 * R, 2 * R, 2 * R, c, generator=g) for c in COUTS}
    return {"m": m, "x": x.double(), "cond": cond.double(), "g_out": g_out.double(), "douts": {c: d.double() for c, d in douts.items()},
            "shape": (scenes, R, cond_dim), "M": M}


@functools.lru_cache(maxsize=None)
def reference_backward(scenes, R, cond_dim, seed=0):
    """(faithful, unrounded) gradients of the block, from the reference alone"""
    c = case_inputs(scenes, R, cond_dim, seed)
    blk = c["m"]["layers"][0]
    fa = vb.block_backward(c["x"], c["cond"], vb.block_weights(blk, cond_dim, True), scenes, R, c["g_out"], True)
    un = vb.block_backward(c["x"], c["cond"], vb.block_weights(blk, cond_dim, False), scenes, R, c["g_out"], False)
    return fa, un


@functools.lru_cache(maxsize=None)
def reference_head_backward(scenes, R, Cout):
    c = case_inputs(scenes, R, CASES[[s[:2] for s in CASES].index((scenes, R))][2])
    fa = vb.head_backward(c["x"], vb.head_weights(c["m"], Cout, True), scenes, R, c["douts"][Cout], True)
    un = vb.head_backward(c["x"], vb.head_weights(c["m"], Cout, False), scenes, R, c["douts"][Cout], False)
    return fa, un


def _rel(a, b, ref):
    a, b, ref = a.double().reshape(-1), b.double().reshape(-1), ref.double().reshape(-1)
    return float((a - b).norm() / ref.norm()), float((a - b).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------- CPU tests

def test_markers_round_like_torch_bfloat16():
    f32 = torch.float32
    special = torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 1.0 + 2.0 ** -8 + 2.0 ** -20, 3.3895313892515355e38,
                            3.3961775292304601e38, -3.3961775292304601e38, 3.4028234663852886e38, 1e-40, -1e-40, 9.1835e-41, 4.5918e-41,
                            1.4e-45, 1.1754943508222875e-38, float("inf"), -float("inf")], dtype=f32)
    # ties of every parity: k * 2^-8 + 2^-9 steps around 1 and around a power-of-two boundary
    ties = torch.cat([1.0 + (torch.arange(64, dtype=f32) + 0.5) * 2.0 ** -7, 2.0 - (torch.arange(64, dtype=f32) + 0.5) * 2.0 ** -8,
                      (torch.arange(1, 200, dtype=f32)) * 2.0 ** -133 * 0.5])
    rnd = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * torch.logspace(-30, 30, 4096)
    v = torch.cat([special, ties, rnd.to(f32)])
    want = v.to(torch.bfloat16).to(f32)
    got = vb.rf(v.double()).to(f32)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(vb.round_bf16(v).view(torch.int32), want.view(torch.int32))
    nan = vb.round_bf16(torch.tensor([float("nan")]))
    assert torch.isnan(nan).all()
    x = v[torch.isfinite(v)].double().requires_grad_(True)
    vb.rb(x).backward(x.detach())                               # rb: identity forward, rounded gradient
    assert torch.equal(x.grad.to(f32).view(torch.int32), want[torch.isfinite(v)].view(torch.int32))
    y = x.detach().clone().requires_grad_(True)
    out = vb.rf(y)
    out.backward(torch.full_like(y, 1.0 + 2.0 ** -12))          # rf: rounded forward, gradient untouched
    assert torch.equal(y.grad, torch.full_like(y, 1.0 + 2.0 ** -12))
    z = x.detach().clone().requires_grad_(True)
    assert torch.equal(vb.rf(z, False), z) and torch.equal(vb.rb(z, False), z)


def test_unrounded_reference_is_the_fp32_restatement():
    """rounding off: block and head reproduce restated_block / restated_voltrans and their autograd gradients"""
    B, R = 1, 4
    m = _perturbed_modules(5, R)
    blk = m["layers"][0]
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(B, 4, 800, 2, 2, 2, generator=g)
    dout = torch.randn(B, 8, 8, 8, 80, generator=g)
    m["pos"].requires_grad_(True)
    feats.requires_grad_(True)
    out32 = restated_voltrans(m, feats)
    (out32 * dout).sum().backward()
    params32 = {"ln1_w": blk["norm1"].weight, "ln1_b": blk["norm1"].bias, "wq": blk["mha"].q_proj_weight, "wo": blk["mha"].out_proj.weight,
                "ln2_w": blk["norm2"].weight, "ln2_b": blk["norm2"].bias, "w1": blk["mlp"][0].weight, "b1": blk["mlp"][0].bias,
                "w2": blk["mlp"][3].weight, "b2": blk["mlp"][3].bias, "ln3_w": blk["norm3"].weight, "ln3_b": blk["norm3"].bias,
                "wconv": blk["cnn"].weight}
    # the same through the reference, roundings off
    w = vb.block_weights(blk, None, False)
    hw = vb.head_weights(m, 80, False)
    x = vb.volume_to_rows(m["pos"].detach().double().expand(B, -1, -1, -1, -1).contiguous()).requires_grad_(True)
    cond = restated_cond(feats.detach()).reshape(-1, 800).double().requires_grad_(True)
    s = vb.block(x, cond, w, B, R, False)
    out64 = vb.head(s["x_out"], hw, B, R, False)
    (out64 * dout.double()).sum().backward()
    blk_out32 = restated_block(blk, m["pos"].detach().expand(B, -1, -1, -1, -1).contiguous(), restated_cond(feats.detach()))
    torch.testing.assert_close(vb.rows_to_volume(s["x_out"].detach(), B, R).float(), blk_out32.detach(), atol=2e-5, rtol=1e-4)
    torch.testing.assert_close(out64.detach().float(), out32.detach(), atol=2e-5, rtol=1e-4)

    def close(got, ref, name):
        err = float((got.double() - ref.double()).abs().max()) / float(ref.abs().max())
        assert err <= 2e-4, f"{name}: {err:.3e}"
    close(vb.rows_to_volume(x.grad, B, R).sum(0, keepdim=True), m["pos"].grad, "pos")
    close(cond.grad.view(B, 2, 2, 2, 4, 800).permute(0, 4, 5, 1, 2, 3), feats.grad, "feats")
    for k, p in params32.items():
        close(w[k].grad, p.grad, k)
    close(w["wkv"].grad, torch.cat([blk["mha"].k_proj_weight.grad, blk["mha"].v_proj_weight.grad], 0), "wkv")
    close(hw["ln_w"].grad, m["norm"].weight.grad, "norm.weight")
    close(hw["ln_b"].grad, m["norm"].bias.grad, "norm.bias")
    close(hw["wd"].grad.view(2, 2, 2, 80, 256).permute(4, 3, 0, 1, 2), m["deconv"].weight.grad, "deconv.weight")
    close(hw["bias8"].grad.view(8, 80).sum(0), m["deconv"].bias.grad, "deconv.bias")


@pytest.mark.parametrize("scenes,R,cond_dim", CASES)
def test_yardstick_measures_bf16_noise(scenes, R, cond_dim):
    """N = ||faithful - unrounded|| / ||unrounded|| must be the size of bf16 noise for every tensor: outside [1e-3, 5e-2] the
    backward bar (a multiple of N) would not be measuring against rounding noise."""
    fa, un = reference_backward(scenes, R, cond_dim)
    for k in un:
        n2, _ = _rel(fa[k], un[k], un[k])
        assert 1e-3 <= n2 <= 5e-2, f"block {k}: N = {n2:.3e}"
    for Cout in COUTS:
        fa, un = reference_head_backward(scenes, R, Cout)
        for k in un:
            n2, _ = _rel(fa[k], un[k], un[k])
            assert 1e-3 <= n2 <= 5e-2, f"head[{Cout}] {k}: N = {n2:.3e}"


# ---------------------------------------------------------------------------------------------- bounds

def ulp_bf16(ref):
    _, e = torch.frexp(ref.abs().double())
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e.clamp(min=-125) - 8)


def gemm_A(a, b, K):
    """fp32 accumulation bound of a . b^T over K terms: K 2^-24 (|a| . |b|)"""
    return K * U * (a.abs() @ b.abs().t())


def ln_A(x, w, b, eps):
    """bounds for fp32 LayerNorm(256) of x with two-pass moments: (A of the output, A of mean, A of rstd)"""
    mean = x.mean(-1, keepdim=True)
    em = 256 * U * x.abs().mean(-1, keepdim=True)
    c = x - mean
    ec = em + U * c.abs()
    var = (c * c).mean(-1, keepdim=True)
    dvar = (2 * c.abs() * ec).mean(-1, keepdim=True) + 258 * U * var
    rstd = 1.0 / torch.sqrt(var + eps)
    rel = dvar / (2 * (var + eps)) + 3 * U
    y = c * rstd * w + b
    return w.abs() * rstd * ec + (c * rstd * w).abs() * (rel + 3 * U) + U * y.abs(), em[:, 0], (rstd * rel)[:, 0]


def tie_flip_ulp(val, err):
    """ulp_bf16(val) where val lies within `err` of a bf16 rounding tie (the device, whose fp32 value differs from val by up to
    err, may then round the other way), else 0"""
    ulp = ulp_bf16(val)
    r = vb.round_bf16(val)
    sgn = torch.where(val >= r, 1.0, -1.0)
    d = (val - (r + sgn * ulp / 2)).abs()       # (ulp is that of val's own binade: the tie beside val is at r +- ulp / 2)
    return torch.where(d <= err, ulp, torch.zeros_like(ulp))


_FAILS = []      # every stage of a test is checked (and printed) before the test asserts that none failed


def _no_failures():
    msg = "; ".join(_FAILS)
    _FAILS.clear()
    assert not msg, msg


def check_bf16(name, got, ref, A):
    d = (got.double() - ref).abs()
    lim = ulp_bf16(ref) + A
    bad = d > lim
    print(f"{name:12s} worst |diff| / (ulp_bf16 + A) = {float((d / lim).max()):.3f}")
    if bad.any():
        _FAILS.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond ulp_bf16 + A; worst |diff| / limit = {float((d / lim).max()):.3f}")


def check_fp32(name, got, ref, A):
    d = (got.double() - ref).abs()
    lim = 4 * A + 2.0 ** -23 * ref.abs()
    bad = d > lim
    print(f"{name:12s} worst |diff| / (4 A + 2^-23 |ref|) = {float((d / lim).max()):.3f}")
    if bad.any():
        _FAILS.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond 4 A + 2^-23 |ref|; worst |diff| / limit = {float((d / lim).max()):.3f}")


# ---------------------------------------------------------------------------------------------- device plumbing

def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev_weights(w):
    """the reference's (bf16-valued) fp64 operands -> the device's structs; returns (tensors, weights struct, transposed struct)"""
    from lara_amd.encoder import _BlockWeights
    from lara_amd.encoder_train import _BlockWeightsT, _GRAD_FIELDS, _fill, _transposed
    bf = torch.bfloat16
    f = {}
    for k in _GRAD_FIELDS:
        t = w[k].detach()
        if k == "wconv":
            t = t.permute(0, 2, 3, 4, 1).reshape(256, 27 * 256)
        f[k] = (t.to(bf) if k in ("wq", "wkv", "wo", "w1", "w2", "wconv") else t.float()).contiguous().to(DEV)
    ft = _transposed(f)
    ws = _fill(_BlockWeights(), f, _GRAD_FIELDS)
    ws.eps = w["eps"]
    wt = _fill(_BlockWeightsT(), ft, ("wq_t", "wkv_t", "wo_t", "w1_t", "w2_t", "wconv_t"))
    return (f, ft), ws, wt


def _read_saved(lib, saved, scenes, R):
    M = scenes * R ** 3
    offs = (ctypes.c_int64 * 11)()
    assert lib.lara_groupblock_save_offsets(scenes, R, offs, 11) == 0
    assert lib.lara_groupblock_save_offsets(scenes, R, offs, 10) != 0 and lib.lara_groupblock_save_offsets(scenes, 5, offs, 11) != 0
    shapes = {"xn1": (M, 256), "q": (M, 256), "kv": (M // 2, 512), "o": (M, 256), "x1": (M, 256), "xn2": (M, 256), "z": (M, 512),
              "h": (M, 512), "x2": (M, 256), "xn3": (M + 1, 256), "stats": (M, 2)}
    out = {}
    for name, off in zip(STAGES, offs):
        dt = torch.float32 if name in ("x1", "x2", "stats") else torch.bfloat16
        n = shapes[name][0] * shapes[name][1] * (4 if dt == torch.float32 else 2)
        out[name] = saved[off:off + n].view(dt).view(shapes[name]).cpu().double()
    return out


_DEVICE = {}


def device_forward(scenes, R, cond_dim):
    """one lara_groupblock_forward_train per case, shared by the tests of that case"""
    key = (scenes, R, cond_dim)
    if key in _DEVICE:
        return _DEVICE[key]
    lib = load_library()
    c = case_inputs(scenes, R, cond_dim)
    w = vb.block_weights(c["m"]["layers"][0], cond_dim, True)
    keep, ws, wt = _dev_weights(w)
    x = c["x"].float().to(DEV)
    cond = c["cond"].to(torch.bfloat16).to(DEV)
    x_out = torch.full_like(x, float("nan"))
    saved = torch.full((int(lib.lara_groupblock_save_bytes(scenes, R)),), 0xFF, dtype=torch.uint8, device=DEV)
    rc = lib.lara_groupblock_forward_train(scenes, R, cond_dim, x.data_ptr(), x_out.data_ptr(), cond.data_ptr(), ctypes.byref(ws),
                                           saved.data_ptr(), _s())
    torch.cuda.synchronize()
    assert rc == 0, rc
    d = {"w": w, "keep": keep, "ws": ws, "wt": wt, "x": x, "cond": cond, "x_out": x_out, "saved": saved,
         "stages": _read_saved(lib, saved, scenes, R), "c": c}
    _DEVICE[key] = d
    return d


# ---------------------------------------------------------------------------------------------- (a) forward

@pytest.mark.gpu
@pytest.mark.parametrize("scenes,R,cond_dim", CASES)
def test_forward_stages_teacher_forced(hip_lib, scenes, R, cond_dim):
    _FAILS.clear()
    d = device_forward(scenes, R, cond_dim)
    c, S = d["c"], d["stages"]
    w = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in d["w"].items()}
    M, eps = c["M"], w["eps"]
    x_in, cond = c["x"], c["cond"]
    # xn1 from x_in
    A, _, _ = ln_A(x_in, w["ln1_w"], w["ln1_b"], eps)
    check_bf16("xn1", S["xn1"], vb.st_ln(x_in, w["ln1_w"], w["ln1_b"], eps), A)
    # kv from cond, q from xn1
    check_bf16("kv", S["kv"], vb.st_kv(cond, w["wkv"]), gemm_A(cond, w["wkv"], cond_dim))
    check_bf16("q", S["q"], vb.st_q(S["xn1"], w["wq"]), gemm_A(S["xn1"], w["wq"], 256))
    # o from q, kv: P = bf16(softmax) is not saved -> the tie term (module docstring)
    p, s, vh = vb.attn_probs(S["q"], S["kv"])
    G = M // 8
    qh = S["q"].view(G, 8, 16, 16).transpose(1, 2)
    kh = S["kv"][:, :256].reshape(G, 4, 16, 16).transpose(1, 2)
    A_s = 16 * U * 0.25 * (qh.abs() @ kh.abs().transpose(-1, -2)) + U * s.abs()
    p_rel = 4 * A_s.amax(-1, keepdim=True) + 2 * U * (s - s.amax(-1, keepdim=True)).abs() + 16 * U
    flip = tie_flip_ulp(p, p_rel * p)
    pb = vb.round_bf16(p)
    A_o = (16 * U * (pb @ vh.abs()) + flip @ vh.abs()).transpose(1, 2).reshape(M, 256)
    check_bf16("o", S["o"], (pb @ vh).transpose(1, 2).reshape(M, 256), A_o)
    print(f"o: {int((flip > 0).sum())} of {flip.numel()} probabilities within the softmax's error of a tie")
    # x1 from o, x_in
    check_fp32("x1", S["x1"], vb.st_x1(S["o"], x_in, w["wo"]), gemm_A(S["o"], w["wo"], 256))
    # xn2 from x1
    A, _, _ = ln_A(S["x1"], w["ln2_w"], w["ln2_b"], eps)
    check_bf16("xn2", S["xn2"], vb.st_ln(S["x1"], w["ln2_w"], w["ln2_b"], eps), A)
    # z from xn2; h from the same fp32 pre-activation (module docstring)
    zpre = vb.st_z(S["xn2"], w["w1"], w["b1"])
    A_z = gemm_A(S["xn2"], w["w1"], 256) + U * (zpre.abs() + w["b1"].abs())
    check_bf16("z", S["z"], zpre, A_z)
    check_bf16("h", S["h"], F.gelu(zpre), 1.13 * A_z + zpre.abs() * (1.5e-7 + 8 * U))
    # x2 from h, x1
    check_fp32("x2", S["x2"], vb.st_x2(S["h"], S["x1"], w["w2"], w["b2"]), gemm_A(S["h"], w["w2"], 512) + U * w["b2"].abs())
    # xn3 and stats from x2; row M of xn3 reads zero
    A, A_mean, A_rstd = ln_A(S["x2"], w["ln3_w"], w["ln3_b"], eps)
    pn = vb.st_ln(S["x2"], w["ln3_w"], w["ln3_b"], eps)
    check_bf16("xn3", S["xn3"][:M], pn, A)
    assert torch.equal(S["xn3"][M], torch.zeros(256, dtype=torch.float64)), "row M of xn3 (the convolution's padding voxels)"
    st = vb.st_stats(S["x2"], eps)
    check_fp32("stats.mean", S["stats"][:, 0], st[:, 0], A_mean)
    check_fp32("stats.rstd", S["stats"][:, 1], st[:, 1], A_rstd)
    # x_out from xn3, x2
    xn3 = S["xn3"][:M]
    A_conv = 27 * 256 * U * vb.st_conv(xn3.abs(), w["wconv"].abs(), scenes, R)
    check_fp32("x_out", d["x_out"].cpu(), pn + vb.st_conv(xn3, w["wconv"], scenes, R), A_conv + A)
    # the in-place inference entry gives the same bits
    lib = load_library()
    xi = d["x"].clone()
    ws = torch.full((int(lib.lara_groupblock_workspace_bytes(scenes, R)),), 0xFF, dtype=torch.uint8, device=DEV)
    assert lib.lara_groupblock_forward(scenes, R, cond_dim, xi.data_ptr(), d["cond"].data_ptr(), ctypes.byref(d["ws"]), ws.data_ptr(), _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(xi, d["x_out"]), "lara_groupblock_forward (in place) != lara_groupblock_forward_train"
    _no_failures()


# ---------------------------------------------------------------------------------------------- (b) backward

def _grads(prefill_seed, cond_shape):
    """pre-filled fp32 accumulators (seeded, non-zero) in the layouts of lara_groupblock_grads, and a pre-filled dcond"""
    from lara_amd.encoder_train import _BlockGrads, _GRAD_FIELDS, _fill
    g = torch.Generator().manual_seed(prefill_seed)
    shapes = {"ln1_w": (256,), "ln1_b": (256,), "wq": (256, 256), "wkv": (512, cond_shape[1]), "wo": (256, 256), "ln2_w": (256,),
              "ln2_b": (256,), "w1": (512, 256), "b1": (512,), "w2": (256, 512), "b2": (256,), "ln3_w": (256,), "ln3_b": (256,),
              "wconv": (256, 27, 256)}
    pre = {k: 0.5 * torch.randn(s, generator=g) for k, s in shapes.items()}
    pre["dcond"] = 0.5 * torch.randn(cond_shape, generator=g)
    dev = {k: v.clone().to(DEV) for k, v in pre.items()}
    return pre, dev, _fill(_BlockGrads(), dev, _GRAD_FIELDS)


def _run_backward(lib, d, scenes, R, cond_dim, g_in, *, saved=True, dkv=None, lddkv=0, chained=0, ws=None, x=None, cond_shape=None,
                  handles=None):
    """one lara_groupblock_backward call; returns (g, accumulators on the device, their pre-fill, workspace)"""
    h = handles or d
    pre, dev, dw = _grads(11, cond_shape)
    g = g_in.clone()
    if ws is None:
        ws = torch.full((int(lib.lara_groupblock_backward_workspace_bytes(scenes, R)),), 0xFF, dtype=torch.uint8, device=DEV)
    rc = lib.lara_groupblock_backward(scenes, R, cond_dim, (h["x"] if x is None else x).data_ptr(), d["cond"].data_ptr(), ctypes.byref(h["ws"]),
                                      ctypes.byref(h["wt"]), h["saved"].data_ptr() if saved else None, g.data_ptr(),
                                      None if dkv is not None else dev["dcond"].data_ptr(), ctypes.byref(dw), chained,
                                      None if dkv is None else dkv.data_ptr(), lddkv, ws.data_ptr(), _s())
    torch.cuda.synchronize()
    assert rc == 0, f"lara_groupblock_backward returned {rc}"
    return g, dev, pre, ws


@pytest.mark.gpu
@pytest.mark.parametrize("scenes,R,cond_dim", CASES)
def test_block_backward(hip_lib, scenes, R, cond_dim):
    lib = load_library()
    d = device_forward(scenes, R, cond_dim)
    c, S = d["c"], d["stages"]
    M = c["M"]
    cshape = (M // 2, cond_dim)
    g_in = c["g_out"].float().to(DEV)
    # the reference: faithful on the device's saved forward; the yardstick from the reference alone
    forced = {k: S[k] for k in ("xn1", "q", "kv", "o", "x1", "xn2", "z", "h", "x2")}
    forced["xn3"] = S["xn3"][:M]
    faf = vb.block_backward(c["x"], c["cond"], d["w"], scenes, R, c["g_out"], True, forced)
    fa, un = reference_backward(scenes, R, cond_dim)
    # 1. dkv == NULL: dcond and every accumulator pre-filled; the result is pre-fill + gradient
    g1, acc1, pre, _ = _run_backward(lib, d, scenes, R, cond_dim, g_in, cond_shape=cshape)
    got = {k: acc1[k].cpu().double() - pre[k].double() for k in pre}
    got["g"] = g1.cpu().double()
    failures = []

    def measure(name, dev_t, key):
        e2, emax = _rel(dev_t, faf[key], un[key])
        n2, nmax = _rel(fa[key], un[key], un[key])
        _LOG[f"{scenes}x{R}^3/c{cond_dim}/{name}"] = {"E_l2": e2, "N_l2": n2, "ratio_l2": e2 / n2, "E_max": emax, "N_max": nmax,
                                                     "ratio_max": emax / nmax}
        print(f"{name:8s} E {e2:.3e}  N {n2:.3e}  E/N {e2 / n2:.4f}   max-norm: E {emax:.3e}  N {nmax:.3e}  E/N {emax / nmax:.4f}")
        if not e2 <= BAR * n2:
            failures.append(f"{name}: E = {e2:.3e} > {BAR} * N = {BAR * n2:.3e}")
        if not emax <= BAR_MAX * nmax:
            failures.append(f"{name}: max-norm E = {emax:.3e} > {BAR_MAX} * N = {BAR_MAX * nmax:.3e}")
    for k in ("g", "dcond") + vb.BLOCK_GRADS:
        measure(k, got[k], k)
    # 2. dkv != NULL, lddkv = 1024, dcond = NULL: this block's 512 columns are written, the other 512 untouched
    dkv = torch.full((M // 2, 1024), -7.0, dtype=torch.bfloat16, device=DEV)
    g2, acc2, _, _ = _run_backward(lib, d, scenes, R, cond_dim, g_in, dkv=dkv[:, 512:], lddkv=1024, cond_shape=cshape)
    assert torch.equal(dkv[:, :512], torch.full_like(dkv[:, :512], -7.0)), "columns beside this block's dK|dV were written"
    measure("dkv", dkv[:, 512:].float().cpu().double(), "dkv")
    assert torch.equal(acc2["dcond"].cpu(), pre["dcond"]), "dcond touched although dkv was given"
    assert torch.equal(g2, g1)
    for k in vb.BLOCK_GRADS:
        assert torch.equal(acc2[k], acc1[k]), f"{k}: differs between the dcond and the dkv form"
    # 3. two runs give identical bits (each on a fresh workspace filled with 0xFF: nothing uninitialised is read)
    g3, acc3, _, _ = _run_backward(lib, d, scenes, R, cond_dim, g_in, cond_shape=cshape)
    assert torch.equal(g3, g1)
    for k in pre:
        assert torch.equal(acc3[k], acc1[k]), f"{k}: not reproducible"
    # 4. saved = NULL: the forward is recomputed inside; every output has the same bits
    g4, acc4, _, _ = _run_backward(lib, d, scenes, R, cond_dim, g_in, saved=False, cond_shape=cshape)
    assert torch.equal(g4, g1)
    for k in pre:
        assert torch.equal(acc4[k], acc1[k]), f"{k}: recompute differs from the saved run"
    # 5. chained: a DIFFERENT block first (its input is this block's output), then this block with chained = 1 on the same
    #    workspace; against the same call with chained = 0 on a fresh 0xFF-filled workspace
    wB = vb.block_weights(_perturbed_modules(991 + R, R)["layers"][0], cond_dim, True)
    keepB, wsB, wtB = _dev_weights(wB)
    savedB = torch.full_like(d["saved"], 0xFF)
    xoB = torch.empty_like(d["x"])
    assert lib.lara_groupblock_forward_train(scenes, R, cond_dim, d["x_out"].data_ptr(), xoB.data_ptr(), d["cond"].data_ptr(),
                                             ctypes.byref(wsB), savedB.data_ptr(), _s()) == 0
    hB = {"x": d["x_out"], "ws": wsB, "wt": wtB, "saved": savedB}
    gB, _, _, ws_shared = _run_backward(lib, d, scenes, R, cond_dim, g_in, cond_shape=cshape, handles=hB)
    assert torch.isfinite(gB).all()
    gc, accc, _, _ = _run_backward(lib, d, scenes, R, cond_dim, gB, chained=1, ws=ws_shared, cond_shape=cshape)
    gf, accf, _, _ = _run_backward(lib, d, scenes, R, cond_dim, gB, chained=0, cond_shape=cshape)
    assert torch.equal(gc, gf), "chained call differs from the unchained one"
    for k in pre:
        assert torch.equal(accc[k], accf[k]), f"{k}: chained call differs from the unchained one"
    assert not failures, "; ".join(failures)


# ---------------------------------------------------------------------------------------------- (c) head

@pytest.mark.gpu
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("scenes,R,cond_dim", CASES)
def test_head_forward_and_backward(hip_lib, scenes, R, cond_dim, Cout):
    lib = load_library()
    c = case_inputs(scenes, R, cond_dim)
    M = c["M"]
    hw = vb.head_weights(c["m"], Cout, True)
    h = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in hw.items()}
    x = c["x"].float().to(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    ln_w, ln_b, bias = h["ln_w"].float().to(DEV), h["ln_b"].float().to(DEV), h["bias8"][:Cout].float().to(DEV)
    wd = h["wd"].to(torch.bfloat16).to(DEV)
    out = torch.full((scenes, 2 * R, 2 * R, 2 * R, Cout), float("nan"), **f32)
    ws = torch.full((M * 512,), 0xFF, dtype=torch.uint8, device=DEV)
    assert lib.lara_voltrans_head_forward(scenes, R, x.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), h["eps"], wd.data_ptr(),
                                          bias.data_ptr(), Cout, out.data_ptr(), ws.data_ptr(), _s()) == 0
    torch.cuda.synchronize()
    # forward: out from x; xn = bf16(norm(x)) is not saved -> the tie term
    A_ln, _, _ = ln_A(c["x"], h["ln_w"], h["ln_b"], h["eps"])
    pn = vb.st_ln(c["x"], h["ln_w"], h["ln_b"], h["eps"])
    xn = vb.round_bf16(pn)
    A = gemm_A(xn, h["wd"], 256) + tie_flip_ulp(pn, A_ln) @ h["wd"].abs().t() + U * h["bias8"].abs()
    ref = xn @ h["wd"].t() + h["bias8"]
    check_fp32(f"head out[{Cout}]", out.cpu(), vb.head_rows_to_out(ref, scenes, R, Cout), vb.head_rows_to_out(A, scenes, R, Cout))
    _no_failures()
    # backward, accumulators pre-filled
    dout = c["douts"][Cout]
    gen = torch.Generator().manual_seed(17)
    pre = {"ln_w": 0.5 * torch.randn(256, generator=gen), "ln_b": 0.5 * torch.randn(256, generator=gen),
           "wd": 0.5 * torch.randn(8 * Cout, 256, generator=gen), "bias8": 0.5 * torch.randn(8 * Cout, generator=gen)}
    acc = {k: v.clone().to(DEV) for k, v in pre.items()}
    g = torch.full((M, 256), float("nan"), **f32)
    wd_t = wd.t().contiguous()
    dd = dout.float().to(DEV)
    bws = torch.full((int(lib.lara_voltrans_head_backward_workspace_bytes(scenes, R, Cout)),), 0xFF, dtype=torch.uint8, device=DEV)
    rc = lib.lara_voltrans_head_backward(scenes, R, x.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), h["eps"], wd_t.data_ptr(), Cout,
                                         dd.data_ptr(), g.data_ptr(), acc["ln_w"].data_ptr(), acc["ln_b"].data_ptr(), acc["wd"].data_ptr(),
                                         acc["bias8"].data_ptr(), bws.data_ptr(), _s())
    torch.cuda.synchronize()
    assert rc == 0, f"lara_voltrans_head_backward returned {rc}"
    got = {k: acc[k].cpu().double() - pre[k].double() for k in pre}
    got["g"] = g.cpu().double()
    # the device's xn is not saved: the faithful reference runs on its own xn (a tie flip there is part of E)
    faf, un = reference_head_backward(scenes, R, Cout)
    failures = []
    for k in ("g",) + vb.HEAD_GRADS:
        e2, emax = _rel(got[k], faf[k], un[k])
        n2, nmax = _rel(faf[k], un[k], un[k])
        _LOG[f"{scenes}x{R}^3/head{Cout}/{k}"] = {"E_l2": e2, "N_l2": n2, "ratio_l2": e2 / n2, "E_max": emax, "N_max": nmax,
                                                 "ratio_max": emax / nmax}
        print(f"head[{Cout}] {k:6s} E {e2:.3e}  N {n2:.3e}  E/N {e2 / n2:.4f}   max-norm: E {emax:.3e}  N {nmax:.3e}  E/N {emax / nmax:.4f}")
        if not e2 <= BAR * n2:
            failures.append(f"{k}: E = {e2:.3e} > {BAR} * N = {BAR * n2:.3e}")
        if not emax <= BAR_MAX * nmax:
            failures.append(f"{k}: max-norm E = {emax:.3e} > {BAR_MAX} * N = {BAR_MAX * nmax:.3e}")
    assert not failures, "; ".join(failures)
