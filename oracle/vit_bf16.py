"""bf16-faithful fp64 reference of the DINO ViT image encoder -- TEST INFRASTRUCTURE ONLY (the checker of
tests/test_vit_bf16.py and tests/test_vit_stages_gpu.py; nothing under lara_amd/ imports it).

It restates, in torch fp64 on the CPU, what lara_vit_forward / lara_vit_backward (include/lara_vit.h, lara_amd/csrc/vit.hip)
compute, and rounds to bf16 exactly where the kernels do.  The two markers are those of oracle/voltrans_bf16.py:
    rf(x)  rounds x to bf16 in the forward, passes the gradient straight through
    rb(x)  identity in the forward, rounds the gradient to bf16 in the backward
so autograd through `forward` IS the faithful backward; only the attention core needs a Function of its own (AttnFn), because
its backward recomputes P from the saved lse and uses the saved, rounded O.  With on=False the same code is the plain network.

Where the device rounds (read off vit.hip):

forward
    a      = bf16((img - mean) / std)            patch_kernel: fp32 subtraction and a true fp32 division, then one rounding
    every weight matrix is cast to bf16 per call (wcast_kernel); every bias is rounded to bf16 before it is added
    x0     = [cls | bf16(a . Wpatch^T + bf16(b))] + pos                      tokens_kernel, fp32
    xn1    = bf16(LN1(x))                        ln_fwd_kernel (fp32 statistics, kept as (mean, rstd))
    q|k|v  = bf16(xn1 . Wqkv^T + bf16(b))        qkv_split_kernel, head-major [NH, Tp, 64]
    o      = bf16(sum_j exp(m_j - m_last) P~_j V_j / l)     attn_fwd_kernel: s = (q . k) / 8; per block j of 32 keys, m_j the running
             maximum, P~_j = bf16(exp(s - m_j)); l sums the UNROUNDED exponentials; lse = m_last + log l
    xmid   = x + bf16(o . Wproj^T + bf16(b))     residual_kernel
    xn2    = bf16(LN2(xmid))
    h      = bf16(xn2 . W1^T + bf16(b1));  g = bf16(gelu_erf(h)) of the ROUNDED h (g is not kept: gelu_kernel redoes it)
    xout   = xmid + bf16(g . W2^T + bf16(b2))
    out    = LN(x_depth)[:, 1:]                  fp32

backward (lara_vit_backward; dres is the fp32 gradient of the residual stream)
    dy     = bf16(dres)                          rows_bf16_kernel: the operand of dW2 / dWproj, of their bias sums and of the dX product
    dh     = bf16(bf16(dy . W2) * gelu'(h))      the product's bf16 output, then gelu_bwd_kernel
    dxn    = bf16(dh . W1), bf16(dqkv . Wqkv);  dob = bf16(dy . Wproj)
    D      = sum_d bf16(dO) bf16(O);  P = exp(s - lse);  dV = bf16(P)^T dO;  dS = bf16(P (dO V^T - D))
    dq, dk = bf16((dS K) / 8), bf16((dS^T Q) / 8);  dv = bf16(dV)
    dconv  = bf16(dres[:, 1:])
    weight gradients: products of the rounded rows; bias gradients: column sums of the rounded rows; dgamma, dbeta of a block's
    norms from the bf16 dxn and the fp32 x^; of the final norm from the fp32 grad.

`defects` (a set of names) builds one wrong kernel each into the same code, for tests/test_vit_bf16.py's proof that the stage
checks can see it: see DEFECTS.
"""
import math

import torch
import torch.nn.functional as F

from oracle.voltrans_bf16 import _force, rb, rf, round_bf16

HD = 64
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BLOCK_STAGES = ("xin", "xn1", "st1", "q", "k", "v", "o", "lse", "xmid", "xn2", "st2", "h")
BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
DEFECTS = {
    "last_key_block": "the padded keys of the last 32-key block are not masked (they enter the softmax with s = 0)",
    "cls_missing_dk": "the class token's row of dK is never written",
    "bias_unrounded": "biases are added in fp32, not rounded to bf16 first",
    "p_round_place": "P is rounded after the normalisation (bf16(softmax)) instead of per key block before it",
    "padded_row": "the first padded row of xn1, o, xn2 and h keeps what the buffer held (here: ones)",
    "gelu_tanh": "the tanh approximation in place of erf, forward and backward",
    "cls_missing_key": "the class token is left out of the forward's key loop",
    "score_rounded": "the scores are rounded to bf16 before the 1/8 scale",
    "scale_after_rounding": "dq, dk = bf16(acc) / 8 instead of bf16(acc / 8) -- the same bits (see test_vit_bf16.py)",
}


def param_names(depth):
    return (["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
            + [f"blocks.{i}.{n}" for i in range(depth) for n in BLOCK_PARAMS] + ["norm.weight", "norm.bias"])


def geometry(N, views, H, W, C, F_, depth):
    h, w = H // 16, W // 16
    T = 1 + h * w
    r = lambda v, m: (v + m - 1) // m * m
    return {"N": N, "views": views, "H": H, "W": W, "C": C, "F": F_, "depth": depth, "heads": C // HD, "h": h, "w": w, "hw": h * w,
            "T": T, "M": N * T, "Mp": r(N * T, 128), "Tp": r(T, 64), "NP": N * h * w, "Pp": r(N * h * w, 128), "NH": N * C // HD}


# ---------------------------------------------------------------------------------------------- stages (unrounded outputs)

def st_patches(images, on=True):
    """images [N, 3, H, W] (fp32 values) -> patch rows [N hw, 768] in (ch, ky, kx) order.  on: the subtraction and the division in
    fp32 (each exactly rounded, as the device's), then bf16; off: plain fp64."""
    N, _, H, W = images.shape
    if on:
        x = images.to(torch.float32)
        x = (x - torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
        x = round_bf16(x).double()
    else:
        # (the fp32 constants, as the restatement's: only the arithmetic is fp64)
        x = (images.double() - torch.tensor(MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)) \
            / torch.tensor(STD, dtype=torch.float32).double().view(1, 3, 1, 1)
    return x.view(N, 3, H // 16, 16, W // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(N * (H // 16) * (W // 16), 768)


def st_ln(x, w, b, eps):
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


def st_stats(x, eps):
    mean = x.mean(-1)
    var = ((x - mean[..., None]) ** 2).mean(-1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], -1)


def split_heads(rows, N, T):
    """[N T, C] -> [N, heads, T, 64]"""
    return rows.view(N, T, -1, HD).transpose(1, 2)


def merge_heads(x):
    N, Hh, T, _ = x.shape
    return x.transpose(1, 2).reshape(N * T, Hh * HD)


def gelu(x, tanh=False):
    return F.gelu(x, approximate="tanh") if tanh else F.gelu(x)


def attn_scores(q, k, defects=()):
    s = q @ k.transpose(-1, -2)
    if "score_rounded" in defects:
        s = round_bf16(s)
    return s * 0.125


def attn_core(q, k, v, defects=()):
    """The forward as attn_fwd_kernel runs it, on [N, heads, T, 64] (bf16 values): -> dict with o (unrounded), lse, and what the
    stage check needs for its bound: s, the per-key running maximum mk, the unrounded e = exp(s - mk), the block weights wk =
    exp(m_j - m_last) per key and l."""
    T = q.shape[-2]
    nb = (T + 31) // 32
    s = attn_scores(q, k, defects)
    live = torch.ones(T, dtype=torch.bool)
    if "cls_missing_key" in defects:
        live[0] = False
    sm = s.masked_fill(~live, -math.inf)
    pad = nb * 32 - T
    fill = 0.0 if "last_key_block" in defects else -math.inf
    sp = F.pad(sm, (0, pad), value=fill)
    bm = sp.view(*sp.shape[:-1], nb, 32).amax(-1)
    mj = torch.cummax(bm, -1).values                              # running maximum behind block j
    m_last = mj[..., -1:]
    mk = mj.repeat_interleave(32, -1)
    e_all = torch.exp(sp - mk)
    wk_all = torch.exp(mk - m_last)
    l = (e_all * wk_all).sum(-1, keepdim=True)                    # = sum_k exp(s_k - m_last): the device's l, up to fp32 rounding
    e, wk, mk = e_all[..., :T], wk_all[..., :T], mk[..., :T]
    if "p_round_place" in defects:
        o = round_bf16(e * wk / l) @ v
    else:
        o = (round_bf16(e) * wk) @ v / l
    return {"o": o, "lse": (m_last + torch.log(l))[..., 0], "s": s, "mk": mk, "e": e, "wk": wk, "l": l, "m": m_last}


class AttnFn(torch.autograd.Function):
    """value: the (unrounded) output of attn_core; backward: attn_dvec_kernel / attn_dq_kernel / attn_dkv_kernel on the saved
    rounded o and the saved lse."""
    @staticmethod
    def forward(ctx, q, k, v, o_pre, o_saved, lse, defects):
        ctx.save_for_backward(q, k, v, o_saved, lse)
        ctx.defects = defects
        return o_pre.clone()

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        df = ctx.defects
        D = (do * o).sum(-1, keepdim=True)
        p = torch.exp(attn_scores(q, k, df) - lse[..., None])
        dv = round_bf16(p).transpose(-1, -2) @ do
        ds = round_bf16(p * (do @ v.transpose(-1, -2) - D))
        dq, dk = ds @ k, ds.transpose(-1, -2) @ q
        if "scale_after_rounding" in df:
            dq, dk = round_bf16(dq) * 0.125, round_bf16(dk) * 0.125
        else:
            dq, dk = dq * 0.125, dk * 0.125
        if "cls_missing_dk" in df:
            dk = dk.clone()
            dk[..., 0, :] = 0.0
        return dq, dk, dv, None, None, None, None


def attention(q, k, v, on, forced, pre, defects):
    """-> (o_pre with the faithful backward, o rounded / forced, lse)"""
    if not on:
        sc = q @ k.transpose(-1, -2) * 0.125
        a = torch.softmax(sc, -1) @ v
        return a, merge_heads(a), torch.logsumexp(sc.detach(), -1)
    core = attn_core(q.detach(), k.detach(), v.detach(), defects)
    N, _, T, _ = q.shape
    o_saved = _force(round_bf16(merge_heads(core["o"])), forced, pre + "o")
    lse = _force(core["lse"], forced, pre + "lse")
    node = AttnFn.apply(q, k, v, core["o"], split_heads(o_saved, N, T), lse, frozenset(defects))
    return node, o_saved, lse


# ---------------------------------------------------------------------------------------------- the encoder

def make_params(values, requires_grad=True):
    """fp32-valued tensors in lara_vit.h order -> fp64 leaves"""
    return [v.detach().to(torch.float32).double().clone().requires_grad_(requires_grad) for v in values]


def forward(images, params, geo, eps=1e-6, on=True, forced=None, defects=()):
    """images [N, 3, H, W] (values of fp32), params: make_params' list (pos_embed [T, C] already on this grid).  Returns every
    stage as the device keeps it -- 'patches', per block 'b{i}.' + BLOCK_STAGES (token rows [M, .]; q, k, v as [N, heads, T, 64]),
    'xfin', 'stf', 'out' [N, hw, C] -- and, for the bounds of the stage checks, the unrounded products 'b{i}.pre_*'.  `forced`:
    device values that replace stages in the forward (the gradient then is evaluated on the device's own activations)."""
    N, T, C, depth = geo["N"], geo["T"], geo["C"], geo["depth"]
    df = frozenset(defects)
    fo = lambda t, n: _force(t, forced, n)
    wm = lambda i: rf(params[i], on)                                # a weight matrix as the kernels see it
    bias = (lambda i: params[i]) if "bias_unrounded" in df else (lambda i: rf(params[i], on))
    tanh = "gelu_tanh" in df
    s = {}
    s["patches"] = fo(st_patches(images, on), "patches")
    s["pre_tok"] = s["patches"] @ wm(2).t() + bias(3)
    tok = rf(rb(s["pre_tok"], on), on).view(N, T - 1, C)
    pos = params[1].view(T, C)
    x = torch.cat([params[0].view(1, 1, C).expand(N, 1, C), tok], 1) + pos
    x = x.reshape(N * T, C)
    for i in range(depth):
        p, b = f"b{i}.", 4 + 12 * i
        x = s[p + "xin"] = fo(x, p + "xin")
        s[p + "st1"] = st_stats(x.detach(), eps)
        s[p + "xn1"] = fo(rf(st_ln(x, params[b], params[b + 1], eps), on), p + "xn1")
        s[p + "pre_qkv"] = rb(s[p + "xn1"], on) @ wm(b + 2).t() + bias(b + 3)
        qkv = rf(rb(s[p + "pre_qkv"], on), on)
        q, k, v = (fo(split_heads(qkv[:, j * C:(j + 1) * C], N, T), p + n) for j, n in enumerate("qkv"))
        s[p + "q"], s[p + "k"], s[p + "v"] = q, k, v
        node, o_saved, s[p + "lse"] = attention(q, k, v, on, forced, p, df)
        s[p + "pre_o"] = node
        o = merge_heads(node)
        s[p + "o"] = o + (o_saved - o).detach()
        s[p + "pre_proj"] = rb(s[p + "o"], on) @ wm(b + 4).t() + bias(b + 5)
        x = s[p + "xmid"] = fo(x + rf(rb(s[p + "pre_proj"], on), on), p + "xmid")
        s[p + "st2"] = st_stats(x.detach(), eps)
        s[p + "xn2"] = fo(rf(st_ln(x, params[b + 6], params[b + 7], eps), on), p + "xn2")
        s[p + "pre_h"] = rb(s[p + "xn2"], on) @ wm(b + 8).t() + bias(b + 9)
        s[p + "h"] = fo(rf(rb(s[p + "pre_h"], on), on), p + "h")
        s[p + "g"] = rf(gelu(s[p + "h"], tanh), on)
        s[p + "pre_fc2"] = rb(s[p + "g"], on) @ wm(b + 10).t() + bias(b + 11)
        x = x + rf(rb(s[p + "pre_fc2"], on), on)
    x = s["xfin"] = fo(x, "xfin")
    s["stf"] = st_stats(x.detach(), eps)
    b = 4 + 12 * depth
    s["out"] = st_ln(x, params[b], params[b + 1], eps).view(N, T, C)[:, 1:]
    return s


def backward(images, values, geo, gout, eps=1e-6, on=True, forced=None, defects=()):
    """-> (stages, [gradient of every parameter, lara_vit.h order]) for dL/d(out) = gout [N, hw, C]"""
    params = make_params(values)
    s = forward(images, params, geo, eps, on, forced, defects)
    (s["out"] * gout.double()).sum().backward()
    return {k: v.detach() for k, v in s.items()}, [p.grad.clone() for p in params]


def device_layout(s, geo, defects=()):
    """The stages of `forward` in the layout of `save` (include/lara_vit.h): xn1, o, xn2, h padded to Mp rows, q, k, v to Tp tokens,
    patches to Pp rows, lse to Tp entries (those t >= T are not written on the device: NaN here)."""
    out = {}
    M, Mp, T, Tp = geo["M"], geo["Mp"], geo["T"], geo["Tp"]
    for k, v in s.items():
        v = v.detach()
        name = k.split(".")[-1]
        if name in ("xn1", "o", "xn2", "h"):
            v = F.pad(v, (0, 0, 0, Mp - M))
            if "padded_row" in defects and Mp > M:
                v[M] = 1.0
        elif name in ("q", "k", "v"):
            v = F.pad(v, (0, 0, 0, Tp - T)).reshape(geo["NH"], Tp, HD)
        elif name == "lse":
            v = F.pad(v, (0, Tp - T), value=float("nan")).reshape(geo["NH"], Tp)
        elif name == "patches":
            v = F.pad(v, (0, 0, 0, geo["Pp"] - geo["NP"]))
        out[k] = v
    return out
