"""bf16-faithful fp64 reference of one GroupAttBlock and of the VolTransformer head -- TEST INFRASTRUCTURE ONLY
(the checker of tests/test_voltrans_stages_gpu.py; nothing under lara_amd/ imports it).

It restates, in torch fp64 on the CPU, what lara_groupblock_forward_train / lara_groupblock_backward and
lara_voltrans_head_forward / _backward compute, and rounds to bf16 exactly where the kernels do.  Against it a kernel's
error is fp32 accumulation order plus the occasional rounding flip, not the bf16 noise the end-to-end bars have to allow.
It works on the group-major token rows of include/lara_groupattn.h and on the module dictionaries of
oracle/voltrans_ref.py (`build_modules`).

Two markers carry the roundings (both take `on`; with on=False the same code is the plain fp64 restatement):
    rf(x)  rounds x to bf16 (nearest even) in the forward, passes the gradient straight through
    rb(x)  identity in the forward, rounds the gradient to bf16 in the backward
so autograd through `block` / `head` IS the faithful backward.  Two places need more than a marker, because the device's
backward does not use the value its forward used (AttnPV, GeluFn below).

Where the device rounds to bf16 (read off encoder_bwd.hip, group_attn.h, mlp_fused.h, mfma_gemm.h):

forward (block_forward_keep + the convolution launch)
    cond, wq, wkv, wo, w1, w2, wconv, wdeconv   cast once on the host; the kernels only ever see bf16
    xn1   = bf16(norm1(x_in))                    group_attn_fused2_kernel step 1 (fp32 LayerNorm, two-pass moments)
    kv    = bf16(cond . wkv^T)                   gemm_ring_kernel / gemm_ring2_kernel, EPI 0
    q     = bf16(xn1 . wq^T)                     group_attn_fused2_kernel step 2
    P     = bf16(softmax(q k^T / 4))             step 3: the normalised probabilities are the bf16 A operand of P.V
                                                 (scores, max, exp, sum, 1/sum in fp32; P is not saved)
    o     = bf16(P . v)                          step 3
    x1    = x_in + o . wo^T                      fp32
    xn2   = bf16(norm2(x1))                      mlp_fused.h
    z     = bf16(xn2 . w1^T + b1)                mlp_fused.h; the saved pre-activation
    h     = bf16(gelu(xn2 . w1^T + b1))          GELU of the fp32 (unrounded) pre-activation, not of z
    x2    = x1 + h . w2^T + b2                   fp32
    xn3   = bf16(norm3(x2)); stats = (mean, rstd) of x2's rows, fp32; row M of xn3 is zero
    x_out = norm3(x2) [fp32, redone from stats] + conv3x3x3(xn3)        EPI 4: the residual is NOT the rounded xn3

backward (lara_groupblock_backward; g = dL/dx_out on entry, dL/dx_in on exit, fp32 throughout)
    gb    = bf16(g)                              cast_bf16_kernel, or the bf16 copy the block before left (chained)
    dwconv += gb^T . gather(xn3)                 fp32 accumulation
    dpn   = g + convT(gb)                        fp32: only the convolution's output gradient is rounded
    g     = dnorm3(dpn; x2, stats)               fp32; dln3_w, dln3_b from dpn, db2 from the fp32 g (EPI 9 / ln_bwd_kernel)
    gb3   = bf16(g)                              the operand of dW2 and of the MLP's dX products
    dzb   = bf16((gb3 . w2) * gelu'(z))          gelu' at the SAVED bf16 z; db1 = column sums of the stored bf16 dzb
    tmpb  = bf16(dzb . w1)                       the bf16 gradient norm2's backward receives
    g     = g + dnorm2(tmpb; x1); gb2 = bf16(g)  dln2_w, dln2_b from tmpb
    dob   = bf16(gb2 . wo)
    dq    = bf16(..), dkv = bf16(..)             group_attn_bwd_kernel: P recomputed in fp32 and NOT rounded (dV = P^T dO and
                                                 dS = P (dP - sum P dP) / 4 use the fp32 P, where the forward multiplied bf16(P))
    dcond += dkv . wkv                           fp32 (or dkv handed to the caller, who runs one product for all layers)
    tmpb  = bf16(dq . wq)
    g     = g + dnorm1(tmpb; x_in); gb = bf16(g) dln1_w, dln1_b from tmpb; gb is what a chained next call gathers
    dw2 += gb3^T h, dw1 += dzb^T xn2, dwo += gb2^T o, dwq += dq^T xn1, dwkv += dkv^T cond      fp32 accumulation

head (lara_voltrans_head_forward / _backward)
    xn    = bf16(norm(x));  out = xn . wdeconv^T + bias, fp32, scattered to channels-last [B, 2R, 2R, 2R, Cout]
    dog   = bf16(dout) gathered into GEMM rows [M, 8 Cout]; d_bias8 = column sums of the bf16 dog (per tap)
    d_wdeconv += dog^T xn;  tmp = bf16(dog . wdeconv_t);  g = dnorm(tmp; x) fp32;  d_ln_w, d_ln_b from tmp
"""
import torch
import torch.nn.functional as F

E, HEADS = 256, 16


# ---------------------------------------------------------------------------------------------- the two markers

def round_bf16(x):
    """Nearest-even bf16 rounding of the fp32 value of x, by integer arithmetic on the fp32 bits (NaN stays NaN, values
    beyond the bf16 maximum's rounding boundary become inf, subnormals round like everything else); result in x's dtype."""
    f = x.detach().to(torch.float32).contiguous()
    u = f.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000)
    r = torch.where(torch.isnan(f), u | 0x00400000, r) & 0xFFFF0000
    r = torch.where(r >= 0x80000000, r - 0x100000000, r).to(torch.int32)
    return r.view(torch.float32).to(x.dtype)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return round_bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return round_bf16(g)


def rf(x, on=True):
    return _RoundFwd.apply(x) if on else x


def rb(x, on=True):
    return _RoundBwd.apply(x) if on else x


def _force(x, forced, name):
    """Teacher forcing: the value becomes the device's saved one, the gradient flows as if it were x."""
    if forced is None or name not in forced:
        return x
    return x + (forced[name].to(x.dtype) - x).detach()


class AttnPV(torch.autograd.Function):
    """o = bf16(P) . v in the forward; the backward uses the unrounded P for dV (and the softmax backward behind it gets the
    unrounded P as well), as group_attn_bwd_kernel does."""
    @staticmethod
    def forward(ctx, p, v, on):
        ctx.save_for_backward(p, v)
        return (round_bf16(p) if on else p) @ v

    @staticmethod
    def backward(ctx, g):
        p, v = ctx.saved_tensors
        return g @ v.transpose(-1, -2), p.transpose(-1, -2) @ g, None


class GeluFn(torch.autograd.Function):
    """gelu (erf) of the unrounded pre-activation; the backward evaluates gelu' at z_saved (the bf16 z the forward kept)."""
    @staticmethod
    def forward(ctx, zpre, z_saved):
        ctx.save_for_backward(z_saved)
        return F.gelu(zpre)

    @staticmethod
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        cdf = 0.5 * (1.0 + torch.erf(z * 0.7071067811865476))
        pdf = torch.exp(-0.5 * z * z) * 0.3989422804014327
        return g * (cdf + z * pdf), None


# ---------------------------------------------------------------------------------------------- layouts

def rows_to_volume(rows, B, R):
    """group-major token rows [B R^3, C] -> [B, C, R, R, R]"""
    g = R // 2
    return rows.view(B, g, g, g, 2, 2, 2, -1).permute(0, 7, 1, 4, 2, 5, 3, 6).reshape(B, -1, R, R, R)


def volume_to_rows(vol):
    B, C, R = vol.shape[:3]
    g = R // 2
    return vol.view(B, C, g, 2, g, 2, g, 2).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B * R ** 3, C)


def block_weights(blk, cond_dim=None, on=True, requires_grad=True):
    """The operands of lara_groupblock_weights as fp64 leaves: matrices rounded to bf16 when `on`.  cond_dim < 800 keeps the
    first cond_dim input columns of the K and V projections (rescaled to the same output variance)."""
    mha = blk["mha"]
    wk, wv = mha.k_proj_weight.detach(), mha.v_proj_weight.detach()
    if cond_dim is not None and cond_dim != wk.shape[1]:
        s = (wk.shape[1] / cond_dim) ** 0.5
        wk, wv = wk[:, :cond_dim] * s, wv[:, :cond_dim] * s
    w = {"ln1_w": blk["norm1"].weight, "ln1_b": blk["norm1"].bias, "wq": mha.q_proj_weight, "wkv": torch.cat([wk, wv], 0),
         "wo": mha.out_proj.weight, "ln2_w": blk["norm2"].weight, "ln2_b": blk["norm2"].bias, "w1": blk["mlp"][0].weight,
         "b1": blk["mlp"][0].bias, "w2": blk["mlp"][3].weight, "b2": blk["mlp"][3].bias, "ln3_w": blk["norm3"].weight,
         "ln3_b": blk["norm3"].bias, "wconv": blk["cnn"].weight}
    out = {}
    for k, v in w.items():
        v = v.detach().to(torch.float32)
        if on and k in ("wq", "wkv", "wo", "w1", "w2", "wconv"):
            v = round_bf16(v)
        out[k] = v.double().clone().requires_grad_(requires_grad)
    out["eps"] = float(blk["norm1"].eps)
    return out


# ---------------------------------------------------------------------------------------------- forward stages (unrounded outputs)

def st_ln(x, w, b, eps):
    return F.layer_norm(x, (E,), w, b, eps)


def st_stats(x, eps):
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], -1)


def st_kv(cond, wkv):
    return cond @ wkv.t()


def st_q(xn1, wq):
    return xn1 @ wq.t()


def attn_probs(q, kv):
    """q [M, 256], kv [M/2, 512] -> (P [G, 16, 8, 4], scores [G, 16, 8, 4], v [G, 16, 4, 16])"""
    G = q.shape[0] // 8
    qh = q.view(G, 8, HEADS, 16).transpose(1, 2)
    kh = kv[:, :E].reshape(G, 4, HEADS, 16).transpose(1, 2)
    vh = kv[:, E:].reshape(G, 4, HEADS, 16).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * 0.25
    return torch.softmax(s, -1), s, vh


def st_o(q, kv, on=True):
    p, _, vh = attn_probs(q, kv)
    return AttnPV.apply(p, vh, on).transpose(1, 2).reshape(q.shape[0], E)


def st_x1(o, x_in, wo):
    return x_in + o @ wo.t()


def st_z(xn2, w1, b1):
    return xn2 @ w1.t() + b1


def st_x2(h, x1, w2, b2):
    return x1 + h @ w2.t() + b2


def st_conv(xn3, wconv, B, R):
    return volume_to_rows(F.conv3d(rows_to_volume(xn3, B, R), wconv, padding=1))


def st_xout(xn3, x2, w, B, R):
    return st_ln(x2, w["ln3_w"], w["ln3_b"], w["eps"]) + st_conv(xn3, w["wconv"], B, R)


# ---------------------------------------------------------------------------------------------- the block and the head

def block(x_in, cond, w, B, R, on=True, forced=None):
    """x_in [B R^3, 256], cond [B (R/2)^3 * 4, cond_dim] (fp64; cond holds bf16 values when `on`).  Returns every stage
    (the rounded values, as the device saves them) and x_out; autograd through it is the device's backward.  `forced`:
    device values that replace stages in the forward (the gradient is then evaluated on the device's own activations)."""
    s, eps = {}, w["eps"]
    fo = lambda t, n: _force(t, forced, n)
    s["xn1"] = fo(rf(st_ln(x_in, w["ln1_w"], w["ln1_b"], eps), on), "xn1")
    s["kv_pre"] = st_kv(cond, w["wkv"])
    s["kv"] = fo(rf(rb(s["kv_pre"], on), on), "kv")
    # (the pre_* tensors are the products in front of a gradient rounding: after a backward their .grad, if retained, is the
    # device's bf16 scratch stage -- dq, dob, gb2, dzb, gb3 of bwd_layout())
    s["pre_q"] = st_q(rb(s["xn1"], on), w["wq"])
    s["q"] = fo(rf(rb(s["pre_q"], on), on), "q")
    s["pre_o"] = st_o(s["q"], s["kv"], on)
    s["o"] = fo(rf(rb(s["pre_o"], on), on), "o")
    s["pre_wo"] = s["o"] @ w["wo"].t()
    s["x1"] = fo(x_in + rb(s["pre_wo"], on), "x1")
    s["xn2"] = fo(rf(st_ln(s["x1"], w["ln2_w"], w["ln2_b"], eps), on), "xn2")
    s["pre_z"] = st_z(rb(s["xn2"], on), w["w1"], w["b1"])
    zpre = rb(s["pre_z"], on)
    s["z"] = fo(rf(zpre, on), "z")
    s["h"] = fo(rf(GeluFn.apply(zpre, s["z"].detach()), on), "h")
    s["pre_w2"] = s["h"] @ w["w2"].t()
    s["x2"] = fo(s["x1"] + rb(s["pre_w2"], on) + w["b2"], "x2")
    pn = st_ln(s["x2"], w["ln3_w"], w["ln3_b"], eps)
    s["xn3"] = fo(rf(pn, on), "xn3")
    s["stats"] = st_stats(s["x2"].detach(), eps)
    s["x_out"] = pn + rb(st_conv(s["xn3"], w["wconv"], B, R), on)
    return s


BLOCK_GRADS = ("ln1_w", "ln1_b", "wq", "wkv", "wo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2", "ln3_w", "ln3_b", "wconv")


def block_backward(x_in, cond, w, B, R, g_out, on=True, forced=None, scratch_stages=False):
    """-> dict: 'g' (dL/dx_in), 'dcond', 'dkv' (the gradient at K|V as the attention backward leaves it) and the fourteen
    parameter gradients, wconv in the device's [256][27][256] layout; scratch_stages: also the backward's bf16 scratch stages
    gb3, dzb, gb2, dob, dq."""
    x = x_in.detach().clone().requires_grad_(True)
    c = cond.detach().clone().requires_grad_(True)
    for k in BLOCK_GRADS:
        w[k].grad = None
    s = block(x, c, w, B, R, on, forced)
    scratch = {"dq": "pre_q", "dob": "pre_o", "gb2": "pre_wo", "dzb": "pre_z", "gb3": "pre_w2"}
    for name in ("kv_pre",) + tuple(scratch.values()):
        s[name].retain_grad()
    (s["x_out"] * g_out).sum().backward()
    out = {"g": x.grad, "dcond": c.grad, "dkv": s["kv_pre"].grad}
    if scratch_stages:
        out.update({k: s[v].grad for k, v in scratch.items()})
    for k in BLOCK_GRADS:
        out[k] = w[k].grad.clone()
    out["wconv"] = out["wconv"].permute(0, 2, 3, 4, 1).reshape(E, 27, E)
    return out


def head_weights(m, Cout, on=True):
    """norm / deconv of `build_modules` (the first Cout output channels) as fp64 leaves; wd is [8 Cout, 256] with row
    tap * Cout + co, tap = (i*2 + j)*2 + k; bias8 the bias repeated per tap."""
    wd = m["deconv"].weight.detach()[:, :Cout].permute(2, 3, 4, 1, 0).reshape(8 * Cout, E).to(torch.float32)
    if on:
        wd = round_bf16(wd)
    lf = lambda t: t.detach().double().clone().requires_grad_(True)
    return {"ln_w": lf(m["norm"].weight), "ln_b": lf(m["norm"].bias), "wd": lf(wd),
            "bias8": lf(m["deconv"].bias.detach()[:Cout].repeat(8)), "eps": float(m["norm"].eps)}


def head_rows_to_out(rows, B, R, Cout):
    """GEMM rows [M, 8 Cout] (group-major tokens) -> channels-last [B, 2R, 2R, 2R, Cout]"""
    g = R // 2
    v = rows.view(B, g, g, g, 2, 2, 2, 2, 2, 2, Cout)               # b gd gh gw z y x i j k c
    return v.permute(0, 1, 4, 7, 2, 5, 8, 3, 6, 9, 10).reshape(B, 2 * R, 2 * R, 2 * R, Cout)


def head(x, hw, B, R, on=True, forced=None):
    Cout = hw["wd"].shape[0] // 8
    xn = _force(rf(st_ln(x, hw["ln_w"], hw["ln_b"], hw["eps"]), on), forced, "xn")
    rows = rb(rb(xn, on) @ hw["wd"].t() + hw["bias8"], on)
    return head_rows_to_out(rows, B, R, Cout)


HEAD_GRADS = ("ln_w", "ln_b", "wd", "bias8")


def head_backward(x_in, hw, B, R, dout, on=True, forced=None):
    x = x_in.detach().clone().requires_grad_(True)
    for k in HEAD_GRADS:
        hw[k].grad = None
    (head(x, hw, B, R, on, forced) * dout).sum().backward()
    out = {"g": x.grad}
    for k in HEAD_GRADS:
        out[k] = hw[k].grad.clone()
    return out
