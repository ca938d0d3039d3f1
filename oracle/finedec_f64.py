"""fp64 reference of the fine decoder's seven entry points (include/lara_finedec.h) -- TEST INFRASTRUCTURE ONLY
(the checker of tests/test_finedec_f64.py and tests/test_finedec_f64_gpu.py; nothing under lara_amd/ imports it).

It restates, in torch fp64 on the CPU, the folded algebra the header documents,
    t = Wqk xn,   s[h, j] = t[h] . pf[j],   P = softmax_j(s),   u[h] = sum_j P[h, j] pf[j],
    hid = relu(W1ov u + b1),   sh = W2 hid + b2,
the chain back (DH, du, the 4-way softmax's backward, DT, d_pf, d_xn), the five weight gradients, and the LayerNorm in front
with its `stats` and per-block `partials`.  It reads nothing of the code under test.  Of the device it assumes only what the
header states: fp32 arithmetic, 512-row slabs with an ordered sum for the weight gradients, `partials` per 256-row block.

Every function returns, beside each value X, the fp32 error bound "A_X" of every element of X, from the reference's own
operands.  The rules, all first order (the acceptance test's factor 4 absorbs the rest):
    a sum or product of K terms        K 2^-24 sum|terms|  (any order, fused or not; a term that is exactly zero costs nothing)
    one operation                      2^-24 |result|
    a softmax weight P                 relative 4 A_s + 2^-23 |s - max| + 16 * 2^-24 (both exponentials' arguments, v_exp_f32,
                                       the four-term sum, the reciprocal and the product: the bound tests/
                                       test_voltrans_stages_gpu.py uses for the same sequence; A_s is the largest score bound
                                       of the head, since the normaliser mixes all four), plus an absolute 2^-126 for terms
                                       that flush to zero
    1 / sqrt(v)                        relative A_v / (2 v) + 4 * 2^-24 (square root and quotient to one ulp each)
    a weight gradient                  K = 512 + the number of slabs: any order that sums inside slabs first, across them second
    a `partials` entry                 K = 256
and through a formula f(a, b, ..) the bounds of the operands propagate with |df/da| A_a + ...

Teacher forcing.  `fine_decoder_backward(.., forced={"U": .., "HID": .., "DH": .., "DT": ..})` takes the arrays a device (or
any other evaluation under test) handed out and restarts the chain from them, with no inherited bound: HID from the forced U,
DH under the mask HID_forced > 0, du from the forced DH, d_xn from the forced DT.  Scores, P, U, and what follows du (DT, d_pf)
have nothing handed out in front of them: their bounds are propagated.  `fine_decoder_wgrad` and `fine_ln_backward` are
forced by construction (their operands are their arguments).

The acceptance test the tests apply to every element: |got - ref| <= 4 A + 2^-23 |ref|  (`ratio`).
"""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
FD, NH, CD, NV, HID, SH, TQ = 80, 8, 8, 4, 64, 12, 64
SLAB, LN_ROWS = 512, 256
WGRAD_PARTS = (("dWqk", (TQ, FD)), ("dW1ov", (HID, TQ)), ("db1", (HID,)), ("dW2", (SH, HID)), ("db2", (SH,)))


def f64(x):
    return torch.as_tensor(x).detach().to("cpu", torch.float64)


def limit(ref, A):
    return 4 * A + 2.0 ** -23 * ref.abs()


def ratio(got, ref, A):
    """|got - ref| / (4 A + 2^-23 |ref|) per element; an element with A = 0 and ref = 0 must be exactly 0 (else inf)"""
    d = (f64(got) - ref).abs()
    lim = limit(ref, A)
    r = torch.where(lim > 0, d / lim, torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return torch.where(torch.isfinite(f64(got)), r, torch.full_like(r, float("inf")))


def _mm(a, b, K):
    """a @ b and K 2^-24 |a| @ |b|"""
    return a @ b, K * U * (a.abs() @ b.abs())


def fine_wgrad_floats():
    return sum(torch.Size(s).numel() for _, s in WGRAD_PARTS)


def fine_ln_blocks(n):
    return 0 if n <= 0 else (n + LN_ROWS - 1) // LN_ROWS


def fine_wgrad_slabs(n):
    return 0 if n <= 0 else (n + SLAB - 1) // SLAB


# ---------------------------------------------------------------------------------------------- the decoder

def fine_decoder_attention(xn, pf, Wqk):
    """xn [n, 80], pf [4, 8, n] -> t [n, 8, 8], s, gap = max - s, P [n, 8, 4], U [n, 64], each with its bound"""
    xn, pf, Wqk = f64(xn), f64(pf), f64(Wqk)
    n = xn.shape[0]
    t, A_t = _mm(xn, Wqk.t(), FD)
    t, A_t = t.view(n, NH, CD), A_t.view(n, NH, CD)
    v = pf.permute(2, 0, 1)                                             # [n, view, c]
    s = torch.einsum("nhc,njc->nhj", t, v)
    A_s = torch.einsum("nhc,njc->nhj", A_t, v.abs()) + CD * U * torch.einsum("nhc,njc->nhj", t.abs(), v.abs())
    gap = s.max(-1, keepdim=True).values - s
    e = torch.exp(-gap)
    P = e / e.sum(-1, keepdim=True)
    rel_P = 4 * A_s.max(-1, keepdim=True).values + 2 * U * gap + 16 * U
    A_P = P * rel_P + TINY
    u = torch.einsum("nhj,njc->nhc", P, v)
    A_u = torch.einsum("nhj,njc->nhc", A_P, v.abs()) + NV * U * torch.einsum("nhj,njc->nhc", P, v.abs())
    return {"t": t, "A_t": A_t, "s": s, "A_s": A_s, "gap": gap, "P": P, "A_P": A_P, "U": u.reshape(n, TQ), "A_U": A_u.reshape(n, TQ)}


def fine_decoder_forward(xn, pf, Wqk, W1ov, b1, W2, b2, att=None, U_forced=None):
    """-> the attention's dict plus PRE (W1ov u + b1), HID, sh and their bounds.  `att`: a (possibly altered) result of
    `fine_decoder_attention`; `U_forced`: u as handed out by the evaluation under test (PRE, HID and sh then carry no bound
    inherited from u)."""
    W1ov, b1, W2, b2 = f64(W1ov), f64(b1), f64(W2), f64(b2)
    r = dict(fine_decoder_attention(xn, pf, Wqk) if att is None else att)
    u, A_u = (r["U"], r["A_U"]) if U_forced is None else (f64(U_forced), torch.zeros_like(r["U"]))
    pre, A_sum = _mm(u, W1ov.t(), TQ + 1)
    pre = pre + b1
    A_pre = A_u @ W1ov.abs().t() + A_sum + (TQ + 1) * U * b1.abs()
    on = pre > 0
    hid, A_hid = torch.where(on, pre, torch.zeros_like(pre)), A_pre * on
    # sh: the terms of dead units are exactly zero and cost nothing; a point with every unit dead has sh = b2 exactly
    k = on.sum(-1, keepdim=True)
    sh = hid @ W2.t() + b2
    A_sh = A_hid @ W2.abs().t() + torch.where(k > 0, k + 1, k) * U * (hid @ W2.abs().t() + b2.abs())
    r.update(PRE=pre, A_PRE=A_pre, HID=hid, A_HID=A_hid, sh=sh, A_sh=A_sh)
    return r


def fine_decoder_backward(xn, pf, Wqk, W1ov, b1, W2, b2, d_sh, att=None, forced=None):
    """-> {"U", "HID", "DH", "DT", "d_xn", "d_pf", "sh"} and "A_" + each.  `forced`: see the module docstring."""
    forced = forced or {}
    Wqk_, W1ov_, W2_, d_sh = f64(Wqk), f64(W1ov), f64(W2), f64(d_sh)
    a = fine_decoder_forward(xn, pf, Wqk, W1ov, b1, W2, b2, att=att)
    n = a["U"].shape[0]
    r = {k: a[k] for k in ("U", "A_U", "sh", "A_sh")}
    if "U" in forced:
        f = fine_decoder_forward(xn, pf, Wqk, W1ov, b1, W2, b2, att=a, U_forced=forced["U"])
        r.update(HID=f["HID"], A_HID=f["A_HID"])
    else:
        r.update(HID=a["HID"], A_HID=a["A_HID"])
    on = (f64(forced["HID"]) > 0) if "HID" in forced else (r["HID"] > 0)
    dh, A_dh = _mm(d_sh, W2_, SH)
    r.update(DH=dh * on, A_DH=A_dh * on)
    dh_in, A_in = (f64(forced["DH"]), torch.zeros_like(dh)) if "DH" in forced else (r["DH"], r["A_DH"])
    du, A_du = _mm(dh_in, W1ov_, HID)
    du, A_du = du.view(n, NH, CD), (A_du + A_in @ W1ov_.abs()).view(n, NH, CD)
    # the 4-way softmax's backward, per head: dp[j] = du . pf[j], dot = sum_j P[j] dp[j], ds[j] = P[j] (dp[j] - dot)
    v = f64(pf).permute(2, 0, 1)
    va = v.abs()
    t, A_t, P, A_P = a["t"], a["A_t"], a["P"], a["A_P"]
    dp = torch.einsum("nhc,njc->nhj", du, v)
    A_dp = torch.einsum("nhc,njc->nhj", A_du, va) + CD * U * torch.einsum("nhc,njc->nhj", du.abs(), va)
    dot = (P * dp).sum(-1, keepdim=True)
    A_dot = (A_P * dp.abs() + P * A_dp).sum(-1, keepdim=True) + NV * U * (P * dp.abs()).sum(-1, keepdim=True)
    diff = dp - dot
    A_diff = A_dp + A_dot + U * (dp.abs() + dot.abs())
    ds = P * diff
    A_ds = A_P * diff.abs() + P * A_diff + U * ds.abs()
    dt = torch.einsum("nhj,njc->nhc", ds, v)
    A_dt = torch.einsum("nhj,njc->nhc", A_ds, va) + NV * U * torch.einsum("nhj,njc->nhc", ds.abs(), va)
    # d_pf[j, c] = sum_h (P[h, j] du[h, c] + ds[h, j] t[h, c]): 16 terms
    dpf = torch.einsum("nhj,nhc->njc", P, du) + torch.einsum("nhj,nhc->njc", ds, t)
    A_dpf = (torch.einsum("nhj,nhc->njc", A_P, du.abs()) + torch.einsum("nhj,nhc->njc", P, A_du)
             + torch.einsum("nhj,nhc->njc", A_ds, t.abs()) + torch.einsum("nhj,nhc->njc", ds.abs(), A_t)
             + 2 * NH * U * (torch.einsum("nhj,nhc->njc", P, du.abs()) + torch.einsum("nhj,nhc->njc", ds.abs(), t.abs())))
    r.update(DT=dt.reshape(n, TQ), A_DT=A_dt.reshape(n, TQ), d_pf=dpf.permute(1, 2, 0), A_d_pf=A_dpf.permute(1, 2, 0))
    dt_in, A_in = (f64(forced["DT"]), torch.zeros_like(r["DT"])) if "DT" in forced else (r["DT"], r["A_DT"])
    dxn, A_dxn = _mm(dt_in, Wqk_, TQ)
    r.update(d_xn=dxn, A_d_xn=A_dxn + A_in @ Wqk_.abs())
    return r


def fine_decoder_wgrad(n, xn, Um, HIDm, DH, DT, d_sh):
    """-> (out, A) as the flat [dWqk | dW1ov | db1 | dW2 | db2] of the header, from the factor arrays as given"""
    xn, Um, HIDm, DH, DT, d_sh = (f64(x)[:n] for x in (xn, Um, HIDm, DH, DT, d_sh))
    K = SLAB + fine_wgrad_slabs(n)
    ones = torch.ones(n, 1, dtype=torch.float64)
    parts = [_mm(DT.t(), xn, K), _mm(DH.t(), Um, K), _mm(DH.t(), ones, K), _mm(d_sh.t(), HIDm, K), _mm(d_sh.t(), ones, K)]
    return torch.cat([p.reshape(-1) for p, _ in parts]), torch.cat([A.reshape(-1) for _, A in parts])


def split_wgrad(flat):
    out, o = {}, 0
    for name, shape in WGRAD_PARTS:
        k = torch.Size(shape).numel()
        out[name] = flat[o:o + k].view(shape)
        o += k
    return out


# ---------------------------------------------------------------------------------------------- the LayerNorm

def fine_ln_forward(x, gamma, beta, eps, stats_forced=None):
    """x [n, 80] -> {"xn", "stats" [n, 2] = (mean, rstd)} and their bounds; `eps` is the fp32 number the device gets.
    `stats_forced`: xn from the stats as handed out (three operations per element, nothing inherited)."""
    x, gamma, beta, eps = f64(x), f64(gamma), f64(beta), float(eps)
    if stats_forced is not None:
        st = f64(stats_forced)
        c = x - st[:, :1]
        xh = c * st[:, 1:]
        y = xh * gamma
        return {"xn": y + beta, "A_xn": gamma.abs() * 2 * U * xh.abs() + U * y.abs() + U * (y + beta).abs() * (y != 0)}
    mean = x.mean(-1, keepdim=True)
    A_mean = U * x.abs().sum(-1, keepdim=True) + 2 * U * mean.abs()              # 80 terms, then the constant 1/80 and its product
    c = x - mean
    A_c = A_mean + U * c.abs()
    vs = (c * c).sum(-1, keepdim=True)
    A_vs = (2 * c.abs() * A_c).sum(-1, keepdim=True) + (FD + 1) * U * vs
    v = vs / FD + eps
    A_v = A_vs / FD + 2 * U * vs / FD + U * v
    rstd = v.rsqrt()
    rel = A_v / (2 * v) + 4 * U
    xh = c * rstd
    A_xh = A_c * rstd + xh.abs() * (rel + U)
    y = xh * gamma
    A_y = gamma.abs() * A_xh + U * y.abs()
    xn = y + beta
    return {"xn": xn, "A_xn": A_y + U * xn.abs() * (y != 0), "stats": torch.cat([mean, rstd], 1),
            "A_stats": torch.cat([A_mean, rstd * rel], 1)}


def fine_ln_backward(x, gamma, stats, d_xn):
    """-> {"d_x", "partials" [blocks, 160], "d_gamma", "d_beta"} and their bounds, from the stats as given"""
    x, gamma, st, g0 = f64(x), f64(gamma), f64(stats), f64(d_xn)
    n = x.shape[0]
    mean, rstd = st[:, :1], st[:, 1:]
    xh = (x - mean) * rstd
    A_xh = 2 * U * xh.abs()
    g = g0 * gamma
    A_g = U * g.abs()
    m1 = g.mean(-1, keepdim=True)
    A_m1 = (A_g.sum(-1, keepdim=True) + FD * U * g.abs().sum(-1, keepdim=True)) / FD + 2 * U * m1.abs()
    tt = g * xh
    A_tt = A_g * xh.abs() + g.abs() * A_xh + U * tt.abs()
    m2 = tt.mean(-1, keepdim=True)
    A_m2 = (A_tt.sum(-1, keepdim=True) + FD * U * tt.abs().sum(-1, keepdim=True)) / FD + 2 * U * m2.abs()
    inner = g - m1 - xh * m2
    A_inner = A_g + A_m1 + A_xh * m2.abs() + xh.abs() * A_m2 + 3 * U * (g.abs() + m1.abs() + (xh * m2).abs())
    dx = rstd * inner
    A_dx = rstd * A_inner + U * dx.abs()
    blocks = fine_ln_blocks(n)
    pad = blocks * LN_ROWS - n
    rows = lambda a: torch.cat([a, a.new_zeros(pad, FD)]).view(blocks, LN_ROWS, FD)
    pg = g0 * xh
    A_pg = g0.abs() * A_xh + U * pg.abs()
    partials = torch.cat([rows(pg).sum(1), rows(g0).sum(1)], 1)
    A_part = torch.cat([rows(A_pg).sum(1) + LN_ROWS * U * rows(pg.abs()).sum(1), LN_ROWS * U * rows(g0.abs()).sum(1)], 1)
    tot, A_tot = partials.sum(0), A_part.sum(0)
    return {"d_x": dx, "A_d_x": A_dx, "partials": partials, "A_partials": A_part, "d_gamma": tot[:FD], "A_d_gamma": A_tot[:FD],
            "d_beta": tot[FD:], "A_d_beta": A_tot[FD:]}
