"""Cases, seeded inputs, cached references and the stage checks shared by tests/test_vit_bf16.py (CPU: the reference against
itself and against the defects built into it) and tests/test_vit_stages_gpu.py (the device against the reference).

The stage checks take `got`, the stages in the layout of `save` (oracle.vit_bf16.device_layout / the device's own buffers), and
recompute every stage in fp64 from GOT's inputs of that stage (teacher forcing), so a deviation is charged to the stage that made
it.  Limits, for every element (no exemptions):
    bf16 stages   |got - ref| <= ulp_bf16(ref) + A           fp32 stages   |got - ref| <= 4 A + 2^-23 |ref|
    a residual    x + bf16(pre):  |got - (x + pre)| <= ulp_bf16(pre) + A + 2^-23 (|x| + |pre|)
with ref the unrounded fp64 value and A the fp32 accumulation bound K 2^-24 (|a| . |b|) of the stage's product (plus 2^-24 of the
bias and of the sum), or the C-term bound on both moments for a LayerNorm.  Named extra terms:
  o      P~ = bf16(exp(s - m_j)) is rounded on the device but not saved.  The device's fp32 exponential differs from the fp64 one
         by at most p_rel = 4 max A_s + 2 * 2^-24 |s - m_j| + 16 * 2^-24 relative (the score's and the running maximum's
         accumulation error A_s = 64 * 2^-24 |q| . |k| / 8 + 2^-24 |s|, the argument's scaling by log2 e, v_exp_f32); where the fp64
         value lies within that of a rounding tie the device may round the other way: A gains ulp_bf16(P~) w_j |v| / l for those.
         The rest of A: ((Tp + 8) 2^-24 + 2 max p_rel) (P~ w . |v|) / l for the accumulation, the rescaling factors and l.
  lse    A = max A_s + 4 * 2^-24 (|m| + |log l| + 1) + Tp 2^-24.
  xout   g = bf16(gelu(h)) is not saved: the reference takes h from `got`; where gelu(h) lies within erff's error
         (0.5 |h| 4 * 2^-24 for erf's absolute error, + 4 * 2^-24 |gelu|) of a tie, A gains ulp_bf16(g) |W2|.
Padded rows (xn1, o, xn2, h: rows >= M; patches: rows >= NP) and padded tokens (q, k, v: t >= T) must be exactly zero.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import vit_bf16 as vr
from oracle.voltrans_bf16 import round_bf16

U = 2.0 ** -24
EPS = 1e-6
# (N, views, H, W, C, F, depth)
CASES = [(1, 1, 16, 16, 64, 64, 1), (3, 1, 64, 128, 128, 192, 1), (2, 2, 112, 144, 320, 1280, 2), (3, 1, 128, 128, 1024, 256, 1),
         (5, 1, 240, 240, 64, 128, 1)]
# One bar for all gradient tensors and cases: E = ||device - faithful|| / ||unrounded|| <= BAR * N.  Twice the largest E / N of the
# first clean run on an MI355X (2 x 0.227, tests/test_vit_stages_gpu.py's docstring), capped at 0.25.  The max-norm is held to BAR_MAX.
BAR = 0.25
BAR_MAX = 1.0
NEG_BIAS = 8         # output channels of qkv and fc1 whose only input is the constant feature (see case_inputs)


def case_id(case):
    return "N{}v{}_{}x{}_C{}_F{}_d{}".format(*case)


# ---------------------------------------------------------------------------------------------- inputs and references

@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """Seeded parameters (lara_vit.h order, fp32), images and the output gradient.  Attention is peaked as in test_dino_gpu._seed
    (q / k weights of std sqrt(3 / C): logits of std ~ 3).  Feature 0 of norm1 and norm2 is the constant 1 (gamma = 0, beta = 1), and
    the first NEG_BIAS output channels of qkv and fc1 read only that feature, with weight -bf16(bias): their pre-activation is
    exactly zero when the bias is rounded before it is added, and bias - bf16(bias) when it is not.
    views > 1: the images are the [:, :views] slice of a [B, views + 1, H, W, 3] tensor, as LaRa's tar_rgb."""
    N, views, H, W, C, F_, depth = case
    geo = vr.geometry(*case)
    T = geo["T"]
    g = torch.Generator().manual_seed(1000 + 7 * N + 13 * T + C + F_)
    rn = lambda *s: torch.randn(*s, generator=g)
    vals = [rn(C), 0.5 * rn(T, C), rn(C, 768) * 768 ** -0.5, 0.1 * rn(C)]
    for _ in range(depth):
        n1w, n1b, n2w, n2b = 1 + 0.1 * rn(C), 0.1 * rn(C), 1 + 0.1 * rn(C), 0.1 * rn(C)
        wqkv, bqkv, w1, b1 = rn(3 * C, C) * (3.0 / C) ** 0.5, 0.1 * rn(3 * C), rn(F_, C) * C ** -0.5, 0.1 * rn(F_)
        for gam, bet, w, b in ((n1w, n1b, wqkv, bqkv), (n2w, n2b, w1, b1)):
            gam[0], bet[0] = 0.0, 1.0
            w[:NEG_BIAS] = 0.0
            w[:NEG_BIAS, 0] = -round_bf16(b[:NEG_BIAS])
        vals += [n1w, n1b, wqkv, bqkv, rn(C, C) * C ** -0.5, 0.1 * rn(C), n2w, n2b, w1, b1, rn(C, F_) * F_ ** -0.5, 0.1 * rn(C)]
    vals += [1 + 0.1 * rn(C), 0.1 * rn(C)]
    B = N // views
    rgb = torch.rand(B, views + (1 if views > 1 else 0), H, W, 3, generator=g)
    images = rgb[:, :views].reshape(N, H, W, 3).permute(0, 3, 1, 2).contiguous()
    gout = rn(N, geo["hw"], C)
    return {"geo": geo, "values": [v.contiguous() for v in vals], "rgb": rgb, "images": images, "gout": gout,
            "names": vr.param_names(depth)}


@functools.lru_cache(maxsize=None)
def reference(case, on=True, defects=()):
    """(stages, gradients) of the reference from the case's inputs alone; cached, never modified"""
    c = case_inputs(case)
    return vr.backward(c["images"], c["values"], c["geo"], c["gout"], EPS, on, None, defects)


def rel(a, b, ref):
    a, b, ref = a.double().reshape(-1), b.double().reshape(-1), ref.double().reshape(-1)
    return float((a - b).norm() / ref.norm()), float((a - b).abs().max() / ref.abs().max())


def yardstick(case):
    """{name: (N_l2, N_max)}: the bf16 noise of every gradient, from the reference alone"""
    fa, un = reference(case, True)[1], reference(case, False)[1]
    return {n: rel(f, u, u) for n, f, u in zip(case_inputs(case)["names"], fa, un)}


def compare_gradients(case, got, faithful, log=None, label="device"):
    """E / N of every gradient of `got` against `faithful` (the reference on got's own forward); -> (failures, largest E / N)"""
    un = reference(case, False)[1]
    ys = yardstick(case)
    failures, worst = [], 0.0
    for name, g, f, u in zip(case_inputs(case)["names"], got, faithful, un):
        if name == "norm.bias":
            # The column sums of the fp32 `grad`: no bf16 rounding lies in front of them, N is exactly 0 (test_vit_bf16.py asserts
            # it) and a multiple of N measures nothing.  Held to the fp32 bound of a sum of rows instead.
            gout = case_inputs(case)["gout"].double().reshape(-1, g.numel())
            lim = 4 * gout.shape[0] * U * gout.abs().sum(0) + 2.0 ** -23 * f.abs()
            ratio = float(((g.double() - f).abs() / lim).max())
            print(f"{label} {name:28s} worst |diff| / (4 A + 2^-23 |ref|) = {ratio:.3f}")
            if log is not None:
                log[f"{case_id(case)}/{name}"] = {"fp32_sum_ratio": ratio}
            if not ratio <= 1.0:
                failures.append(f"{name}: |diff| / (4 A + 2^-23 |ref|) = {ratio:.3f}")
            continue
        e2, emax = rel(g, f, u)
        n2, nmax = ys[name]
        worst = max(worst, e2 / n2)
        if log is not None:
            log[f"{case_id(case)}/{name}"] = {"E_l2": e2, "N_l2": n2, "ratio_l2": e2 / n2, "E_max": emax, "N_max": nmax,
                                              "ratio_max": emax / nmax}
        print(f"{label} {name:28s} E {e2:.3e}  N {n2:.3e}  E/N {e2 / n2:.4f}   max-norm: E {emax:.3e}  N {nmax:.3e}  E/N {emax / nmax:.4f}")
        if not e2 <= BAR * n2:
            failures.append(f"{name}: E = {e2:.3e} > {BAR} * N = {BAR * n2:.3e}")
        if not emax <= BAR_MAX * nmax:
            failures.append(f"{name}: max-norm E = {emax:.3e} > {BAR_MAX} * N = {BAR_MAX * nmax:.3e}")
    return failures, worst


# ---------------------------------------------------------------------------------------------- bounds

def ulp_bf16(ref):
    _, e = torch.frexp(ref.abs().double())
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e.clamp(min=-125) - 8)


def gemm_A(a, w, b, pre):
    """fp32 accumulation bound of a . w^T + b over K terms: K 2^-24 (|a| . |w|), and 2^-24 of the bias and of the sum"""
    return a.shape[-1] * U * (a.abs() @ w.abs().t()) + U * (b.abs() + pre.abs())


def ln_A(x, w, b, eps):
    """bounds for the fp32 LayerNorm of x [rows, C] with two-pass moments: (A of the output, A of mean, A of rstd)"""
    C = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    em = C * U * x.abs().mean(-1, keepdim=True)
    c = x - mean
    ec = em + U * c.abs()
    var = (c * c).mean(-1, keepdim=True)
    dvar = (2 * c.abs() * ec).mean(-1, keepdim=True) + (C + 2) * U * var
    rstd = 1.0 / torch.sqrt(var + eps)
    rl = dvar / (2 * (var + eps)) + 3 * U
    y = c * rstd * w + b
    return w.abs() * rstd * ec + (c * rstd * w).abs() * (rl + 3 * U) + U * y.abs(), em[:, 0], (rstd * rl)[:, 0]


def tie_flip_ulp(val, err):
    """ulp_bf16(val) where val lies within `err` of a bf16 rounding tie (the device, whose fp32 value differs from val by up to
    err, may then round the other way), else 0"""
    ulp = ulp_bf16(val)
    r = round_bf16(val)
    sgn = torch.where(val >= r, 1.0, -1.0)
    d = (val - (r + sgn * ulp / 2)).abs()
    return torch.where(d <= err, ulp, torch.zeros_like(ulp))


class Checker:
    """every stage is checked (and its worst ratio printed) before the test asserts that none failed"""

    def __init__(self):
        self.fails, self.worst = [], {"bf16": 0.0, "fp32": 0.0}

    def _judge(self, name, kind, d, lim, what):
        ratio = float((d / lim).max()) if d.numel() else 0.0
        self.worst[kind] = max(self.worst[kind], ratio)
        print(f"{name:12s} worst |diff| / ({what}) = {ratio:.3f}")
        bad = ~(d <= lim)
        if bad.any():
            self.fails.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond {what}; worst |diff| / limit = {ratio:.3f}")

    def bf16(self, name, got, ref, A):
        self._judge(name, "bf16", (got.double() - ref).abs(), ulp_bf16(ref) + A, "ulp_bf16 + A")

    def fp32(self, name, got, ref, A):
        self._judge(name, "fp32", (got.double() - ref).abs(), 4 * A + 2.0 ** -23 * ref.abs(), "4 A + 2^-23 |ref|")

    def residual(self, name, got, base, pre, A):
        lim = ulp_bf16(pre) + A + 2.0 ** -23 * (base.abs() + pre.abs())
        self._judge(name, "bf16", (got.double() - (base + pre)).abs(), lim, "ulp_bf16(pre) + A + 2^-23 (|x| + |pre|)")

    def zero(self, name, t):
        if t.numel() and not bool((t == 0).all()):
            self.fails.append(f"{name}: {int((t != 0).sum())} of {t.numel()} padded elements are not zero")

    def equal(self, name, a, b):
        if not torch.equal(a, b):
            self.fails.append(f"{name}: {int((a != b).sum())} of {a.numel()} elements differ (must be bitwise)")


def check_forward(case, got):
    """`got`: stages in the layout of `save` plus 'out', fp64 tensors.  -> Checker"""
    c = case_inputs(case)
    geo, vals = c["geo"], [v.double() for v in c["values"]]
    N, T, Tp, C, M, NP, depth = geo["N"], geo["T"], geo["Tp"], geo["C"], geo["M"], geo["NP"], geo["depth"]
    wm = lambda i: round_bf16(vals[i])
    ck = Checker()
    # patches: bitwise, the padded rows included
    ck.equal("patches", got["patches"], F.pad(vr.st_patches(c["images"]), (0, 0, 0, geo["Pp"] - NP)))
    # the tokens from the patch rows
    a, w, b = got["patches"][:NP], wm(2), wm(3)
    pre = a @ w.t() + b
    x0 = got["b0.xin"].view(N, T, C)
    pos = vals[1].view(T, C)
    ck.fp32("x0[cls]", x0[:, 0], (vals[0] + pos[0]).expand(N, C), torch.zeros(N, C, dtype=torch.float64))
    ck.residual("x0", x0[:, 1:].reshape(NP, C), pos[1:].repeat(N, 1), pre, gemm_A(a, w, b, pre))
    for i in range(depth):
        p, bi = f"b{i}.", 4 + 12 * i
        S = {k: got[p + k] for k in vr.BLOCK_STAGES}
        for k in ("xn1", "o", "xn2", "h"):
            ck.zero(p + k + "[rows >= M]", S[k][M:])
        for k in ("q", "k", "v"):
            ck.zero(p + k + "[t >= T]", S[k][:, T:])
        for xk, nk, sk, gi in (("xin", "xn1", "st1", bi), ("xmid", "xn2", "st2", bi + 6)):
            A, A_mean, A_rstd = ln_A(S[xk], vals[gi], vals[gi + 1], EPS)
            ck.bf16(p + nk, S[nk][:M], vr.st_ln(S[xk], vals[gi], vals[gi + 1], EPS), A)
            st = vr.st_stats(S[xk], EPS)
            ck.fp32(p + sk + ".mean", S[sk][:, 0], st[:, 0], A_mean)
            ck.fp32(p + sk + ".rstd", S[sk][:, 1], st[:, 1], A_rstd)
        # q, k, v from xn1
        xn1, w, b = S["xn1"][:M], wm(bi + 2), wm(bi + 3)
        pre = xn1 @ w.t() + b
        A = gemm_A(xn1, w, b, pre)
        heads = lambda t: t.view(geo["NH"], Tp, vr.HD)[:, :T].reshape(N, geo["heads"], T, vr.HD)
        q, k, v = heads(S["q"]), heads(S["k"]), heads(S["v"])
        for j, (n, t) in enumerate((("q", q), ("k", k), ("v", v))):
            ck.bf16(p + n, vr.merge_heads(t), pre[:, j * C:(j + 1) * C], A[:, j * C:(j + 1) * C])
        # o, lse from q, k, v (module docstring)
        co = vr.attn_core(q, k, v)
        A_s = vr.HD * U * 0.125 * (q.abs() @ k.abs().transpose(-1, -2)) + U * co["s"].abs()
        As = A_s.amax(-1, keepdim=True)
        p_rel = 4 * As + 2 * U * (co["s"] - co["mk"]).abs() + 16 * U
        flip = tie_flip_ulp(co["e"], p_rel * co["e"])
        pw = round_bf16(co["e"]) * co["wk"]
        A_o = ((Tp + 8) * U + 2 * p_rel.amax(-1, keepdim=True)) * (pw @ v.abs()) / co["l"] + ((flip * co["wk"]) @ v.abs()) / co["l"]
        ck.bf16(p + "o", S["o"][:M], vr.merge_heads(co["o"]), vr.merge_heads(A_o))
        print(f"{p}o: {int((flip > 0).sum())} of {flip.numel()} exponentials within their error of a tie")
        lse = S["lse"].view(geo["NH"], Tp)[:, :T].reshape(N, geo["heads"], T)
        ck.fp32(p + "lse", lse, co["lse"], As[..., 0] + 4 * U * (co["m"][..., 0].abs() + torch.log(co["l"][..., 0]).abs() + 1) + Tp * U)
        # xmid from o, xin
        o, w, b = S["o"][:M], wm(bi + 4), wm(bi + 5)
        pre = o @ w.t() + b
        ck.residual(p + "xmid", S["xmid"], S["xin"], pre, gemm_A(o, w, b, pre))
        # h from xn2
        xn2, w, b = S["xn2"][:M], wm(bi + 8), wm(bi + 9)
        pre = xn2 @ w.t() + b
        ck.bf16(p + "h", S["h"][:M], pre, gemm_A(xn2, w, b, pre))
        # xout from h (g = bf16(gelu(h)) is not saved), xmid
        h = S["h"][:M]
        gv = vr.gelu(h)
        g, w, b = round_bf16(gv), wm(bi + 10), wm(bi + 11)
        pre = g @ w.t() + b
        A = gemm_A(g, w, b, pre) + tie_flip_ulp(gv, 0.5 * h.abs() * 4 * U + 4 * U * gv.abs()) @ w.abs().t()
        xout = got[f"b{i + 1}.xin"] if i + 1 < depth else got["xfin"]
        ck.residual(p + "xout", xout, S["xmid"], pre, A)
    # the final norm: the class-token rows of stf and out do not exist
    gi = 4 + 12 * depth
    xf = got["xfin"].view(N, T, C)[:, 1:].reshape(NP, C)
    A, A_mean, A_rstd = ln_A(xf, vals[gi], vals[gi + 1], EPS)
    st = vr.st_stats(xf, EPS)
    stf = got["stf"].view(N, T, 2)[:, 1:].reshape(NP, 2)
    ck.fp32("stf.mean", stf[:, 0], st[:, 0], A_mean)
    ck.fp32("stf.rstd", stf[:, 1], st[:, 1], A_rstd)
    ck.fp32("out", got["out"].reshape(NP, C), vr.st_ln(xf, vals[gi], vals[gi + 1], EPS), A)
    return ck


def forced_from(got, geo):
    """the stages of `got` (the layout of `save`) as what oracle.vit_bf16.forward takes for `forced`"""
    N, T, Tp, M = geo["N"], geo["T"], geo["Tp"], geo["M"]
    f = {"patches": got["patches"][:geo["NP"]], "xfin": got["xfin"]}
    for i in range(geo["depth"]):
        p = f"b{i}."
        for k in ("xin", "xmid"):
            f[p + k] = got[p + k]
        for k in ("xn1", "o", "xn2", "h"):
            f[p + k] = got[p + k][:M]
        for k in ("q", "k", "v"):
            f[p + k] = got[p + k].view(geo["NH"], Tp, vr.HD)[:, :T].reshape(N, geo["heads"], T, vr.HD)
        f[p + "lse"] = got[p + "lse"].view(geo["NH"], Tp)[:, :T].reshape(N, geo["heads"], T)
    return f
