"""fp64 reference of the coarse decoder's two entry points (include/lara_coarsedec.h), stage by stage -- TEST INFRASTRUCTURE
ONLY (the checker of tests/test_coarsedec_f64.py and tests/test_coarsedec_f64_gpu.py; nothing under lara_amd/ imports it, and
it reads nothing of the code under test).  Written from the header and from lightning/network.py:259-278.

Stages, in torch fp64 on the CPU, rounded to bf16 (nearest even) exactly where the header says ("weights and biases are rounded
to bf16 when they are staged, activations when they become the next layer's operand", "a bf16 result"):
    W_l b = bf16(W_l), b_l b = bf16(b_l)
    xb  = bf16(x)
    h1  = relu(bf16(W1b xb + b1b)),   h2 = relu(bf16(W2b h1 + b2b)),   z = bf16(W3b h2 + b3b)
    per k the split [3 | sh_dim | 1 | 2 | 4] of z:  offset = 2 sigmoid(z) - 1,  sh = z,  opacity = z + opacity_shift,
                                                     scaling = z + scaling_shift,  rotation = z
    dz3 = bf16(g act'),  act' = (1 - o^2) / 2 on the offset columns (o = the offset OUTPUT handed in), 1 elsewhere
    dz2 = [h2 > 0] bf16(W3b^T dz3),   dz1 = [h1 > 0] bf16(W2b^T dz2),   dx = W1b^T dz1  (fp32)
    G_l = dz_l^T [act_l | 1 | 0..0]   (act_1 = xb, act_2 = h1, act_3 = h2; all M_pad rows of the factor matrices as given)

Every function returns, beside each value X, the fp32 error bound A_X of every element of X from the reference's own operands
(the rules of oracle/finedec_f64.py, all first order; the acceptance test's factor 4 absorbs the rest):
    a sum of K terms       K 2^-24 sum|terms|, any order, fused or not.  Products of two bf16 numbers are exact in fp32 and
                           cost nothing; a term that is exactly zero costs nothing either: K is the number of non-zero terms,
                           at most 81 for a layer with its bias, 48 or 80 for the transposed products, M_pad (+ 1 for a
                           pre-filled destination) for a weight gradient -- and a "sum" of at most one term is exact, A = 0.
    one operation          2^-24 |result|
    exact = True           (the integer cases of tests/coarsedec_cases.py) every operand is an integer, so a sum whose
                           sum|terms| (returned as S_X: every partial sum in any order stays below it) is below 2^24 is
                           exact in fp32: A = 0 for those elements.

The offset activation.  The device evaluates o = 2 / (1 + e) - 1 with e = exp(-z) from a hardware exponential: the argument
is scaled by log2(e) (one rounding, 2^-24 |z| log2(e) absolute in the exponent, i.e. |z| 2^-24 relative in e, doubled for a
range reduction or a fused scale of either kind) and v_exp_f32 is good to one ulp of its result and of its argument's last
place; together a relative error of e of at most (|z| + 2) 2^-23.  It reaches o through |do/de| = 2 / (1 + e)^2, i.e.
    |do| <= 2 e / (1 + e)^2 (|z| + 2) 2^-23            [= 2 s (1 - s) (|z| + 2) 2^-23 with s = sigmoid(z): no overflow]
then 1 + e (2^-24 (1 + e), which the quotient turns into 2^-24 * 2 / (1 + e)), the quotient itself (2^-24 * 2 / (1 + e)) and
the subtraction (2^-24 |o|):
    A_o = 2 s (1 - s) (|z| + 2) 2^-23 + 2 * 2^-24 * 2 s + 2^-24 |o|
For z >= 17.4 fp32 has 1 + e = 1 and o = 1 exactly, for z <= -89 e overflows and o = -1 exactly; both lie inside A_o of the
fp64 value.  z = 0 gives e = 1 and o = 0 exactly on any hardware; the bound does not rely on it.
The backward's act' = 0.5 (1 - o o): the product and the difference (fused or not) cost 2^-24 (o^2 + |1 - o^2|) on 1 - o^2,
the product with g 2^-24 |g act'|; 1 - o^2 = 0 (a saturated offset, o = +-1) is exact and gives an exact zero.

Acceptance (`ratio_f32`, `ratio_bf16`, `output_ratios`: |got - ref| / limit per element, inf for a non-finite `got`):
    fp32 stages   |got - ref| <= 4 A + 2^-23 |ref|                                    (dx, G_l)
    bf16 stages   |got - ref| <= 4 A + ulp_bf16(|ref| + 4 A) / 2 + 2^-126,            (h1, h2, z, dz_l)
                  ref the UNROUNDED fp64 value: the correctly rounded value of any fp32 sum within the accumulation bound
                  passes; truncation, or a second rounding, does not.  Behind a ReLU ref is relu(pre), and where pre < -4 A
                  every correct fp32 sum is negative: the value must be exactly 0.
    A = 0         the value is determined: it must equal ref (fp32 stages) or bf16(ref) (bf16 stages) exactly; in particular
                  an element with A = 0 and ref = 0 must be 0.  -0.0 counts as 0 (fmaxf(-0, 0) may keep the sign).
    outputs       z is not handed out, so an output is held to the bf16 stage z and the fp32 operation behind it together:
                  |got - f(c)| <= slope * L_z + 4 A_f + 2^-23 |f(c)|, with c = the unrounded z, L_z its bf16-stage limit
                  (c = bf16(z) and L_z = 0 where A_z = 0), slope the largest |f'| over [c - L_z, c + L_z] (1 for the shifts,
                  2 s (1 - s) at the end nearer to 0 for the offset).  sh and rotation are z itself: the bf16 rule alone.

Teacher forcing.  `forward(.., forced={"xb", "h1", "h2"})` and `backward(.., forced={"dz3", "dz2", "dz1"})` restart each stage
from the arrays an evaluation under test handed out, with no inherited bound; the ReLU masks are taken from the `h1`, `h2`
arguments (the arrays under test, or the reference's own).  `wgrad` is forced by construction.
"""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
EXACT_BELOW = 2.0 ** 24
F, FA, O, PTS = 80, 88, 48, 128
NAMES = ("offset", "sh", "scaling", "rotation", "opacity")
FACTORS = (("xb", FA), ("h1", FA), ("h2", FA), ("dz1", F), ("dz2", F), ("dz3", O))
INF = float("inf")


def f64(x):
    return torch.as_tensor(x).detach().to("cpu", torch.float64)


def bf16(x):
    """Nearest-even bf16 rounding of the fp32 value of x by integer arithmetic on the fp32 bits (NaN stays NaN, subnormals
    round like everything else, values beyond the last tie become inf) -> fp64"""
    f = torch.as_tensor(x).detach().to("cpu", torch.float32).contiguous()
    u = f.view(torch.int32)                                      # (two's complement: the sum below cannot wrap for a non-NaN)
    r = (u + (0x7FFF + ((u >> 16) & 1))) & -65536
    r = torch.where(torch.isnan(f), (u | 0x00400000) & -65536, r)
    return r.view(torch.float32).to(torch.float64)


def ulp_bf16(v):
    """the spacing of bf16 numbers at |v| (2^-133 below 2^-126)"""
    v = f64(v).abs()
    _, e = torch.frexp(v)
    ulp = torch.pow(torch.full_like(v, 2.0), (e - 8).to(torch.float64))
    return torch.where(v < TINY, torch.full_like(v, 2.0 ** -133), ulp)


def padded_rows(M):
    return (M + PTS - 1) // PTS * PTS


def widths(sh_dim):
    return {"offset": 3, "sh": sh_dim, "scaling": 2, "rotation": 4, "opacity": 1}


def columns(K, sh_dim):
    """{output tensor: the columns of z it is made of, in the tensor's own order [k * width + c]}: network.py:262-270"""
    per = 10 + sh_dim
    start = {"offset": 0, "sh": 3, "opacity": 3 + sh_dim, "scaling": 4 + sh_dim, "rotation": 6 + sh_dim}
    return {n: torch.tensor([k * per + start[n] + c for k in range(K) for c in range(w)], dtype=torch.long)
            for n, w in widths(sh_dim).items()}


def operands(t, on=True):
    """the six parameters as the kernels stage them: rounded to bf16, W3 and b3 padded with zeros to 48 outputs"""
    rnd = bf16 if on else f64
    w = {k: rnd(t[k]) for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    n_par = w["w3"].shape[0]
    w["w3"] = torch.cat([w["w3"], torch.zeros(O - n_par, F, dtype=torch.float64)])
    w["b3"] = torch.cat([w["b3"], torch.zeros(O - n_par, dtype=torch.float64)])
    return w


def _terms(a, b, extra, kmax, exact):
    """a @ b (+ extra), its bound and sum|terms|"""
    val, S = a @ b, a.abs() @ b.abs()
    nnz = (a != 0).to(torch.float64) @ (b != 0).to(torch.float64)
    if extra is not None:
        val, S, nnz = val + extra, S + extra.abs(), nnz + (extra != 0).to(torch.float64)
    k = torch.where(nnz <= 1, torch.zeros_like(nnz), nnz.clamp(max=kmax))
    A = k * U * S
    if exact:
        A = torch.where(S < EXACT_BELOW, torch.zeros_like(A), A)
    return val, A, S


# ---------------------------------------------------------------------------------------------- the stages

def forward(t, K, sh_dim, on=True, forced=None, exact=False):
    """x [M, 80] -> xb, pre1 / h1, pre2 / h2, z_pre (unrounded) / z [M, 48] with "A_" and "S_" of the three sums, and the five
    outputs of the unforced chain ("out": {name: [M, K * width]})"""
    forced = forced or {}
    rnd = bf16 if on else f64
    w = operands(t, on)
    r = {"xb": rnd(t["x"])}
    a = f64(forced["xb"]) if "xb" in forced else r["xb"]
    for i, name in ((1, "h1"), (2, "h2")):
        pre, A, S = _terms(a, w[f"w{i}"].t(), w[f"b{i}"], F + 1, exact)
        r.update({f"pre{i}": pre, f"A_pre{i}": A, f"S_pre{i}": S, name: torch.relu(rnd(pre))})
        a = f64(forced[name]) if name in forced else r[name]
    pre, A, S = _terms(a, w["w3"].t(), w["b3"], F + 1, exact)
    r.update(z_pre=pre, A_z=A, S_z=S, z=rnd(pre))
    r["out"] = {n: v[0] for n, v in activations(r["z"], K, sh_dim, t["opacity_shift"], t["scaling_shift"], exact).items()}
    return r


def activations(z, K, sh_dim, opacity_shift, scaling_shift, exact=False):
    """z [M, 48] (fp64, as given) -> {name: (value, A of the fp32 operation, |f'|)} [M, K * width]"""
    out = {}
    for n, idx in columns(K, sh_dim).items():
        c = z[:, idx]
        if n == "offset":
            s = torch.sigmoid(c)
            o = 2 * s - 1
            slope = 2 * s * (1 - s)
            out[n] = (o, slope * (c.abs() + 2) * 2 * U + 2 * U * 2 * s + U * o.abs(), slope)
        elif n in ("scaling", "opacity"):
            shift = float(scaling_shift if n == "scaling" else opacity_shift)
            v = c + shift
            A = U * v.abs() * (c != 0) * (shift != 0)
            if exact:
                A = torch.where(v.abs() < EXACT_BELOW, torch.zeros_like(A), A)
            out[n] = (v, A, torch.ones_like(c))
        else:
            out[n] = (c, torch.zeros_like(c), torch.ones_like(c))
    return out


def backward(t, K, sh_dim, g, offset_out, h1, h2, on=True, forced=None, exact=False):
    """g: {name: [M, K * width] or None}; offset_out: the forward's offset output as handed to the entry point (needed when
    g["offset"] is given); h1, h2 [M, 80]: the activations whose sign is the ReLU mask.
    -> dz3_pre / dz3 [M, 48], dz2_pre / dz2, dz1_pre / dz1 [M, 80] (pre: unrounded, already masked), dx, with "A_" and "S_" """
    forced = forced or {}
    rnd = bf16 if on else f64
    w = operands(t, on)
    M = f64(t["x"]).shape[0]
    pre, A = torch.zeros(M, O, dtype=torch.float64), torch.zeros(M, O, dtype=torch.float64)
    for n, idx in columns(K, sh_dim).items():
        if g.get(n) is None or not idx.numel():
            continue
        gn = f64(g[n]).reshape(M, -1)
        if n == "offset":
            o = f64(offset_out).reshape(M, -1)
            o2 = o * o
            d = 1 - o2
            v = gn * 0.5 * d
            pre[:, idx], A[:, idx] = v, (gn.abs() * 0.5 * U * (o2 + d.abs()) + U * v.abs()) * (d != 0)
        else:
            pre[:, idx] = gn
    r = {"dz3_pre": pre, "A_dz3": A, "dz3": rnd(pre)}
    a = f64(forced["dz3"]) if "dz3" in forced else r["dz3"]
    for name, wk, kmax, h in (("dz2", "w3", O, h2), ("dz1", "w2", F, h1)):
        mask = (f64(h) > 0).to(torch.float64)
        pre, A, S = _terms(a, w[wk], None, kmax, exact)
        r.update({name + "_pre": pre * mask, "A_" + name: A * mask, "S_" + name: S * mask, name: rnd(pre) * mask})
        a = f64(forced[name]) if name in forced else r[name]
    r["dx"], r["A_dx"], r["S_dx"] = _terms(a, w["w1"], None, F, exact)
    return r


def with_ones(act, rows):
    """[M, 80] -> the activation factor matrix [rows, 88]: a column of ones, seven of zeros, rows >= M zero"""
    out = torch.zeros(rows, FA, dtype=torch.float64)
    out[:act.shape[0], :F] = f64(act)
    out[:act.shape[0], F] = 1.0
    return out


def wgrad(dz, act, prefill=None, exact=False):
    """dz [rows, n], act [rows, 88] as given (all rows) -> G = prefill + dz^T act [n, 88], A, S"""
    dz, act = f64(dz), f64(act)
    return _terms(dz.t(), act, None if prefill is None else f64(prefill), dz.shape[0] + 1, exact)


# ---------------------------------------------------------------------------------------------- acceptance

def _ratio(got, ref, lim):
    got = f64(got).reshape(ref.shape)
    d = (got - ref).abs()
    r = torch.where(lim > 0, d / lim, torch.where(d > 0, torch.full_like(d, INF), torch.zeros_like(d)))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, INF))


def ratio_f32(got, ref, A):
    return _ratio(got, ref, torch.where(A > 0, 4 * A + 2 * U * ref.abs(), torch.zeros_like(A)))


def limit_bf16(ref, A):
    return 4 * A + ulp_bf16(ref.abs() + 4 * A) / 2 + TINY


def ratio_bf16(got, ref, A, relu=False):
    """`ref`: the unrounded fp64 value (in front of the ReLU when relu=True)"""
    centre = torch.relu(ref) if relu else ref
    lim = limit_bf16(centre, A)
    if relu:
        lim = torch.where(ref < -4 * A, torch.zeros_like(lim), lim)
    det = A == 0
    if bool(det.any()):
        rounded = torch.relu(bf16(ref)) if relu else bf16(ref)
        centre, lim = torch.where(det, rounded, centre), torch.where(det, torch.zeros_like(lim), lim)
    return _ratio(got, centre, lim)


def output_ratios(got, z_pre, A_z, K, sh_dim, opacity_shift, scaling_shift, exact=False):
    """the five outputs against the unrounded z_pre [M, 48] and its bound -> {name: ratio [M, K * width]}"""
    det = A_z == 0
    c = torch.where(det, bf16(z_pre), z_pre)
    L = torch.where(det, torch.zeros_like(A_z), limit_bf16(z_pre, A_z))
    res = {}
    at_c = activations(c, K, sh_dim, opacity_shift, scaling_shift, exact)
    near = activations(torch.relu(c.abs() - L), K, sh_dim, opacity_shift, scaling_shift, exact)   # the end of [c - L, c + L] nearer to 0
    for n, idx in columns(K, sh_dim).items():
        ref, A_f, _ = at_c[n]
        if n in ("sh", "rotation"):
            res[n] = ratio_bf16(got[n], z_pre[:, idx], A_z[:, idx])
            continue
        lim = near[n][2] * L[:, idx] + torch.where(A_f > 0, 4 * A_f + 2 * U * ref.abs(), torch.zeros_like(A_f))
        res[n] = _ratio(got[n], ref, lim)
    return res
