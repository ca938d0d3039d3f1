"""The cases of tests/test_coarsedec_f64.py and tests/test_coarsedec_f64_gpu.py: seeded inputs at the sizes csrc/coarsedec.hip
has code for, and the one check both files put an evaluation through -- the device's, or the fp32 CPU stand-in's.

A case is (regime, M, K, sh_dim).

Exact cases ("exact").  Every operand is a small integer: x in [-7, 7], W1 in [-3, 3], W2 and W3 in [-2, 2], biases in
[-8, 8], the shifts -2 and -5, output gradients in [-40, 40] (no offset gradient: the offset output is no integer), so
every product and every partial sum, in any order, is an integer; where sum|terms| (oracle/coarsedec_f64.py: S) stays below
2^24 the fp32 sum is exact and the reference's bound is 0: the array must then equal the reference bit for bit (-0 = 0).  The
hidden layers still round (integers above 256 are no bf16 numbers), tie, and die.  tests/test_coarsedec_f64.py asserts the
condition on every element of every exact case; only the weight gradients of the two large cases exceed 2^24 and fall under
the bound.  The one output that is no integer, offset = 2 sigmoid(z) - 1, is held to the bound of its activation at the exact z.

Ordinary cases, held to the bounds, teacher-forced stage by stage:
    default     nn.Linear's default init, biases + 0.3 randn, x = 1.1 randn (the construction of tests/test_coarsedec.py)
    saturated   weights x 4, biases +-2: |z| reaches the hundreds, offsets are exactly +-1 and act' = 0 there
    zero_row    default, rows 0, 5 and M - 1 of x all zero
    dead_layer  b1 = -1000: h1 = 0, so h2 = relu(bf16(b2)), z = bf16(W3b h2 + b3b) for every row, dz1 = dx = G1 = 0, all exact

Sizes: 1, 15, 16, 17, 31, 32, 33 (one or two 16-row column blocks of a wave, waves without a row), 127, 128, 129 (a workgroup
trip, one row more); 529 (position independence); 66 000 (516 trips: a second backward trip for four workgroups of 512);
131 205 = 1025 * 128 + 5 (a second forward trip for one workgroup of 1024, a third backward one, a ragged tail).  The exact
form runs the full cross product of the ten small sizes with the eight (K, sh_dim); a large size gets one (K, sh_dim).
"""
import functools

import torch

from oracle import coarsedec_f64 as cr

KS = [(2, 12), (1, 12), (1, 27), (3, 6), (3, 3), (4, 2), (4, 0), (1, 0)]
SMALL = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129]
LARGE = 131205
EXACT_CASES = [("exact", M, K, s) for M in SMALL for K, s in KS] + [("exact", 529, 2, 12), ("exact", 66000, 2, 12), ("exact", LARGE, 4, 2)]
REGIMES = ("default", "saturated", "zero_row", "dead_layer")
ORDINARY_CASES = ([(r, 529, 2, 12) for r in REGIMES]
                  + [("default", 129, 1, 0), ("saturated", 129, 3, 6), ("zero_row", 129, 1, 27), ("dead_layer", 129, 4, 0),
                     ("default", 33, 4, 2), ("default", 66000, 3, 3), ("default", LARGE, 2, 12)])
CASES = EXACT_CASES + ORDINARY_CASES
OPACITY_SHIFT, SCALING_SHIFT = -2.0, -5.0
GRAD_RANGE = 40
TENSORS = cr.NAMES + ("xb", "h1", "h2", "dz3", "dz2", "dz1", "dx", "G1", "G2", "G3")
PER_ROW = cr.NAMES + ("xb", "h1", "h2", "dz3", "dz2", "dz1", "dx")


def case_id(case):
    return "-".join(str(c) for c in case)


def _randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def inputs(regime, M, K, sh_dim):
    """the fp32 tensors an evaluation gets: x, w1 .. b3, g = {name: [M, K * width] or None}, the two shifts"""
    n_par = K * (10 + sh_dim)
    g = torch.Generator().manual_seed(10007 * (["exact"] + list(REGIMES)).index(regime) + 101 * (M % 9973) + 7 * K + sh_dim)
    w = cr.widths(sh_dim)
    if regime == "exact":
        t = {"x": _randint(g, -7, 7, M, 80), "w1": _randint(g, -3, 3, 80, 80), "b1": _randint(g, -8, 8, 80),
             "w2": _randint(g, -2, 2, 80, 80), "b2": _randint(g, -8, 8, 80), "w3": _randint(g, -2, 2, n_par, 80),
             "b3": _randint(g, -8, 8, n_par)}
        grads = {n: (None if n == "offset" else _randint(g, -GRAD_RANGE, GRAD_RANGE, M, K * w[n])) for n in cr.NAMES}
    else:
        b = 80 ** -0.5
        uni = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * b
        t = {"x": 1.1 * torch.randn(M, 80, generator=g)}
        for i, rows in ((1, 80), (2, 80), (3, n_par)):
            t[f"w{i}"], t[f"b{i}"] = uni(rows, 80), uni(rows) + 0.3 * torch.randn(rows, generator=g)
        grads = {n: torch.randn(M, K * w[n], generator=g) for n in cr.NAMES}
        if regime == "saturated":
            for i in (1, 2, 3):
                t[f"w{i}"] = t[f"w{i}"] * 4
                t[f"b{i}"] = torch.where(torch.arange(t[f"b{i}"].numel()) % 2 == 0, 2.0, -2.0) + t[f"b{i}"]
        elif regime == "zero_row":
            t["x"][[0, min(5, M - 1), M - 1]] = 0.0
        elif regime == "dead_layer":
            t["b1"] = torch.full((80,), -1000.0)
    t.update(g=grads, opacity_shift=OPACITY_SHIFT, scaling_shift=SCALING_SHIFT)
    return t


# ---------------------------------------------------------------------------------------------- the check

def _worst(r):
    return float(r.max()) if r.numel() else 0.0


def _bad(flag):
    return cr.INF if bool(flag) else 0.0


def factor_structure(got, M, n_par):
    """what the header promises of the six factor matrices beyond their values -> {name: 0 or inf}"""
    Mp = cr.padded_rows(M)
    res = {}
    for name, cols in cr.FACTORS:
        a = got[name]
        bad = tuple(a.shape) != (Mp, cols) or not bool(torch.isfinite(a).all())
        if not bad and name in ("xb", "h1", "h2"):
            bad = bool((a[:, 80] != 1).any()) or bool((a[:, 81:] != 0).any())       # the ones column, all M_pad rows; the zeros
        if not bad and name.startswith("dz"):
            bad = bool((a[M:] != 0).any())                                           # rows M .. M_pad
        if not bad and name == "dz3":
            bad = bool((a[:, n_par:] != 0).any())
        res[name] = _bad(bad)
    return res


def check(case, t, got, prefill=None, flips=None):
    """`got`: the five outputs [M, K * width] of the forward entry point; of the backward one (run with got's own offset as
    `offset_out`) dx [M, 80] and the six factor matrices [M_pad, .] as fp32; G1, G2, G3 = prefill + the three products of
    lara_gemm_tn_bf16 on those matrices.  -> {tensor: worst |diff| / limit}, inf where the structure of a factor matrix is broken.
    Ordinary cases are teacher-forced from got's own xb, h1, h2, dz3, dz2, dz1; exact cases are held to the reference's own
    chain, whose bound is 0 wherever sum|terms| < 2^24.  `flips` (a dict) receives, per bf16 stage, the share of elements that are
    not the reference's fp64 value rounded: the ratios of these stages approach 1 at every near-tie by construction (a correctly
    rounded value sits up to half an ulp from the unrounded reference), so this share is the figure that tells two correct
    evaluations apart."""
    regime, M, K, sh_dim = case
    exact = regime == "exact"
    n_par = K * (10 + sh_dim)
    res = factor_structure(got, M, n_par)
    if any(res.values()):
        broken = {k for k, v in res.items() if v}
        got = dict(got, **{k: torch.nan_to_num(got[k], 0.0, 0.0, 0.0) for k in broken})
    cut = lambda k: got[k][:M, :80]
    fo = None if exact else {k: cut(k) for k in ("xb", "h1", "h2")}
    f = cr.forward(t, K, sh_dim, forced=fo, exact=exact)
    res["xb"] = max(res["xb"], _bad((cr.f64(cut("xb")) != f["xb"]).any()))
    for i, k in ((1, "h1"), (2, "h2")):
        res[k] = max(res[k], _worst(cr.ratio_bf16(cut(k), f[f"pre{i}"], f[f"A_pre{i}"], relu=True)))
        if flips is not None:
            flips[k] = float((cr.f64(cut(k)) != torch.relu(cr.bf16(f[f"pre{i}"]))).double().mean())
    out = cr.output_ratios(got, f["z_pre"], f["A_z"], K, sh_dim, t["opacity_shift"], t["scaling_shift"], exact=exact)
    res.update({k: _worst(v) for k, v in out.items()})
    if flips is not None:
        zb = cr.bf16(f["z_pre"])
        flips["z"] = float(torch.cat([cr.f64(got[n]) != zb[:, cr.columns(K, sh_dim)[n]] for n in ("sh", "rotation")], 1).double().mean())
    h1, h2 = (f["h1"], f["h2"]) if exact else (cut("h1"), cut("h2"))
    bo = None if exact else {"dz3": got["dz3"][:M], "dz2": got["dz2"][:M], "dz1": got["dz1"][:M]}
    b = cr.backward(t, K, sh_dim, t["g"], got["offset"], h1, h2, forced=bo, exact=exact)
    for k in ("dz3", "dz2", "dz1"):
        res[k] = max(res[k], _worst(cr.ratio_bf16(got[k][:M], b[k + "_pre"], b["A_" + k])))
        if flips is not None:
            flips[k] = float((cr.f64(got[k][:M]) != cr.bf16(b[k + "_pre"])).double().mean())
    res["dx"] = _worst(cr.ratio_f32(got["dx"], b["dx"], b["A_dx"]))
    Mp = cr.padded_rows(M)
    for i, (dz, act) in enumerate((("dz1", "xb"), ("dz2", "h1"), ("dz3", "h2")), 1):
        if exact:
            d, a = torch.cat([b[dz], b[dz].new_zeros(Mp - M, b[dz].shape[1])]), cr.with_ones(f[act], Mp)
        else:
            d, a = got[dz], got[act]
        G, A, _ = cr.wgrad(d, a, prefill=None if prefill is None else prefill[f"G{i}"], exact=exact)
        res[f"G{i}"] = _worst(cr.ratio_f32(got[f"G{i}"], G, A))
    return res


def exactness(case, t):
    """an exact case -> {stage: (largest sum|terms|, every operand an integer?)} of the reference's own chain"""
    _, M, K, sh_dim = case
    f = cr.forward(t, K, sh_dim, exact=True)
    b = cr.backward(t, K, sh_dim, t["g"], None, f["h1"], f["h2"], exact=True)
    whole = lambda *xs: all(bool((x == x.round()).all()) for x in xs)
    w = cr.operands(t)
    res = {"pre1": (float(f["S_pre1"].max()), whole(f["xb"], w["w1"], w["b1"]) and torch.equal(f["xb"], cr.f64(t["x"]))),
           "pre2": (float(f["S_pre2"].max()), whole(f["h1"], w["w2"], w["b2"])),
           "z": (float(f["S_z"].max()), whole(f["h2"], w["w3"], w["b3"])),
           "dz2": (float(b["S_dz2"].max()), whole(b["dz3"])), "dz1": (float(b["S_dz1"].max()), whole(b["dz2"])),
           "dx": (float(b["S_dx"].max()), whole(b["dz1"]))}
    for i, (dz, act) in enumerate((("dz1", "xb"), ("dz2", "h1"), ("dz3", "h2")), 1):
        res[f"G{i}"] = (float(cr.wgrad(b[dz], cr.with_ones(f[act], M))[2].max()), True)
    return res, f, b


def exact_claims(case, t, got):
    """what a regime promises exactly, beyond the bounds -> list of failures"""
    regime, M, K, sh_dim = case
    fails = []
    cols = cr.columns(K, sh_dim)
    if regime == "dead_layer":
        w = cr.operands(t)
        h2 = torch.relu(w["b2"])
        for k in ("h1", "dz1"):
            if bool((got[k][:, :80] != 0).any()):
                fails.append(f"{k} is not zero behind a dead layer")
        if bool((got["dx"] != 0).any()) or bool((got["G1"] != 0).any()) or bool((got["G2"][:, :80] != 0).any()):
            fails.append("dx, G1 or dW2 is not zero behind a dead layer")
        if not torch.equal(cr.f64(got["h2"][:M, :80]), h2.expand(M, 80)):
            fails.append("h2 is not relu(bf16(b2)) behind a dead layer")
        for n in cr.NAMES:                # every row is the same row
            if got[n].numel() and not torch.equal(got[n], got[n][:1].expand_as(got[n])):
                fails.append(f"{n}: rows differ behind a dead layer")
    if regime == "saturated":
        o = got["offset"]
        sat = o.abs() == 1
        if not bool(sat.any()):
            fails.append("no saturated offset")
        if bool((got["dz3"][:M][:, cols["offset"]][sat] != 0).any()):
            fails.append("dz3 of a saturated offset is not zero")
    if bool((got["offset"].abs() > 1).any()):
        fails.append("an offset outside [-1, 1]")
    return fails
