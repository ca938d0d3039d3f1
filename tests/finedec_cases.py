"""The cases of tests/test_finedec_f64.py and tests/test_finedec_f64_gpu.py: sizes at the edges csrc/finedec.hip has code for,
seeded value regimes, the fp64 reference's results (oracle/finedec_f64.py; computed once per case, shared, never modified) and
the checks both files put an evaluation of the stage through -- the device's, or the fp32 CPU stand-in's.

Sizes (the ordinary regime runs at all of them): 1; 32 +- 1 (a wave), 128 +- 1 (a tile of the persistent decoder kernels), 256 +- 1
(a LayerNorm block), 512 +- 1 (a weight-gradient slab), 527 / 529 (a slab + 15 / 17 rows: either side of its 16-row K step),
512 k + 1 for k in 2..8 and 12 (k + 1 slabs: every phase and both chains of the reduce, which walks slabs eight at a time in
four phases), 4096 (exactly eight slabs) and 131205 = 1025 tiles + 5: a second forward trip for workgroups 0 and 1 only, three
backward trips, 257 slabs, 513 LayerNorm blocks.

Value regimes of the decoder (each also at n = 129 and 529):
    ordinary   parameters of FineDecoderRef() + 0.1 randn, randn inputs (as tests/test_finedec.py)
    saturated  pf x 4 and Wqk scaled so that the scores have a standard deviation of 40: maxima beyond 88 (only the max
               subtraction keeps exp finite), gaps beyond 104 (P = 1 for one view, the others flush to zero).  The prescribed
               bound of P is relative to the scores' own bound (4 A_s ~ 3 % here), whatever the saturation, and 8 x what
               it leaves of the pre-activations' bound is wider than their spread: b1 gets +-40 on alternate units, which
               places every unit far from zero by construction, as the dead regime does
    ties       a third of the points with four identical views (P = 1/4 whatever the query), a third with two identical views
               (which tie for the maximum wherever they are the maximum)
    dead       b1 = -1000 on 16 units (dead for every point).  b1 is one vector for all points, so "every unit dead on every
               fifth point" is made from the inputs: W1ov gets -0.1 on its eight channel-7 columns and those points carry 600
               in channel 7 of all four views (u[h, 7] = 600 whatever P), which puts every unit near -480 (and shifts the
               other points' units by 0.1 randn only).  There sh = b2 and
               d_xn, d_pf, DH, DT are exactly zero
    zero_dsh   d_sh = 0: every gradient and DH, DT exactly zero
LayerNorm regimes (n in 1, 255, 257, 529; ordinary also 256 and 131205): ordinary rows; constant rows (multiples of 1/8, so the
fp32 sum and mean are exact: xn = beta exactly, rstd = 1 / sqrt(eps)); an offset of 1e3 plus unit noise; one outlier feature of
1e4 per row; gamma zero on 8 columns.

The kink condition.  No hidden pre-activation lies within 8 x its own propagated bound of zero (oracle/finedec_f64.py: A_PRE):
whatever the summation order, every correct fp32 evaluation then takes the reference's branch of the ReLU.  Offending points are
nudged for up to 50 rounds; none may be left, no point is dropped.  The nudge of round r is a seeded random step away from
where the point was drawn (0.1 (1 + r / 5) randn on xn and on pf -- 0.4 where pf is scaled by 4 -- the same step for the four
views so that identical views stay identical; pf too, because with identical or saturated views u does not depend on xn), not
the 0.3 % scaling of tests/test_finedec.py: the window here is 8 x a worst-case bound (K = 80 for t, four times the score
bound inside P), some 5e-3 wide against that test's 1e-5, so that a third of all points have one of their 64 units inside it,
a 0.3 % scaling does not carry a point out of it, and a few points in 10^5 stay inside for any small step.
"""
import functools

import torch

from oracle import finedec_f64 as fr
from oracle.finedec_ref import FineDecoderRef

SIZES = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 527, 529] + [512 * k + 1 for k in (2, 3, 4, 5, 6, 7, 8, 12)] + [4096, 131205]
LARGE = 131205
REGIMES = ("ordinary", "saturated", "ties", "dead", "zero_dsh")
CASES = [("ordinary", n) for n in SIZES] + [(r, n) for r in REGIMES[1:] for n in (129, 529)]
LN_REGIMES = ("ordinary", "constant", "offset", "outlier", "gamma0")
LN_CASES = [(r, n) for r in LN_REGIMES for n in (1, 255, 257, 529)] + [("ordinary", 256), ("ordinary", LARGE)]
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))
KINK = 8.0
DEAD_UNITS = list(range(3, 64, 4))         # 16 units
DEAD_EVERY, DEAD_VALUE, DEAD_WEIGHT = 5, 600.0, 0.1
GAMMA0 = list(range(5, 80, 10))            # 8 columns
DECODER_TENSORS = ("sh", "U", "HID", "DH", "DT", "d_xn", "d_pf", "wgrad")


def case_id(case):
    return f"{case[0]}-{case[1]}"


def _weights(g, seed):
    from lara_amd.fine import _fold_fine_weights
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        dec = FineDecoderRef()
    with torch.no_grad():
        for p in dec.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
        return [w.detach().clone() for w in _fold_fine_weights(dec)]


def pure_forward(t):
    return fr.fine_decoder_forward(t["xn"], t["pf"], t["Wqk"], t["W1ov"], t["b1"], t["W2"], t["b2"])


def on_kink(f):
    """[n] bool: a hidden pre-activation within KINK x its own bound of zero"""
    return (f["PRE"].abs() <= KINK * f["A_PRE"]).any(-1)


@functools.lru_cache(maxsize=None)
def inputs(regime, n):
    """the fp32 tensors the device gets: xn [n, 80], pf [4, 8, n], the five folded parameters, d_sh [n, 12]"""
    seed = 1000 * REGIMES.index(regime) + n % 1000 + n // 1000
    g = torch.Generator().manual_seed(seed)
    Wqk, W1ov, b1, W2, b2 = _weights(g, seed)
    xn, pf, d_sh = torch.randn(n, 80, generator=g), torch.randn(4, 8, n, generator=g), torch.randn(n, 12, generator=g)
    if regime == "saturated":
        pf = pf * 4
        s = fr.fine_decoder_attention(xn, pf, Wqk)["s"]
        Wqk = (Wqk * (40.0 / float(s.std()))).float()
        b1 = torch.where(torch.arange(64) % 2 == 0, 40.0, -40.0) + b1
    elif regime == "ties":
        third = torch.arange(n) % 3
        pf[:, :, third == 0] = pf[:1, :, third == 0]
        pf[1, :, third == 1] = pf[3, :, third == 1]
    elif regime == "dead":
        b1[DEAD_UNITS] = -1000.0
        W1ov[:, 7::8] -= DEAD_WEIGHT
        pf[:, 7, ::DEAD_EVERY] = DEAD_VALUE
    elif regime == "zero_dsh":
        d_sh = torch.zeros(n, 12)
    t = {"xn": xn, "pf": pf, "Wqk": Wqk, "W1ov": W1ov, "b1": b1, "W2": W2, "b2": b2, "d_sh": d_sh}
    step = 0.4 if regime == "saturated" else 0.1
    bad = on_kink(pure_forward(t)).nonzero().squeeze(-1)
    xn0, pf0 = xn.clone(), pf.clone()
    for rnd in range(50):
        if not bad.numel():
            break
        grow = 1 + rnd / 5            # a stubborn point is moved further from where it was drawn
        t["xn"][bad] = xn0[bad] + 0.1 * grow * torch.randn(bad.numel(), 80, generator=g)
        # (one step for the four views: identical views stay identical)
        t["pf"][:, :, bad] = pf0[:, :, bad] + step * grow * torch.randn(1, 8, bad.numel(), generator=g)
        bad = bad[on_kink(pure_forward(dict(t, xn=t["xn"][bad], pf=t["pf"][:, :, bad])))]
    assert not bad.numel(), f"{regime}/{n}: {bad.numel()} points left on the ReLU's kink after 50 rounds"
    return t


@functools.lru_cache(maxsize=None)
def ln_inputs(regime, n):
    g = torch.Generator().manual_seed(7000 + 1000 * LN_REGIMES.index(regime) + n % 1000)
    x = torch.randn(n, 80, generator=g) * (0.5 + 1.5 * torch.rand(n, 1, generator=g)) + torch.randn(n, 1, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(80, generator=g), 0.2 * torch.randn(80, generator=g)
    d_xn = torch.randn(n, 80, generator=g)
    if regime == "constant":
        x = (torch.randint(-40, 41, (n, 1), generator=g).float() / 8).expand(n, 80).contiguous()
    elif regime == "offset":
        x = torch.randn(n, 80, generator=g) + 1e3
    elif regime == "outlier":
        x[torch.arange(n), torch.randint(0, 80, (n,), generator=g)] = 1e4
    elif regime == "gamma0":
        gamma[GAMMA0] = 0.0
    return {"x": x, "gamma": gamma, "beta": beta, "d_xn": d_xn}


# ---------------------------------------------------------------------------------------------- the checks

def _worst(got, ref, A):
    r = fr.ratio(got, ref, A)
    return float(r.max()) if r.numel() else 0.0


def check_decoder(t, got, att=None, drop_row=None):
    """`got`: sh of the forward entry point, and of the backward one d_xn, d_pf, U, HID, DH, DT, then wgrad (the flat `out` of
    the weight-gradient entry point run on those arrays) -> {tensor: worst |diff| / limit}, the five parts of wgrad also one
    by one.  Teacher-forced from got's own U, HID, DH, DT.  The mutation checks: `att` replaces the reference's attention,
    `drop_row` leaves that row out of the reference's weight gradients."""
    n = t["xn"].shape[0]
    w = [t[k] for k in ("xn", "pf", "Wqk", "W1ov", "b1", "W2", "b2")]
    r = fr.fine_decoder_backward(*w, t["d_sh"], att=att, forced={k: got[k] for k in ("U", "HID", "DH", "DT")})
    out = {k: _worst(got[k], r[k], r["A_" + k]) for k in DECODER_TENSORS if k != "wgrad"}
    keep = torch.ones(n, 1, dtype=torch.float64)
    if drop_row is not None:
        keep[drop_row] = 0.0
    ref, A = fr.fine_decoder_wgrad(n, *(fr.f64(x) * keep for x in (t["xn"], got["U"], got["HID"], got["DH"], got["DT"], t["d_sh"])))
    out["wgrad"] = _worst(got["wgrad"], ref, A)
    parts = zip(fr.split_wgrad(fr.f64(got["wgrad"])).items(), fr.split_wgrad(ref).values(), fr.split_wgrad(A).values())
    out.update({"wgrad." + k: _worst(g, rr, aa) for (k, g), rr, aa in parts})
    return out


def check_ln(t, got):
    """`got`: xn, stats of the forward entry point, d_x and partials of the backward one run on got's own stats"""
    f = fr.fine_ln_forward(t["x"], t["gamma"], t["beta"], LN_EPS)
    ff = fr.fine_ln_forward(t["x"], t["gamma"], t["beta"], LN_EPS, stats_forced=got["stats"])
    b = fr.fine_ln_backward(t["x"], t["gamma"], got["stats"], t["d_xn"])
    tot = fr.f64(got["partials"]).sum(0)
    return {"xn": _worst(got["xn"], f["xn"], f["A_xn"]), "xn|stats": _worst(got["xn"], ff["xn"], ff["A_xn"]),
            "stats": _worst(got["stats"], f["stats"], f["A_stats"]), "d_x": _worst(got["d_x"], b["d_x"], b["A_d_x"]),
            "partials": _worst(got["partials"], b["partials"], b["A_partials"]),
            "d_gamma": _worst(tot[:80], b["d_gamma"], b["A_d_gamma"]), "d_beta": _worst(tot[80:], b["d_beta"], b["A_d_beta"])}


def exact_claims(regime, t, got):
    """what a regime promises exactly, beyond the bounds -> list of failures"""
    fails = []
    if regime == "dead":
        dead = torch.zeros(t["xn"].shape[0], dtype=torch.bool)
        dead[::DEAD_EVERY] = True
        if not torch.equal(got["sh"][dead], t["b2"].expand(int(dead.sum()), 12)):
            fails.append("sh of a point with every unit dead is not b2")
        for k in ("d_xn", "HID", "DH", "DT"):
            if bool((got[k][dead] != 0).any()):
                fails.append(f"{k} of a point with every unit dead is not zero")
        if bool((got["d_pf"][:, :, dead] != 0).any()):
            fails.append("d_pf of a point with every unit dead is not zero")
        if bool((got["HID"][:, DEAD_UNITS] != 0).any()) or bool((got["DH"][:, DEAD_UNITS] != 0).any()):
            fails.append("a dead unit is alive")
    if regime == "zero_dsh":
        for k in ("d_xn", "d_pf", "DH", "DT", "wgrad"):
            if bool((got[k] != 0).any()):
                fails.append(f"{k} is not zero for d_sh = 0")
    return fails


def ln_exact_claims(regime, t, got):
    fails = []
    if regime == "constant" and not torch.equal(got["xn"], t["beta"].expand_as(got["xn"])):
        fails.append("xn of a constant row is not beta")
    if regime == "constant" and not torch.equal(got["stats"][:, 0], t["x"][:, 0]):
        fails.append("the mean of a constant row is not its value")
    if regime == "gamma0" and not torch.equal(got["xn"][:, GAMMA0], t["beta"][GAMMA0].expand(got["xn"].shape[0], len(GAMMA0))):
        fails.append("xn of a column with gamma = 0 is not beta")
    return fails
