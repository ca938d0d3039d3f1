"""The fp64 reference of the fine decoder (oracle/finedec_f64.py) and the cases built on it (tests/finedec_cases.py), without a
GPU.  What tests/test_finedec_f64_gpu.py then holds csrc/finedec.hip to rests on these:

  - with float32 inputs the reference reproduces `forward_fine_folded` plus autograd, and on the 700 rows of
    tests/golden/finedec_ref.npz the reference project's own output and gradients, at that file's existing bars;
  - every case meets the kink condition and every regime contains what it claims;
  - the reference alone stays inside its own bar: the same algebra evaluated in fp32 on the CPU (the stand-in: `forward_fine_folded`
    and autograd, restated line by line so that U, HID, DH = the gradient at the pre-activation and DT = the gradient at t can
    be read off, and asserted bit for bit equal to the original; a numpy fp32 LayerNorm; slab-wise fp32 weight gradients)
    passes exactly the checks the device gets, at every case.  The largest |diff| / limit of the stand-in is 0.218 (xn
    recomputed from its own stats, ordinary rows, n = 131205); of the decoder 0.089 (DH, n = 131205); no bound lacked a term;
  - the checks notice a wrong evaluation: three mutations of the reference each fail the tensors they touch, and only those.
"""
import os

import numpy as np
import pytest
import torch

from oracle import finedec_f64 as fr
from oracle.finedec_ref import FineDecoderRef, forward_fine_folded
from tests import finedec_cases as fc

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finedec_ref.npz")
W_KEYS = ("Wqk", "W1ov", "b1", "W2", "b2")
PARAMS = ["norm.weight", "norm.bias", "cross_att.q_proj_weight", "cross_att.k_proj_weight", "cross_att.v_proj_weight",
          "cross_att.out_proj.weight", "mlp_fine.0.weight", "mlp_fine.0.bias", "mlp_fine.2.weight", "mlp_fine.2.bias"]


# ---------------------------------------------------------------------------------------------- the fp32 stand-in

def slabwise_wgrad(xn, Um, HIDm, DH, DT, d_sh):
    """the five weight gradients in fp32: one product per 512-row slab, the slabs added in order"""
    out = torch.zeros(fr.fine_wgrad_floats())
    for r0 in range(0, xn.shape[0], fr.SLAB):
        s = slice(r0, r0 + fr.SLAB)
        out = out + torch.cat([(DT[s].t() @ xn[s]).reshape(-1), (DH[s].t() @ Um[s]).reshape(-1), DH[s].sum(0),
                               (d_sh[s].t() @ HIDm[s]).reshape(-1), d_sh[s].sum(0)])
    return out


def standin_decoder(t):
    """`forward_fine_folded` and autograd in fp32, with the intermediates the device hands out"""
    xn, pf, Wqk, W1ov, b1, W2, b2 = a = [t[k].clone().requires_grad_(True) for k in ("xn", "pf") + W_KEYS]
    n = xn.shape[0]
    tq = xn @ Wqk.t()
    v = pf.permute(2, 0, 1)
    p = torch.softmax(torch.einsum("nhc,njc->nhj", tq.view(n, 8, 8), v), dim=-1)
    u = torch.einsum("nhj,njc->nhc", p, v).reshape(n, 64)
    pre = u @ W1ov.t() + b1
    hid = torch.relu(pre)
    sh = hid @ W2.t() + b2
    for x in (tq, pre):
        x.retain_grad()
    (sh * t["d_sh"]).sum().backward()
    b = [t[k].clone().requires_grad_(True) for k in ("xn", "pf") + W_KEYS]
    ref = forward_fine_folded(*b)
    (ref * t["d_sh"]).sum().backward()
    assert torch.equal(sh, ref) and all(torch.equal(x.grad, y.grad) for x, y in zip(a, b)), "the stand-in is not forward_fine_folded"
    got = {"sh": sh.detach(), "d_xn": xn.grad, "d_pf": pf.grad, "U": u.detach(), "HID": hid.detach(), "DH": pre.grad, "DT": tq.grad}
    got["wgrad"] = slabwise_wgrad(t["xn"], got["U"], got["HID"], got["DH"], got["DT"], t["d_sh"])
    return got, torch.cat([w.grad.reshape(-1) for w in (Wqk, W1ov, b1, W2, b2)])


def standin_ln(t):
    """the LayerNorm and its backward in numpy fp32"""
    x, gamma, beta, d = (t[k].numpy() for k in ("x", "gamma", "beta", "d_xn"))
    f32, n = np.float32, x.shape[0]
    mean = x.mean(1, dtype=f32, keepdims=True)
    c = x - mean
    rstd = (f32(1) / np.sqrt((c * c).mean(1, dtype=f32, keepdims=True) + f32(fc.LN_EPS))).astype(f32)
    xn = c * rstd * gamma + beta
    xh = c * rstd
    g = d * gamma
    m1, m2 = g.mean(1, dtype=f32, keepdims=True), (g * xh).mean(1, dtype=f32, keepdims=True)
    dx = rstd * (g - m1 - xh * m2)
    blocks = fr.fine_ln_blocks(n)
    parts = np.stack([np.concatenate([(d * xh)[k * 256:(k + 1) * 256].sum(0, dtype=f32), d[k * 256:(k + 1) * 256].sum(0, dtype=f32)])
                      for k in range(blocks)])
    out = {"xn": xn, "stats": np.concatenate([mean, rstd], 1), "d_x": dx, "partials": parts}
    assert all(v.dtype == f32 for v in out.values())
    return {k: torch.from_numpy(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def worst():
    log = {}
    yield log
    if log:
        k = max(log, key=log.get)
        print(f"\nfp32 stand-in: largest |diff| / limit = {log[k]:.3f} ({k})")


# ---------------------------------------------------------------------------------------------- the reference is the operator

def _rel(got, want):
    got, want = fr.f64(got), fr.f64(want)
    return float((got - want).abs().max() / max(float(want.abs().max()), 1e-12))


@pytest.mark.parametrize("case", [("ordinary", 257), ("ordinary", 1025), ("ties", 129)], ids=fc.case_id)
def test_reference_reproduces_forward_fine_folded_and_autograd(case):
    """no forcing: values, input gradients and all five weight gradients, to the fp32 evaluation's own precision"""
    t = fc.inputs(*case)
    got, wg = standin_decoder(t)
    r = fr.fine_decoder_backward(*(t[k] for k in ("xn", "pf") + W_KEYS), t["d_sh"])
    for k in ("sh", "d_xn", "d_pf", "U", "HID", "DH", "DT"):
        assert _rel(got[k], r[k]) <= 2e-5, f"{k}: {_rel(got[k], r[k]):.2e}"
    ref, _ = fr.fine_decoder_wgrad(case[1], t["xn"], r["U"], r["HID"], r["DH"], r["DT"], t["d_sh"])
    for k, v in fr.split_wgrad(ref).items():
        assert _rel(fr.split_wgrad(wg)[k], v) <= 1e-4, f"{k}: {_rel(fr.split_wgrad(wg)[k], v):.2e}"


def test_reference_reproduces_the_reference_fixture():
    """LayerNorm + decoder + both backwards + weight gradients on the fixture's 700 rows, at tests/test_finedec.py's bars:
    2e-5 max|ref| for the output and the input gradients, 1e-4 max|ref| for the ten parameter gradients"""
    from lara_amd.fine import _fold_fine_weights
    fx = np.load(FX)
    dec = FineDecoderRef.from_fixture(fx)
    folded = _fold_fine_weights(dec)
    W = [w.detach() for w in folded]
    vol, pf, gout = torch.from_numpy(fx["vol"]), torch.from_numpy(fx["pf_planar"]), torch.from_numpy(fx["gout"]).reshape(-1, 12)
    eps = float(torch.tensor(dec.norm.eps, dtype=torch.float32))
    ln = fr.fine_ln_forward(vol, dec.norm.weight, dec.norm.bias, eps)
    r = fr.fine_decoder_backward(ln["xn"], pf, *W, gout)
    lb = fr.fine_ln_backward(vol, dec.norm.weight, ln["stats"], r["d_xn"])
    assert _rel(r["sh"], fx["sh"].reshape(-1, 12)) <= 2e-5
    assert _rel(lb["d_x"], fx["d_vol"]) <= 2e-5
    assert _rel(r["d_pf"], fx["d_pf_planar"]) <= 2e-5
    wg, _ = fr.fine_decoder_wgrad(700, ln["xn"], r["U"], r["HID"], r["DH"], r["DT"], gout)
    torch.autograd.backward(list(folded), [g.float() for g in fr.split_wgrad(wg).values()])
    grads = {k: p.grad for k, p in dec.named_parameters()}
    grads["norm.weight"], grads["norm.bias"] = lb["d_gamma"], lb["d_beta"]
    for k in PARAMS:
        assert _rel(grads[k], fx["g." + k]) <= 1e-4, f"grad {k}: {_rel(grads[k], fx['g.' + k]):.2e}"


# ---------------------------------------------------------------------------------------------- the cases

def test_sizes_cover_the_mechanisms():
    n = set(fc.SIZES)
    assert {1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 527, 529, 4096} <= n
    assert {fr.fine_wgrad_slabs(k) for k in n} >= set(range(1, 10)) | {13, 257}          # every phase and chain of the reduce
    assert -(-fc.LARGE // 128) == 1024 + 2 and fr.fine_wgrad_slabs(fc.LARGE) == 257 and fr.fine_ln_blocks(fc.LARGE) == 513
    assert [c for c in fc.CASES if c[1] == fc.LARGE] == [("ordinary", fc.LARGE)]
    assert all((r, k) in fc.CASES for r in fc.REGIMES for k in (129, 529))


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_case_meets_the_kink_condition_and_contains_what_it_claims(case):
    regime, n = case
    t = fc.inputs(*case)
    f = fc.pure_forward(t)
    assert not fc.on_kink(f).any()
    assert float((f["PRE"].abs() / f["A_PRE"]).min()) > fc.KINK
    assert all(v.dtype == torch.float32 for v in t.values())
    s, gap, P = f["s"], f["gap"], f["P"]
    if regime == "ordinary":
        assert float(s.max()) < 88
    if regime == "saturated":
        assert float(s.max()) > 88 and float(gap.max()) > 104
        assert int((P < fr.TINY).sum()) > 0 and int((P > 1 - 1e-9).sum()) > 0, "flushed terms and P = 1"
        fp32 = torch.softmax(s.float(), -1)
        assert int((fp32 == 0).sum()) > 0 and int((fp32 == 1).sum()) > 0
    if regime == "ties":
        third = torch.arange(n) % 3
        assert torch.equal(P[third == 0], torch.full_like(P[third == 0], 0.25))
        two = gap[third == 1]
        assert torch.equal(two[..., 1], two[..., 3])
        assert int(((two[..., 1] == 0) & (two[..., 3] == 0)).sum()) >= two.shape[0], "two equal maximal views"
    if regime == "dead":
        dead = torch.zeros(n, dtype=torch.bool)
        dead[::fc.DEAD_EVERY] = True
        assert float(f["PRE"][:, fc.DEAD_UNITS].max()) < -100 and float(f["PRE"][dead].max()) < -100
        assert float((f["HID"][~dead] > 0).any(-1).float().mean()) > 0.9, "the other points keep live units"
        assert torch.equal(f["sh"][dead], fr.f64(t["b2"]).expand(int(dead.sum()), 12)) and float(f["A_sh"][dead].max()) == 0
    if regime == "zero_dsh":
        assert not t["d_sh"].any()
        r = fr.fine_decoder_backward(*(t[k] for k in ("xn", "pf") + W_KEYS), t["d_sh"])
        assert all(not r[k].any() and not r["A_" + k].any() for k in ("DH", "DT", "d_xn", "d_pf"))


@pytest.mark.parametrize("case", fc.LN_CASES, ids=fc.case_id)
def test_layernorm_case_contains_what_it_claims(case):
    regime, n = case
    t = fc.ln_inputs(*case)
    x = t["x"]
    f = fr.fine_ln_forward(x, t["gamma"], t["beta"], fc.LN_EPS)
    if regime == "constant":
        assert torch.equal(x, x[:, :1].expand_as(x)) and torch.equal(x * 8, (x * 8).round())
        assert torch.equal(f["xn"], fr.f64(t["beta"]).expand_as(f["xn"]))
        assert torch.equal(f["stats"][:, 1], torch.full((n,), fc.LN_EPS, dtype=torch.float64).rsqrt())
    if regime == "offset":
        assert float(x.min()) > 990 and 0.5 < float(x.std(1).mean()) < 1.5
    if regime == "outlier":
        assert bool(((x == 1e4).sum(1) == 1).all())
    if regime == "gamma0":
        assert int((t["gamma"] == 0).sum()) == 8


# ---------------------------------------------------------------------------------------------- the reference inside its own bar

@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_fp32_standin_passes_the_decoder_checks(case, worst):
    t = fc.inputs(*case)
    got, _ = standin_decoder(t)
    res = fc.check_decoder(t, got)
    worst.update({f"{fc.case_id(case)}/{k}": v for k, v in res.items()})
    bad = {k: round(v, 3) for k, v in res.items() if not v <= 1.0}
    assert not bad, f"a correct fp32 evaluation fails the reference's bound: {bad}"
    assert not fc.exact_claims(case[0], t, got)


@pytest.mark.parametrize("case", fc.LN_CASES, ids=fc.case_id)
def test_fp32_standin_passes_the_layernorm_checks(case, worst):
    t = fc.ln_inputs(*case)
    got = standin_ln(t)
    res = fc.check_ln(t, got)
    worst.update({f"ln-{fc.case_id(case)}/{k}": v for k, v in res.items()})
    bad = {k: round(v, 3) for k, v in res.items() if not v <= 1.0}
    assert not bad, f"a correct fp32 evaluation fails the reference's bound: {bad}"
    assert not fc.ln_exact_claims(case[0], t, got)


# ---------------------------------------------------------------------------------------------- mutation checks

def _touched(res, touched):
    """the touched tensors fail, every other tensor still passes"""
    names = [k for k in res if not k.startswith("wgrad.")]
    assert all(res[k] > 1.0 for k in touched), {k: res[k] for k in touched}
    assert all(res[k] <= 1.0 for k in names if k not in touched), {k: res[k] for k in names if k not in touched}


def test_mutation_swapped_softmax_weights_fail():
    """two views' weights swapped for one head of one point: U, sh, DT, d_pf fail (HID, DH, d_xn and the weight gradients are
    forced from the arrays under test and stay)"""
    t = fc.inputs("ordinary", 529)
    got, _ = standin_decoder(t)
    att = dict(fr.fine_decoder_attention(t["xn"], t["pf"], t["Wqk"]))
    P = att["P"].clone()
    i, h = divmod(int((P[..., 0] - P[..., 1]).abs().argmax()), 8)
    P[i, h, 0], P[i, h, 1] = att["P"][i, h, 1], att["P"][i, h, 0]
    att["P"] = P
    att["U"] = torch.einsum("nhj,njc->nhc", P, fr.f64(t["pf"]).permute(2, 0, 1)).reshape(529, 64)
    _touched(fc.check_decoder(t, got, att=att), ("U", "sh", "DT", "d_pf"))


def test_mutation_zeroed_wqk_column_fails():
    """column 79 of Wqk zeroed: t changes, and with it U, sh, DT, d_pf; d_xn loses its column 79"""
    t = dict(fc.inputs("ordinary", 529))
    got, _ = standin_decoder(t)
    t["Wqk"] = t["Wqk"].clone()
    t["Wqk"][:, 79] = 0
    _touched(fc.check_decoder(t, got), ("U", "sh", "DT", "d_pf", "d_xn"))


def test_mutation_row_left_out_of_a_slab_fails():
    """row 520 (the ninth of the second slab's seventeen) left out at n = 529: all five weight gradients fail, nothing else"""
    t = fc.inputs("ordinary", 529)
    got, _ = standin_decoder(t)
    res = fc.check_decoder(t, got, drop_row=520)
    _touched(res, ("wgrad",))
    assert all(res["wgrad." + k] > 1.0 for k, _ in fr.WGRAD_PARTS), res
