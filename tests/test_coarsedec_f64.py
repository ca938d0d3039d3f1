"""The fp64 stage reference of the coarse decoder (oracle/coarsedec_f64.py) and the cases built on it
(tests/coarsedec_cases.py), without a GPU.  What tests/test_coarsedec_f64_gpu.py then holds csrc/coarsedec.hip to rests on these:

  - with its roundings switched off the reference is `oracle/coarsedec_ref.forward_coarse(bf16=False)` and its autograd
    gradients (1e-6 of max), with them on its forward is `forward_coarse(bf16=True)` bit for bit on the exact cases, and it
    reproduces the reference project's own run of tests/golden/coarsedec_ref.npz; its `bf16()` is torch's conversion bit for bit;
  - every case contains what it claims: on the exact cases every operand is an integer and sum|terms| < 2^24 on 100 % of the
    elements of every per-row stage (of the weight gradients too, except at M = 66 000 and 131 205), more than 1 % of the
    pre-activations of h2 and of z are exact rounding ties, 30 - 70 % of the hidden units are dead, dz2 rounds;
  - a correct evaluation passes: torch fp32 matmuls with the same rounding points (the stand-in below, which imports nothing
    of lara_amd) passes every check the device gets, at every case.  Its worst |diff| / limit per tensor is printed: 0 on
    the exact cases (offset 0.08), on the ordinary ones 0.023 for dx and 0.067 for the weight gradients; the bf16 stages and
    the outputs come to 0.99 - 0.9999 there by construction (a correctly rounded value near a tie sits half an ulp from the
    unrounded reference, and half an ulp is the limit's leading term), so for them the bar is sharp from above and the
    mutations below are what shows that it bites;
  - the checks notice a wrong evaluation: seven mutations of the stand-in each fail the tensors they touch, and only those.
"""
import os

import numpy as np
import pytest
import torch

from oracle import coarsedec_f64 as cr
from oracle import coarsedec_ref
from tests import coarsedec_cases as cc

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coarsedec_ref.npz")
PARAMS = ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]
W_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


# ---------------------------------------------------------------------------------------------- the fp32 stand-in

def r32(x):
    return x.to(torch.bfloat16).float()


def trunc32(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def standin(case, t, mutation=None, prefill=None):
    """both entry points and the three weight-gradient products in torch fp32, rounding where the header says; `mutation`:
    one of the seven wrong evaluations of the mutation tests"""
    _, M, K, sh_dim = case
    n_par, Mp = K * (10 + sh_dim), cr.padded_rows(M)
    cols = cr.columns(K, sh_dim)
    w1, b1, w2, b2 = (r32(t[k]) for k in ("w1", "b1", "w2", "b2"))
    w3, b3 = torch.zeros(48, 80), torch.zeros(48)
    w3[:n_par], b3[:n_par] = r32(t["w3"]), (t["b3"] if mutation == "b3_unrounded" else r32(t["b3"]))

    def hidden(x, round2=r32):
        xb = r32(x)
        h1 = torch.relu(r32(xb @ w1.t() + b1))
        return xb, h1, torch.relu(round2(h1 @ w2.t() + b2))
    # the forward entry point
    x = t["x"]
    if mutation == "last_row_from_its_neighbour":
        x = x.clone()
        x[M - 1] = x[M - 2]
    round2 = trunc32 if mutation == "layer2_truncates" else r32
    z = r32(hidden(x, round2)[2] @ w3.t() + b3)
    if mutation == "opacity_scaling_swapped":
        z = z.clone()
        i, j = int(cols["opacity"][-1]), int(cols["scaling"][-2])
        z[:, [i, j]] = z[:, [j, i]]
    got = {"offset": 2.0 / (1.0 + torch.exp(-z[:, cols["offset"]])) - 1.0, "sh": z[:, cols["sh"]], "rotation": z[:, cols["rotation"]],
           "scaling": z[:, cols["scaling"]] + t["scaling_shift"], "opacity": z[:, cols["opacity"]] + t["opacity_shift"]}
    # the backward entry point
    xb, h1, h2 = hidden(t["x"], round2)
    g = torch.zeros(M, 48)
    for n, idx in cols.items():
        if t["g"][n] is not None and idx.numel():
            g[:, idx] = t["g"][n] * (0.5 * (1.0 - got["offset"] * got["offset"])) if n == "offset" else t["g"][n]
    dz3 = r32(g)
    dz2 = r32(dz3 @ w3) * (h2 > 0)
    dz1 = r32(dz2 @ w2) * ((h2 if mutation == "dz1_masked_by_h2" else h1) > 0)
    got["dx"] = dz1 @ w1

    def act_rows(a):        # rows M .. M_pad repeat row M - 1, as a kernel that clamps its row index leaves them
        full = torch.cat([a, a[-1:].expand(Mp - M, 80)])
        return torch.cat([full, torch.ones(Mp, 1), torch.zeros(Mp, 7)], 1)
    dz_rows = lambda a: torch.cat([a, torch.zeros(Mp - M, a.shape[1])])
    got.update(xb=act_rows(xb), h1=act_rows(h1), h2=act_rows(h2), dz1=dz_rows(dz1), dz2=dz_rows(dz2), dz3=dz_rows(dz3))
    if mutation == "dz2_pad_row_left":
        got["dz2"][Mp - 1, 3] = 0.5
    if mutation == "h1_without_ones":
        got["h1"][:, 80] = 0.0
    for i, (dz, act) in enumerate((("dz1", "xb"), ("dz2", "h1"), ("dz3", "h2")), 1):
        got[f"G{i}"] = got[dz].t() @ got[act] + (0.0 if prefill is None else prefill[f"G{i}"])
    assert all(v.dtype == torch.float32 for v in got.values())
    return got


@pytest.fixture(scope="module")
def worst():
    log = {}
    yield log
    for k in cc.TENSORS:
        vals = {c: v for (c, n), v in log.items() if n == k}
        if vals:
            c = max(vals, key=vals.get)
            print(f"\nfp32 stand-in: {k:9s} worst |diff| / limit = {vals[c]:.4f} ({c})", end="")


# ---------------------------------------------------------------------------------------------- the reference is the operator

def _rel(got, want):
    got, want = cr.f64(got).reshape(-1), cr.f64(want).reshape(-1)
    return float((got - want).abs().max() / max(float(want.abs().max()), 1e-12)) if want.numel() else 0.0


def _reference_run(t, K, sh_dim, on):
    """the unforced chain -> outputs, dx, [(dW, db)] * 3"""
    M = t["x"].shape[0]
    f = cr.forward(t, K, sh_dim, on=on)
    b = cr.backward(t, K, sh_dim, t["g"], f["out"]["offset"], f["h1"], f["h2"], on=on)
    n_par = K * (10 + sh_dim)
    grads = []
    for dz, act, rows in (("dz1", "xb", 80), ("dz2", "h1", 80), ("dz3", "h2", n_par)):
        G = cr.wgrad(b[dz], cr.with_ones(f[act], M))[0]
        grads += [G[:rows, :80], G[:rows, 80]]
    return f, b, grads


def _oracle_run(t, K, sh_dim, bf16):
    x = t["x"].clone().requires_grad_(True)
    ps = [t[k].clone().requires_grad_(True) for k in W_KEYS]
    res = coarsedec_ref.forward_coarse(x, *ps, K, sh_dim, t["opacity_shift"], t["scaling_shift"], bf16=bf16)
    loss = sum((r * t["g"][n].reshape(r.shape)).sum() for r, n in zip(res, cr.NAMES) if t["g"][n] is not None and r.numel())
    loss.backward()
    M = x.shape[0]
    return {n: r.detach().reshape(M, -1) for r, n in zip(res, cr.NAMES)}, x.grad, [p.grad for p in ps]


@pytest.mark.parametrize("case", [("default", 33, 4, 2), ("default", 129, 1, 0), ("zero_row", 129, 1, 27), ("default", 529, 2, 12)],
                         ids=cc.case_id)
def test_reference_without_roundings_is_the_fp32_oracle_and_its_autograd(case):
    t = cc.inputs(*case)
    f, b, grads = _reference_run(t, case[2], case[3], on=False)
    out, dx, pg = _oracle_run(t, case[2], case[3], bf16=False)
    for n in cr.NAMES:
        assert _rel(out[n], f["out"][n]) <= 1e-6, f"{n}: {_rel(out[n], f['out'][n]):.2e}"
    assert _rel(dx, b["dx"]) <= 1e-6, f"dx: {_rel(dx, b['dx']):.2e}"
    for k, got, want in zip(W_KEYS, pg, grads):
        assert _rel(got, want) <= 1e-6, f"grad {k}: {_rel(got, want):.2e}"


@pytest.mark.parametrize("case", [c for c in cc.EXACT_CASES if c[1] <= 529], ids=cc.case_id)
def test_reference_forward_is_the_bf16_oracle_bit_for_bit_on_exact_cases(case):
    t = cc.inputs(*case)
    f = cr.forward(t, case[2], case[3], exact=True)
    out, _, _ = _oracle_run(t, case[2], case[3], bf16=True)
    for n in ("sh", "scaling", "rotation", "opacity"):
        assert torch.equal(cr.f64(out[n]), f["out"][n]), n
    assert _rel(out["offset"], f["out"]["offset"]) <= 1e-6


@pytest.mark.parametrize("tag,on", [("fp32", False), ("bf16", True)])
def test_reference_reproduces_the_reference_fixture(tag, on):
    fx = np.load(FX)
    t = {k: torch.from_numpy(fx["p." + p]) for k, p in zip(W_KEYS, PARAMS)}
    t["x"] = torch.from_numpy(fx["feats"]).reshape(-1, 80)
    M = t["x"].shape[0]
    t.update(opacity_shift=float(fx["opacity_shift"]), scaling_shift=float(fx["scaling_shift"]),
             g={n: torch.from_numpy(fx["gout." + n]).reshape(M, -1) for n in cr.NAMES})
    f, b, grads = _reference_run(t, 2, 12, on=on)
    bar = 2e-2 if on else 1e-5
    for n in cr.NAMES:
        assert _rel(f["out"][n], fx[f"{tag}.{n}"]) <= bar, f"{tag} {n}: {_rel(f['out'][n], fx[f'{tag}.{n}']):.2e}"
    assert _rel(b["dx"], fx[f"{tag}.d_feats"]) <= bar, f"{tag} d_feats: {_rel(b['dx'], fx[f'{tag}.d_feats']):.2e}"
    for p, got in zip(PARAMS, grads):
        assert _rel(got, fx[f"{tag}.g.{p}"]) <= bar, f"{tag} grad {p}: {_rel(got, fx[f'{tag}.g.{p}']):.2e}"
    if on:
        same = float((f["out"]["sh"].reshape(-1) == cr.f64(fx["bf16.sh"]).reshape(-1)).double().mean())
        assert same >= 0.97, same


def test_bf16_is_torchs_conversion_bit_for_bit():
    f32 = torch.float32
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, 255.0, 256.0, 257.0, 258.0, 259.0, 3.3895313892515355e38, 3.3961775292304601e38,
                            -3.3961775292304601e38, 3.4028234663852886e38, 1e-40, -1e-40, 9.1835e-41, 4.5918e-41, 1.4e-45,
                            1.1754943508222875e-38, float("inf"), -float("inf")], dtype=f32)
    k = torch.arange(64, dtype=f32)
    ties = torch.cat([1.0 + (k + 0.5) * 2.0 ** -7, 2.0 - (k + 0.5) * 2.0 ** -8, 256.0 + 2 * k + 1, 512.0 - (2 * k + 1),   # both parities, a binade border
                      torch.arange(1, 200, dtype=f32) * 2.0 ** -134])                                                  # subnormal ties
    rnd = (torch.randn(4096, generator=torch.Generator().manual_seed(3)) * torch.logspace(-30, 30, 4096)).to(f32)
    v = torch.cat([special, ties, -ties, rnd])
    want, got = v.to(torch.bfloat16).to(f32), cr.bf16(v).to(f32)
    assert torch.equal(want.view(torch.int32), got.view(torch.int32))
    assert bool(torch.isnan(cr.bf16(torch.tensor([float("nan")]))).all())
    # the spacing: one ulp above a bf16 number is the next one
    b = want[torch.isfinite(want) & (want.abs() < 1e38)].double()
    nxt = b.abs() + cr.ulp_bf16(b)
    assert torch.equal(cr.bf16(nxt), nxt) and torch.equal(cr.bf16(b.abs() + 0.49 * cr.ulp_bf16(b)), b.abs())


# ---------------------------------------------------------------------------------------------- the cases

def test_sizes_cover_the_mechanisms():
    assert all(K * (10 + s) <= 48 for K, s in cc.KS) and {K * (10 + s) for K, s in cc.KS} >= {48, 44, 10}
    assert {(c[2], c[3]) for c in cc.EXACT_CASES if c[1] == 129} == set(cc.KS)
    assert {c[1] for c in cc.EXACT_CASES} >= {1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 66000, cc.LARGE}
    trips = lambda M: -(-M // 128)
    assert 512 < trips(66000) < 1024 and trips(cc.LARGE) == 1026 and cc.LARGE % 128 == 5
    assert [cr.padded_rows(M) for M in (0, 1, 128, 129)] == [0, 128, 128, 256]
    for K, s in cc.KS:
        idx = torch.cat(list(cr.columns(K, s).values()))
        assert sorted(idx.tolist()) == list(range(K * (10 + s)))


@pytest.mark.parametrize("case", cc.EXACT_CASES, ids=cc.case_id)
def test_exact_case_is_exact_and_contains_what_it_claims(case):
    _, M, K, sh_dim = case
    t = cc.inputs(*case)
    assert all(t[k].dtype == torch.float32 for k in ("x",) + W_KEYS) and t["g"]["offset"] is None
    res, f, b = cc.exactness(case, t)
    for k, (S, whole) in res.items():
        assert whole, f"{k}: an operand is no integer"
        if not (k.startswith("G") and M > 1000):
            assert S < 2.0 ** 24, f"{k}: sum|terms| reaches {S:.3e}"
    print(f"{cc.case_id(case)}: largest sum|terms| " + ", ".join(f"{k} {S:.3g}" for k, (S, _) in res.items()))
    if M < 31:
        return

    def tie_share(pre):
        r = cr.bf16(pre)
        return float(((r != pre) & ((r - pre).abs() == cr.ulp_bf16(pre) / 2)).double().mean())
    n_par = K * (10 + sh_dim)
    assert tie_share(f["pre2"]) > 0.01 and tie_share(f["z_pre"][:, :n_par]) > 0.01
    assert float((cr.bf16(f["z_pre"]) != f["z_pre"])[:, :n_par].double().mean()) > 0.3
    for k in ("h1", "h2"):
        assert 0.3 < float((f[k] == 0).double().mean()) < 0.7, k
    live = b["dz2_pre"] != 0
    if n_par > 10:      # (seven gradient columns of at most 40 * 2 each seldom reach 256)
        assert float((cr.bf16(b["dz2_pre"]) != b["dz2_pre"])[live].double().mean()) > 0.01, "dz2 never rounds"


@pytest.mark.parametrize("case", cc.ORDINARY_CASES, ids=cc.case_id)
def test_ordinary_case_contains_what_it_claims(case):
    regime, M, K, sh_dim = case
    t = cc.inputs(*case)
    f = cr.forward(t, K, sh_dim)
    o32 = f["out"]["offset"].float()
    if regime == "default":
        assert float(f["out"]["scaling"].abs().max()) > 4 and not bool((o32.abs() == 1).any())
    if regime == "saturated":
        assert float((o32.abs() == 1).double().mean()) > 0.005 and float((o32.abs() < 1).double().mean()) > 0.02
    if regime == "zero_row":
        assert not t["x"][0].any() and not t["x"][M - 1].any()
    if regime == "dead_layer":
        assert not f["h1"].any() and float(f["A_pre2"].max()) == 0 and torch.equal(f["h2"], torch.relu(cr.bf16(t["b2"])).expand(M, 80))


# ---------------------------------------------------------------------------------------------- the reference inside its own bar

@pytest.mark.parametrize("case", cc.CASES, ids=cc.case_id)
def test_fp32_standin_passes_every_check(case, worst):
    t = cc.inputs(*case)
    got = standin(case, t)
    res = cc.check(case, t, got)
    worst.update({(cc.case_id(case), k): v for k, v in res.items()})
    bad = {k: round(v, 3) for k, v in res.items() if not v <= 1.0}
    assert set(res) == set(cc.TENSORS) and not bad, f"a correct fp32 evaluation fails the reference's bound: {bad}"
    assert not cc.exact_claims(case, t, got)
    if case[0] == "exact":
        assert all(v == 0.0 for k, v in res.items() if k != "offset" and not (k.startswith("G") and case[1] > 1000)), res


def test_fp32_standin_passes_with_a_prefilled_destination():
    case = ("default", 529, 2, 12)
    t = cc.inputs(*case)
    g = torch.Generator().manual_seed(5)
    prefill = {"G1": torch.randn(80, 88, generator=g) * 30, "G2": torch.randn(80, 88, generator=g) * 30, "G3": torch.randn(48, 88, generator=g) * 30}
    res = cc.check(case, t, standin(case, t, prefill=prefill), prefill=prefill)
    assert all(v <= 1.0 for v in res.values()), res
    res = cc.check(case, t, standin(case, t), prefill=prefill)
    assert all(res[k] > 1.0 for k in ("G1", "G2", "G3")), "a product that overwrites its destination passes"


# ---------------------------------------------------------------------------------------------- mutation checks

OUTPUTS = set(cr.NAMES)
MUTATIONS = [("layer2_truncates", {"h2"}), ("b3_unrounded", OUTPUTS), ("opacity_scaling_swapped", {"opacity", "scaling"}),
             ("last_row_from_its_neighbour", OUTPUTS), ("dz2_pad_row_left", {"dz2"}), ("dz1_masked_by_h2", {"dz1"}),
             ("h1_without_ones", {"h1"})]


@pytest.mark.parametrize("case", [("default", 529, 2, 12), ("exact", 129, 2, 12)], ids=cc.case_id)
@pytest.mark.parametrize("mutation,touched", MUTATIONS, ids=[m for m, _ in MUTATIONS])
def test_mutation_fails_the_tensors_it_touches_and_only_those(case, mutation, touched):
    """(a) truncation in layer 2, (b) b3 not rounded, (c) the opacity column swapped with the first scaling column of the last
    k, (d) the forward's row M - 1 computed from row M - 2's input, (e) a dz2 pad row left non-zero, (f) dz1 masked by h2,
    (g) h1 without its column of ones.  On the ordinary case every later stage is forced from the arrays under test, so a
    wrong stage fails alone; on the exact case the reference's own chain is the bar and everything behind the wrong stage
    fails with it (b3 holds integers there: nothing to round)."""
    t = cc.inputs(*case)
    res = cc.check(case, t, standin(case, t, mutation=mutation))
    if case[0] == "exact":
        if mutation == "b3_unrounded":
            assert all(v <= 1.0 for v in res.values())
            return
        behind = {"layer2_truncates": {"h2", "G3"} | OUTPUTS, "dz1_masked_by_h2": {"dz1", "dx", "G1"},     # (truncation keeps the ReLU masks)
                  "dz2_pad_row_left": {"dz2", "G2"}, "h1_without_ones": {"h1", "G2"}}
        touched = behind.get(mutation, touched)
    assert all(res[k] > 1.0 for k in touched), {k: res[k] for k in touched}
    rest = {k: v for k, v in res.items() if k not in touched}
    assert all(v <= 1.0 for v in rest.values()), {k: v for k, v in rest.items() if v > 1.0}
