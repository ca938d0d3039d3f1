"""The two kernels of csrc/coarsedec.hip and the three weight-gradient products behind them, through the C ABI only
(`lara_amd._native.call` and `query`; one test through `lara_amd.coarse.forward_coarse`), against the fp64 stage reference
(oracle/coarsedec_f64.py) at the cases of tests/coarsedec_cases.py.  tests/test_coarsedec_f64.py shows, without a GPU, that
the reference is the operator, that every case contains what it claims, that a correct fp32 evaluation passes every check
below and that seven wrong ones do not.

Element by element, nothing exempted, no percentile (the rules and the derivations are in the reference's docstring):
    fp32 stages (dx, G1..G3)            |got - ref| <= 4 A + 2^-23 |ref|
    bf16 stages (h1, h2, dz3, dz2, dz1) |got - ref| <= 4 A + ulp_bf16(|ref| + 4 A) / 2 + 2^-126, ref the unrounded fp64 value
    the five outputs                    the bf16 stage z and the fp32 operation behind it together
    A = 0                               the value is determined and must be met exactly (-0 = 0); xb = bf16(x) always
each stage recomputed from the device's own arrays of the stage in front of it (h1 from xb, h2 from h1, the outputs from h2 of
the backward call on the same inputs, dz3 from the gradients and the offset output handed in, dz2 from dz3 and the mask h2 > 0,
dz1 from dz2 and h1 > 0, dx from dz1, G_l from the device's factor pair, all M_pad rows).  On the exact cases (integer operands)
the reference's own unforced chain is the bar and every array equals it bit for bit; only offset = 2 sigmoid(z) - 1 (no
integer: held to its activation's bound at the exact z) and the weight gradients at M = 66 000 and 131 205 (sum|terms| beyond
2^24: held to their bound) are not bit comparisons there.

Every output and every factor matrix sits NaN-filled (0xFFFF-filled for the bf16 matrices) between two 64-element guards in
every run of this file: all of it written, no guard touched.  Rows M .. M_pad of dz1, dz2, dz3 are zero, of xb, h1, h2 finite
with the column of ones; columns 81..87 are zero, columns >= K (10 + sh_dim) of dz3 are zero.

Every worst |diff| / limit, per tensor and case, goes to coarsedec_f64_errors.json in the directory LARA2DGS_TEST_OUT names
(default: test_out/ in the repository root, kept out of git).

Measured on an MI355X (first clean run: 83 exact and 11 ordinary cases, and the interface tests; every test passed on the
kernels as they were -- these cases found no defect in csrc/coarsedec.hip or lara_amd/coarse.py).
Exact cases: every figure 0, i.e. all five outputs but offset, the six factor matrices, dx and G1..G3 equal the reference as
bits at every M and (K, sh_dim), the weight gradients at M = 66 000 and 131 205 included (their sum|terms| passes 2^24, the
partial sums the device forms do not); offset 0.083 of its activation's bound at worst.
Ordinary cases, worst |diff| / limit: dx 0.016 (default, M = 66 000); G1 0.054, G2 0.100, G3 0.129 (K = M_pad against sums
that round like random walks).  The bf16 stages and the outputs come to 0.99 - 0.9999 (h1 0.991, h2 0.997, dz3 0.9999, dz2 0.9994,
dz1 0.996, offset 0.993, sh 0.995, scaling 0.995, rotation 0.996, opacity 0.995): by construction, since a correctly rounded
value near a tie sits half an ulp from the unrounded reference and half an ulp is the limit's leading term; the fp32 CPU
stand-in of tests/test_coarsedec_f64.py lands on the same figures.  What tells evaluations apart there is the share of
elements that are not the reference's fp64 value rounded (logged per case): at most 9.7e-5 (dz2, dz1 at M = 129: one element
each), 1.6e-5 (h1), 7e-6 (h2), 1.2e-5 (z) at M = 131 205 -- each a sum within a few 2^-24 of a rounding tie; 0 on every
exact case.
The forward's and the backward's hidden layers are bit-identical: test_forward_and_backward_kernels_compute_the_same_hidden_layers
reads the forward kernel's h2 out through a selecting last layer and finds all 529 x 80 values equal to the backward's, so
the outputs are held to the device's h2 of the backward call, with no tie term.
"""
import json
import os

import pytest
import torch

from lara_amd import _native
from lara_amd._native import call, query
from oracle import coarsedec_f64 as cr
from tests import coarsedec_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
E_INVALID = -1
W_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")
ORD = ("default", 529, 2, 12)
_LOG, _FLIPS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    if not _LOG:
        return
    out = os.environ.get("LARA2DGS_TEST_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_out")
    os.makedirs(out, exist_ok=True)
    per_tensor = {}
    for key, v in _LOG.items():
        name = key.split("/", 1)[1]
        if v > per_tensor.get(name, (-1.0, ""))[0]:
            per_tensor[name] = (v, key)
    with open(os.path.join(out, "coarsedec_f64_errors.json"), "w") as f:
        json.dump({"max_diff_over_limit": max(_LOG.values()), "per_tensor": {k: {"worst": v, "at": at} for k, (v, at) in per_tensor.items()},
                   "worst_diff_over_limit": _LOG, "share_not_the_rounded_fp64_value": _FLIPS}, f, indent=1)


# ---------------------------------------------------------------------------------------------- device plumbing

def _guarded(shape, dtype=torch.float32):
    """a contiguous tensor of `shape` inside a NaN-filled (bf16: 0xFFFF-filled) buffer -> (tensor, whole buffer)"""
    k = torch.Size(shape).numel()
    if dtype == torch.float32:
        whole = torch.full((GUARD + k + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    else:
        whole = torch.full((GUARD + k + GUARD,), -1, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return whole[GUARD:GUARD + k].view(shape), whole


def _guards_intact(whole, k):
    if whole.dtype == torch.float32:
        return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + k:]).all())
    bits = whole.view(torch.int16)
    return bool((bits[:GUARD] == -1).all()) and bool((bits[GUARD + k:] == -1).all())


def _written_inside(name, tensor, whole):
    assert bool(torch.isfinite(tensor.float()).all()), f"{name}: elements left unwritten (or not finite)"
    assert _guards_intact(whole, tensor.numel()), f"{name}: written outside the tensor"


def _untouched(name, tensor, whole):
    assert bool(torch.isnan(tensor.float()).all()) and _guards_intact(whole, tensor.numel()), f"{name}: written by a refused call"


def _buffers(M, K, sh_dim):
    Mp = query("lara_coarse_decoder_padded_rows", M)
    assert Mp == cr.padded_rows(M)
    bufs = {n: _guarded((M, K * w)) for n, w in cr.widths(sh_dim).items()}
    bufs["dx"] = _guarded((M, 80))
    bufs.update({n: _guarded((Mp, c), torch.bfloat16) for n, c in cr.FACTORS})
    return bufs, Mp


def run(case, t, prefill=None):
    """both entry points and the three products of lara_gemm_tn_bf16 on one case, every output guarded -> {name: CPU fp32}.
    The offset output of the forward call is the `offset_out` of the backward call; without an offset gradient it is NULL."""
    _, M, K, sh_dim = case
    d = {k: t[k].to(DEV).contiguous() for k in ("x",) + W_KEYS}
    g = {n: (None if v is None or not v.numel() else v.to(DEV).contiguous()) for n, v in t["g"].items()}
    bufs, Mp = _buffers(M, K, sh_dim)
    out = {n: (bufs[n][0] if bufs[n][0].numel() else None) for n in cr.NAMES}        # sh_dim = 0: sh = NULL
    call("lara_coarse_decoder_forward", DEV, M, K, sh_dim, d["x"], *(d[k] for k in W_KEYS), float(t["opacity_shift"]),
         float(t["scaling_shift"]), *(out[n] for n in cr.NAMES))
    call("lara_coarse_decoder_backward", DEV, M, K, sh_dim, d["x"], *(d[k] for k in W_KEYS[:5]),
         out["offset"] if g["offset"] is not None else None, *(g[n] for n in cr.NAMES), bufs["dx"][0],
         *(bufs[n][0] for n, _ in cr.FACTORS))
    ws = torch.empty(max(query("lara_gemm_tn_workspace_bytes"), 16), dtype=torch.uint8, device=DEV)
    for i, (dz, act) in enumerate((("dz1", "xb"), ("dz2", "h1"), ("dz3", "h2")), 1):
        G = bufs[f"G{i}"] = _guarded((bufs[dz][0].shape[1], 88))
        G[0].copy_(prefill[f"G{i}"]) if prefill is not None else G[0].zero_()
        call("lara_gemm_tn_bf16", DEV, Mp, bufs[dz][0].shape[1], 88, bufs[dz][0], bufs[act][0], G[0], ws)
    torch.cuda.synchronize()
    for k, (x, whole) in bufs.items():
        _written_inside(k, x, whole)
    return {k: x.float().cpu() for k, (x, _) in bufs.items()}


def _record(prefix, res):
    for k, v in res.items():
        _LOG[f"{prefix}/{k}"] = v
        print(f"{prefix + '/' + k:40s} worst |diff| / limit = {v:.4f}")
    return [f"{k}: worst |diff| / limit = {v:.3f}" for k, v in res.items() if not v <= 1.0]


def _same(a, b, what, keys=None):
    for k in keys or a:
        assert torch.equal(a[k], b[k]), f"{k}: {what}"


def _rc(name, *args):
    """the entry point's return code itself (`call` raises on every non-zero one)"""
    a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args] + [_native.current_stream(torch.device(DEV))]
    with torch.cuda.device(DEV):
        return getattr(_native.load_library(), name)(*a)


# ---------------------------------------------------------------------------------------------- the tests

def test_padded_rows(hip_lib):
    assert [query("lara_coarse_decoder_padded_rows", M) for M in (0, 1, 128, 129)] == [0, 128, 128, 256]


@pytest.mark.parametrize("case", cc.EXACT_CASES, ids=cc.case_id)
def test_exact_cases_bit_for_bit(hip_lib, case):
    """integer operands: the five outputs (offset: within its activation's bound), the six factor matrices, dx and G1..G3
    (M > 1000: within their bound) equal the reference's own chain as bits"""
    t = cc.inputs(*case)
    got = run(case, t)
    res = cc.check(case, t, got)
    fails = _record(cc.case_id(case), res) + cc.exact_claims(case, t, got)
    assert not fails, "; ".join(fails)
    inexact = {"offset"} | ({"G1", "G2", "G3"} if case[1] > 1000 else set())
    assert all(v == 0.0 for k, v in res.items() if k not in inexact), {k: v for k, v in res.items() if v}


@pytest.mark.parametrize("case", cc.ORDINARY_CASES, ids=cc.case_id)
def test_ordinary_cases_element_by_element(hip_lib, case):
    t = cc.inputs(*case)
    got = run(case, t)
    flips = {}
    fails = _record(cc.case_id(case), cc.check(case, t, got, flips=flips)) + cc.exact_claims(case, t, got)
    _FLIPS[cc.case_id(case)] = flips
    print(cc.case_id(case), "share of elements that are not the rounded fp64 value:", {k: round(v, 5) for k, v in flips.items()})
    assert not fails, "; ".join(fails)


def test_forward_and_backward_kernels_compute_the_same_hidden_layers(hip_lib):
    """The forward hands out no hidden layer; a last layer that selects (W3 = rows of the identity, b3 = 0, shifts 0) does:
    z = bf16(1 * h2[unit]) = h2[unit] exactly, on every column without an activation.  Three selections cover the 80 units;
    the forward kernel's h2 must be the backward kernel's h2 as bits (K = 4, sh_dim = 2: all 48 outputs, 36 without activation)."""
    M, K, sh_dim = 529, 4, 2
    t = dict(cc.inputs("default", M, K, sh_dim), opacity_shift=0.0, scaling_shift=0.0)
    cols = cr.columns(K, sh_dim)
    plain = torch.cat([cols[n] for n in ("sh", "scaling", "rotation", "opacity")])
    seen = torch.full((M, 80), float("nan"))
    h2 = None
    for r in range(3):
        units = torch.arange(36 * r, min(36 * r + 36, 80))
        w3 = torch.zeros(48, 80)
        w3[plain[:units.numel()], units] = 1.0
        got = run(("default", M, K, sh_dim), dict(t, w3=w3, b3=torch.zeros(48)))
        z = torch.cat([got[n] for n in ("sh", "scaling", "rotation", "opacity")], 1)       # the columns `plain`, in order
        seen[:, units] = z[:, :units.numel()]
        assert h2 is None or torch.equal(h2, got["h2"])
        h2 = got["h2"]
    same = seen == h2[:M, :80]
    print(f"forward h2 == backward h2 on {int(same.sum())} of {same.numel()} elements")
    assert bool(same.all()), f"{int((~same).sum())} hidden values differ between the two kernels"


def test_a_row_does_not_depend_on_its_position(hip_lib):
    """M = 529: the five outputs, dx and the six factor rows of a point are the same bits at row i, at row (i + 37) mod 529 of
    the rotated input, and among the first 100 rows run alone"""
    M = ORD[1]
    t = cc.inputs(*ORD)
    base = run(ORD, t)
    rolled = run(ORD, dict(t, x=t["x"].roll(37, 0), g={n: v.roll(37, 0) for n, v in t["g"].items()}))
    head = run(("default", 100) + ORD[2:], dict(t, x=t["x"][:100], g={n: v[:100] for n, v in t["g"].items()}))
    for k in cc.PER_ROW:
        assert torch.equal(rolled[k][:M].roll(-37, 0), base[k][:M]), f"{k}: a row's bits change with its position"
        assert torch.equal(head[k][:100], base[k][:100]), f"{k}: a row's bits change with M"


@pytest.mark.parametrize("absent", cr.NAMES + ("all",))
def test_absent_gradients(hip_lib, absent):
    """each of the five gradients NULL in turn (offset: `offset_out` NULL with it), and all of them: dx and dz* exactly 0"""
    t = cc.inputs(*ORD)
    t = dict(t, g={n: (None if absent in (n, "all") else v) for n, v in t["g"].items()})
    got = run(ORD, t)
    fails = _record(f"{cc.case_id(ORD)}-no-{absent}", cc.check(ORD, t, got))
    assert not fails, "; ".join(fails)
    if absent == "all":
        assert all(not bool(got[k].any()) for k in ("dx", "dz1", "dz2", "dz3", "G1", "G2", "G3"))


def test_offset_gradient_with_the_offset_output(hip_lib):
    """d_offset alone: every other gradient NULL"""
    t = cc.inputs(*ORD)
    t = dict(t, g={n: (v if n == "offset" else None) for n, v in t["g"].items()})
    fails = _record(f"{cc.case_id(ORD)}-offset-only", cc.check(ORD, t, run(ORD, t)))
    assert not fails, "; ".join(fails)


def test_two_runs_give_the_same_bits_and_a_prefilled_destination_accumulates(hip_lib):
    t = cc.inputs(*ORD)
    a = run(ORD, t)
    _same(run(ORD, t), a, "two runs differ")
    g = torch.Generator().manual_seed(5)
    prefill = {f"G{i}": torch.randn(rows, 88, generator=g) * 30 for i, rows in ((1, 80), (2, 80), (3, 48))}
    got = run(ORD, t, prefill=prefill)
    _same(got, a, "changes with the destination's content", keys=cc.PER_ROW)
    fails = _record(f"{cc.case_id(ORD)}-prefilled", cc.check(ORD, t, got, prefill=prefill))
    assert not fails, "; ".join(fails)


def _entry_args(case, t, bufs):
    _, M, K, sh_dim = case
    d = {k: t[k].to(DEV).contiguous() for k in ("x",) + W_KEYS}
    g = {n: t["g"][n].to(DEV).contiguous() for n in cr.NAMES}
    fwd = [M, K, sh_dim, d["x"]] + [d[k] for k in W_KEYS] + [float(t["opacity_shift"]), float(t["scaling_shift"])] + [bufs[n][0] for n in cr.NAMES]
    offset_out = torch.zeros(M, 3 * K, device=DEV)
    bwd = ([M, K, sh_dim, d["x"]] + [d[k] for k in W_KEYS[:5]] + [offset_out] + [g[n] for n in cr.NAMES] + [bufs["dx"][0]]
           + [bufs[n][0] for n, _ in cr.FACTORS])
    return fwd, bwd, (d, g, offset_out)


def test_no_rows(hip_lib):
    """M = 0 returns OK and writes nothing"""
    case = ("default", 16, 2, 12)
    t = cc.inputs(*case)
    bufs, _ = _buffers(16, 2, 12)
    fwd, bwd, keep = _entry_args(case, t, bufs)
    fwd[0] = bwd[0] = 0
    assert _rc("lara_coarse_decoder_forward", *fwd) == 0 and _rc("lara_coarse_decoder_backward", *bwd) == 0
    torch.cuda.synchronize()
    for k, (x, whole) in bufs.items():
        _untouched(k, x, whole)


FWD_ARG = {"M": 0, "K": 1, "sh_dim": 2, "w1": 4, "b3": 9, "sh": 13}
BWD_ARG = {"M": 0, "K": 1, "sh_dim": 2, "w1": 4, "w3": 8, "offset_out": 9}
BAD = [("K=0", {"K": 0}), ("49 outputs", {"K": 1, "sh_dim": 39}), ("M<0", {"M": -1}), ("w1=NULL", {"w1": None}), ("b3=NULL", {"b3": None}),
       ("w3=NULL", {"w3": None}), ("sh=NULL", {"sh": None}), ("d_offset without offset_out", {"offset_out": None})]


@pytest.mark.parametrize("what,change", BAD, ids=[w for w, _ in BAD])
def test_argument_errors(hip_lib, what, change):
    """each returns LARA2DGS_E_INVALID from the entry points it applies to and leaves outputs and guards untouched"""
    case = ("default", 16, 2, 12)
    t = cc.inputs(*case)
    bufs, _ = _buffers(16, 2, 12)
    fwd, bwd, keep = _entry_args(case, t, bufs)
    ran = 0
    for name, args, index in (("lara_coarse_decoder_forward", fwd, FWD_ARG), ("lara_coarse_decoder_backward", bwd, BWD_ARG)):
        if not all(k in index for k in change):
            continue
        for k, v in change.items():
            args[index[k]] = v
        assert _rc(name, *args) == E_INVALID, f"{name}: {what}"
        with pytest.raises(RuntimeError):
            call(name, DEV, *args)
        ran += 1
    assert ran
    torch.cuda.synchronize()
    for k, (x, whole) in bufs.items():
        _untouched(k, x, whole)


def test_python_entry_on_a_view_and_on_a_copy(hip_lib):
    """`coarse.forward_coarse` on a non-contiguous `feats` view and on a contiguous copy: the same bits forward and backward,
    and the bits of the C ABI (outputs, dx, and dW_l | db_l = G_l of a zero-filled destination)"""
    from lara_amd import coarse
    from lara_amd.pipeline import CoarseFineDecoder
    _, M, K, sh_dim = ORD
    t = cc.inputs(*ORD)
    abi = run(ORD, t)
    dec = CoarseFineDecoder(K=K, sh_dim=sh_dim)
    with torch.no_grad():
        for i, layer in zip((1, 2, 3), (0, 2, 4)):
            dec.mlp_coarse[layer].weight.copy_(t[f"w{i}"])
            dec.mlp_coarse[layer].bias.copy_(t[f"b{i}"])
    dec = dec.to(DEV)
    wide = torch.zeros(1, M, 96, device=DEV)
    wide[..., 7:87] = t["x"].to(DEV)

    def go(contiguous):
        dec.zero_grad(set_to_none=True)
        leaf = wide.clone().requires_grad_(True)
        feats = leaf[..., 7:87]
        assert not feats.is_contiguous()
        res = coarse.forward_coarse(dec, feats.contiguous() if contiguous else feats, t["opacity_shift"], t["scaling_shift"])
        sum((r.reshape(M, -1) * t["g"][n].to(DEV)).sum() for r, n in zip(res, cr.NAMES)).backward()
        torch.cuda.synchronize()
        out = {n: r.detach().reshape(M, -1).cpu() for r, n in zip(res, cr.NAMES)}
        out["dx"] = leaf.grad[0, :, 7:87].cpu()
        assert not bool(leaf.grad[..., :7].any()) and not bool(leaf.grad[..., 87:].any())
        for i, layer in zip((1, 2, 3), (0, 2, 4)):
            out[f"dW{i}"], out[f"db{i}"] = dec.mlp_coarse[layer].weight.grad.cpu(), dec.mlp_coarse[layer].bias.grad.cpu()
        return out
    view = go(False)
    _same(go(True), view, "changes with a contiguous copy of feats")
    n_par = K * (10 + sh_dim)
    want = {n: abi[n] for n in cr.NAMES + ("dx",)}
    for i, rows in ((1, 80), (2, 80), (3, n_par)):
        want[f"dW{i}"], want[f"db{i}"] = abi[f"G{i}"][:rows, :80], abi[f"G{i}"][:rows, 80]
    _same(want, view, "the Python entry and the C ABI differ")
