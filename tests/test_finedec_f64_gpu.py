"""The six kernels of csrc/finedec.hip, through the entry points of include/lara_finedec.h only (`lara_amd._native.call` and
`query`), against the fp64 reference (oracle/finedec_f64.py) at the cases of tests/finedec_cases.py.
tests/test_finedec_f64.py shows (without a GPU) that every case meets the kink condition and contains what it claims, that a
correct fp32 evaluation passes every check below, and that three wrong ones do not.

Element by element, nothing exempted:
        |got - ref| <= 4 A + 2^-23 |ref|
with ref the fp64 value and A the fp32 error bound of THAT element from the reference's own operands (K 2^-24 sum|terms| for a
sum or product of K terms; the softmax's relative 4 A_s + 2^-23 |s - max| + 16 * 2^-24 plus 2^-126; K = 512 + slabs for a weight
gradient; K = 256 for a `partials` entry), propagated through the formulas where the interface hands nothing out (scores -> P ->
U; hid -> sh in the forward kernel; du -> DT, d_pf) and restarted from the device's own arrays where it does (HID from U, DH
under the mask HID > 0, d_xn from DT, the five weight gradients from U, HID, DH, DT, the LayerNorm's backward from `stats`, and
xn once more from `stats`).  An element with A = 0 and ref = 0 must be exactly 0: sh = b2 and zero DH, DT, d_xn, d_pf of a point
whose units are all dead, every gradient for d_sh = 0; xn = beta exactly for a constant row and a column with gamma = 0.

Position independence (n = 529): sh, d_xn, d_pf, U, HID, DH, DT of a point are the same bits at row i, at row (i + 37) mod 529 of
the rotated input, and among the first 100 rows run alone -- a point is one MFMA column and never mixes with its neighbours.

Interface branches (n = 129 and 529): every output sits NaN-filled between two 64-element NaN guards, in every test of this
file -- all of it written (sh[8..11], d_xn[72..79], the four factor arrays, `out` of the weight gradients, `partials` for
lara_fine_ln_blocks(n) blocks), no guard touched; a 0xFF-filled workspace gives the bits of a zero-filled one; n = 0 writes
nothing (the weight gradients: zero-fill `out`); two runs give the same bits.  Through Python (n = 257): `forward_fine` with
`folded=` and with point_feats as the einsum view or a contiguous copy gives the same bits.

Every worst |diff| / limit, per tensor and case, goes to finedec_f64_errors.json in the directory LARA2DGS_TEST_OUT names
(default: test_out/ in the repository root, kept out of git).

Measured on an MI355X (first clean run, all 34 decoder and 22 LayerNorm cases).  The largest |diff| / limit is 0.166 (xn
recomputed from the device's own stats, LayerNorm, ordinary rows, n = 131205: three operations per element, the tightest bound
here; 0.150 - 0.166 at every size).  Per tensor: DH 0.088, d_xn 0.029, HID 0.022 (the teacher-forced stages, K = 12 - 65);
wgrad 0.0042 (dWqk, saturated, n = 529; dW1ov 0.0019, dW2 0.0016, db1 0.0007, db2 0.0004: K = 512 + slabs against sums that
round like random walks); sh 0.0024, U 0.0010, DT 0.0011, d_pf 0.0006 (the propagated stages: the prescribed 4 A_s inside P's
bound is a worst case over 80-term and 8-term sums, a few hundred times what the kernel's error is, so these four would notice
a wrong term or operand -- the mutation checks of tests/test_finedec_f64.py show it -- but not a lost digit; their sharp
checks are the forced stages behind them); LayerNorm: xn 0.079 (one outlier of 1e4, n = 255), stats 0.035, d_x 0.030,
partials = d_gamma 0.0019, d_beta 0.0003.  The fp32 CPU stand-in of tests/test_finedec_f64.py lands within a factor of 1.3
of each decoder figure; its LayerNorm sums (numpy's pairwise sums) come to 0.007 / 0.002 and its xn from stats to 0.218.  These cases found no defect in csrc/finedec.hip: every test passed on the kernels as they were.
"""
import json
import os

import pytest
import torch

from lara_amd._native import call, query
from oracle import finedec_f64 as fr
from tests import finedec_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
W_KEYS = ("Wqk", "W1ov", "b1", "W2", "b2")
BWD_OUT = {"d_xn": lambda n: (n, 80), "d_pf": lambda n: (4, 8, n), "U": lambda n: (n, 64), "HID": lambda n: (n, 64),
           "DH": lambda n: (n, 64), "DT": lambda n: (n, 64)}
_LOG = {}


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
    with open(os.path.join(out, "finedec_f64_errors.json"), "w") as f:
        json.dump({"max_diff_over_limit": max(_LOG.values()), "per_tensor": {k: {"worst": v, "at": at} for k, (v, at) in per_tensor.items()},
                   "worst_diff_over_limit": _LOG}, f, indent=1)


# ---------------------------------------------------------------------------------------------- device plumbing

def _guarded(shape):
    """a contiguous fp32 tensor of `shape` inside a NaN-filled buffer -> (tensor, whole buffer)"""
    k = torch.Size(shape).numel()
    whole = torch.full((GUARD + k + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return whole[GUARD:GUARD + k].view(shape), whole


def _written_inside(name, tensor, whole):
    assert bool(torch.isfinite(tensor).all()), f"{name}: elements left unwritten"
    assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + tensor.numel():]).all()), f"{name}: written outside the tensor"


def run_decoder(t, ws_fill=0xFF):
    """forward, backward and the weight gradients of one case, every output guarded -> {name: CPU tensor}"""
    n = t["xn"].shape[0]
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    w = [d[k] for k in ("xn", "pf") + W_KEYS]
    bufs = {"sh": _guarded((n, 12)), "wgrad": _guarded((query("lara_fine_wgrad_floats"),))}
    bufs.update({k: _guarded(shape(n)) for k, shape in BWD_OUT.items()})
    call("lara_fine_decoder_forward", DEV, n, *w, bufs["sh"][0])
    call("lara_fine_decoder_backward", DEV, n, *w, d["d_sh"], *(bufs[k][0] for k in BWD_OUT))
    ws = torch.full((max(query("lara_fine_wgrad_workspace_bytes", n), 16),), ws_fill, dtype=torch.uint8, device=DEV)
    call("lara_fine_decoder_wgrad", DEV, n, d["xn"], *(bufs[k][0] for k in ("U", "HID", "DH", "DT")), d["d_sh"], bufs["wgrad"][0], ws)
    torch.cuda.synchronize()
    for k, (x, whole) in bufs.items():
        _written_inside(k, x, whole)
    return {k: x.cpu() for k, (x, _) in bufs.items()}


def run_ln(t):
    n = t["x"].shape[0]
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    blocks = query("lara_fine_ln_blocks", n)
    assert blocks == fr.fine_ln_blocks(n)
    bufs = {"xn": _guarded((n, 80)), "stats": _guarded((n, 2)), "d_x": _guarded((n, 80)), "partials": _guarded((blocks, 160))}
    call("lara_fine_ln_forward", DEV, n, d["x"], d["gamma"], d["beta"], fc.LN_EPS, bufs["xn"][0], bufs["stats"][0])
    call("lara_fine_ln_backward", DEV, n, d["x"], d["gamma"], bufs["stats"][0], d["d_xn"], bufs["d_x"][0], bufs["partials"][0])
    torch.cuda.synchronize()
    for k, (x, whole) in bufs.items():
        _written_inside(k, x, whole)
    return {k: x.cpu() for k, (x, _) in bufs.items()}


def _record(prefix, res):
    for k, v in res.items():
        _LOG[f"{prefix}/{k}"] = v
        print(f"{prefix + '/' + k:40s} worst |diff| / limit = {v:.4f}")
    return [f"{k}: worst |diff| / limit = {v:.3f}" for k, v in res.items() if not v <= 1.0]


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: {what}"


# ---------------------------------------------------------------------------------------------- the tests

@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_decoder_element_by_element(hip_lib, case):
    """lara_fine_decoder_forward, _backward and _wgrad: every element of sh, U, HID, DH, DT, d_xn, d_pf and the five weight
    gradients within the fp32 bound of that element"""
    t = fc.inputs(*case)
    assert query("lara_fine_wgrad_floats") == fr.fine_wgrad_floats()
    assert query("lara_fine_wgrad_workspace_bytes", case[1]) == fr.fine_wgrad_slabs(case[1]) * fr.fine_wgrad_floats() * 4
    got = run_decoder(t)
    fails = _record(fc.case_id(case), fc.check_decoder(t, got)) + fc.exact_claims(case[0], t, got)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("case", fc.LN_CASES, ids=fc.case_id)
def test_layernorm_element_by_element(hip_lib, case):
    """lara_fine_ln_forward and _backward: xn, stats, d_x, every `partials` entry, and their column sums as d_gamma / d_beta"""
    t = fc.ln_inputs(*case)
    got = run_ln(t)
    fails = _record("ln-" + fc.case_id(case), fc.check_ln(t, got)) + fc.ln_exact_claims(case[0], t, got)
    assert not fails, "; ".join(fails)


def test_a_point_does_not_depend_on_its_position(hip_lib):
    t = fc.inputs("ordinary", 529)
    rows = ("xn", "d_sh")
    base = run_decoder(t)
    rolled = run_decoder({k: (v.roll(37, 0) if k in rows else v.roll(37, 2) if k == "pf" else v) for k, v in t.items()})
    head = run_decoder({k: (v[:100] if k in rows else v[:, :, :100] if k == "pf" else v) for k, v in t.items()})
    for k in ("sh",) + tuple(BWD_OUT):
        axis = 2 if k == "d_pf" else 0
        assert torch.equal(rolled[k].roll(-37, axis), base[k]), f"{k}: a point's bits change with its row"
        assert torch.equal(head[k], base[k].narrow(axis, 0, 100)), f"{k}: a point's bits change with n"


@pytest.mark.parametrize("n", [129, 529])
def test_interface_branches_are_bitwise(hip_lib, n):
    """(the NaN fill and the guards around every output are checked inside run_decoder / run_ln)"""
    t = fc.inputs("ordinary", n)
    a = run_decoder(t)
    _same(run_decoder(t, ws_fill=0), a, "depends on the workspace's content")
    _same(run_decoder(t), a, "two runs differ")
    ln = fc.ln_inputs("ordinary", 529 if n == 529 else 257)
    _same(run_ln(ln), run_ln(ln), "two runs differ")


def test_no_points(hip_lib):
    """n = 0: forward and backward return OK and write nothing; the weight gradients zero-fill `out`"""
    t = {k: v.to(DEV) for k, v in fc.inputs("ordinary", 1).items()}
    w = [t[k] for k in ("xn", "pf") + W_KEYS]
    bufs = [_guarded((16,))[1] for _ in range(7)]
    call("lara_fine_decoder_forward", DEV, 0, *w, bufs[0])
    call("lara_fine_decoder_backward", DEV, 0, *w, t["d_sh"], *bufs[1:7])
    ln = [_guarded((16,))[1] for _ in range(4)]
    call("lara_fine_ln_forward", DEV, 0, t["xn"], t["b1"], t["b1"], fc.LN_EPS, ln[0], ln[1])
    call("lara_fine_ln_backward", DEV, 0, t["xn"], t["b1"], ln[1], t["xn"], ln[2], ln[3])
    out, whole = _guarded((query("lara_fine_wgrad_floats"),))
    assert query("lara_fine_wgrad_workspace_bytes", 0) == 0 and query("lara_fine_ln_blocks", 0) == 0
    call("lara_fine_decoder_wgrad", DEV, 0, None, None, None, None, None, None, out, None)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b).all()) for b in bufs + ln), "n = 0 wrote something"
    assert not bool(out.any())
    _written_inside("wgrad", out, whole)


def test_forward_fine_folded_argument_and_point_feats_layout(hip_lib):
    """n = 257 through lara_amd.fine.forward_fine: `folded=` and a contiguous copy of the einsum view change no bit"""
    from lara_amd.fine import fold_fine_weights, forward_fine
    from oracle.finedec_ref import FineDecoderRef
    n = 257
    g = torch.Generator().manual_seed(257)
    torch.manual_seed(257)
    dec = FineDecoderRef().to(DEV)
    vol0, pfp0, gout = torch.randn(n, 80, generator=g).to(DEV), torch.randn(4, 8, n, generator=g).to(DEV), torch.randn(n, 1, 12, generator=g).to(DEV)

    def run(folded, contiguous):
        dec.zero_grad(set_to_none=True)
        vol, pfp = vol0.clone().requires_grad_(True), pfp0.clone().requires_grad_(True)
        pf = torch.einsum('lcb->blc', pfp)
        assert not pf.is_contiguous()
        sh = forward_fine(dec, vol, pf.contiguous() if contiguous else pf, folded=fold_fine_weights(dec) if folded else None)
        (sh * gout).sum().backward()
        torch.cuda.synchronize()
        return {"sh": sh.detach(), "d_vol": vol.grad, "d_pf": pfp.grad, **{k: p.grad.clone() for k, p in dec.named_parameters()}}
    base = run(False, False)
    assert base["sh"].shape == (n, 1, 12)
    _same(run(True, False), base, "changes with folded=")
    _same(run(False, True), base, "changes with a contiguous copy of point_feats")
