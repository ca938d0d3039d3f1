"""The image-feature volume (csrc/featvol.hip, through lara_featvol_forward / _backward / _workspace_bytes only) against the
bf16-faithful fp64 reference (oracle/featvol_bf16.py), at the cases of tests/featvol_cases.py -- each a shape at an edge the
kernels have code for: (B, V, C, E, h, w, R) =
    a (1, 1, 64, 0, 1, 1, 1)        one texel (no key bits in the placement), one point, lanes 16..63 masked, view_embed = NULL
    b (2, 3, 320, 4, 5, 7, 5)       S = 125 = 3 blocks + 29, hw = 35 (a partial scan chunk), a quarter-full channel slice, 2 scenes
    c (1, 8, 64, 32, 3, 2, 6)       8 views, 864 entries onto 6 texels: lists many 64-entry chunks long, chunks with one key
    d (1, 2, 1024, 256, 9, 15, 4)   the largest C and E, hw = 135 (two scan chunks + 7), S = 64 = exactly two blocks
    e (1, 4, 128, 32, 64, 128, 3)   hw = 8192 = LARA_FEATVOL_MAX_HW, 99 % of the texel lists empty
tests/test_featvol_faithful.py shows (without a GPU) that every case has points inside, across each border and outside, a view
that sees nothing, and no point whose position rounding could go the other way on the device.

Two regimes.  A: mlp_w = 0, so [shift | scale] = bf16(bias) exactly and everything behind it is plain fp32.  B: mlp_w random.

Element by element, nothing exempted (regime A: out, dx, d_ln_w, d_ln_b; both regimes: d_view_embed):
        |got - ref| <= 4 A + 2^-23 |ref|            TOKENS layout:  |got - ref| <= ulp_bf16(ref) + A
with ref the fp64 value and A the fp32 error bound of THAT element from the reference's own operands: K 2^-24 sum|terms| with K
the number of terms (C for each LayerNorm moment, 4 taps, the texel's list length for dY, the token count for d_ln_w / d_ln_b,
B S for d_view_embed), propagated through the formulas (`_bounds`), plus the fp32 error of the bilinear weights
(2 * 2^-24 (|position| + 1) per coordinate).  A texel with an empty list has A = 0 and ref = 0: its dx must be exactly zero, as
every dx of the view that sees nothing.  The embedding columns of out are exact in both layouts.

By the noise yardstick (regime B: every tensor; both regimes: d_mlp_w, d_mlp_b, which sum the bf16 rows d[shift | scale]):
per tensor, N = ||faithful - unrounded||_2 / ||unrounded||_2 (from the reference alone; `unrounded` keeps the position
roundings, which are no noise: the device's positions are the reference's) and E = ||device - faithful||_2 / ||unrounded||_2;
the test asserts E <= BAR * N with one BAR for all tensors and cases, and the same ratio in the max-norm <= 1.0.  Every E, N,
ratio and worst |diff| / limit goes to featvol_faithful_errors.json in the directory LARA2DGS_TEST_OUT names (default: test_out/
in the repository root, kept out of git).

Measured on an MI355X (first clean run, all five cases, both regimes).  The largest E / N is 0.0122 (tokens at (d), regime B;
d_mlp_b 0.0065 - 0.0099 at (b), (c), (d) in either regime; out 0.0053 and tokens 0.0073 at (b); d_mlp_w <= 0.0034; dx, d_ln_w,
d_ln_b <= 0.0001): BAR = 2 x 0.0122 = 0.0245.  In the max-norm the largest ratio is 0.134 (out at (b), regime B; tokens 0.107 at (b),
0.097 at (d); d_mlp_b <= 0.059), against its bar of 1.0.  The worst |diff| / limit of the fp32 parts: out 0.009, dx 0.004,
d_ln_w 0.005, d_ln_b 0.037 (case (a): one token, one term), d_view_embed 0.010, and 0.499 for the TOKENS layout (half a bf16 ulp:
the correctly rounded value).  These cases found no defect in csrc/featvol.hip: every test passed on the kernels as they were.

The interface branches run on (b) and (c): every output inside a NaN-filled buffer (all written, no guard touched: "writes,
does not accumulate", the tokens with empty lists included); a 0xFF-filled workspace gives the bits of a zero-filled one; the
gradient through either grad_layout, and out and every gradient from the three layouts of x (contiguous, channels-last,
channels-last one element into its buffer: the scalar path), are bitwise equal, dx at x's strides; d_view_embed = NULL changes
no other gradient; two runs give the same bits.
"""
import json
import os

import pytest
import torch

from lara_amd._native import FeatvolDims, call, query
from oracle import featvol_bf16 as fb
from tests import featvol_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
VOLUME, TOKENS = 0, 1
GUARD = 64            # guard elements on either side of every output (keeps the 16-byte alignment of the vector path)
# One bar for all tensors and cases: twice the largest E / N of the first clean run on an MI355X (2 x 0.0122), at most 0.5.
BAR = 0.0245
BAR_MAX = 1.0
_LOG = {"fp32": {}, "noise": {}}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    if not (_LOG["fp32"] or _LOG["noise"]):
        return
    out = os.environ.get("LARA2DGS_TEST_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_out")
    os.makedirs(out, exist_ok=True)
    noise = _LOG["noise"].values()
    with open(os.path.join(out, "featvol_faithful_errors.json"), "w") as f:
        json.dump({"bar": BAR, "max_ratio_l2": max((v["ratio_l2"] for v in noise), default=None),
                   "max_ratio_max": max((v["ratio_max"] for v in noise), default=None),
                   "max_fp32_diff_over_limit": max(_LOG["fp32"].values(), default=None),
                   "fp32_worst_diff_over_limit": _LOG["fp32"], "noise": _LOG["noise"]}, f, indent=1)


# ---------------------------------------------------------------------------------------------- device plumbing

def _guarded(shape, dtype, stride=None, offset=0):
    """a tensor of `shape` (contiguous, or at `stride`) inside a NaN-filled buffer, `offset` elements past the front guard
    -> (tensor, whole buffer, [first, last) of the tensor's storage span in it)"""
    t0 = torch.empty(shape, device="meta").contiguous() if stride is None else torch.empty_strided(shape, stride, device="meta")
    span = 1 + sum((n - 1) * s for n, s in zip(t0.shape, t0.stride()))
    whole = torch.full((GUARD + offset + span + GUARD,), float("nan"), dtype=dtype, device=DEV)
    return whole.as_strided(tuple(shape), t0.stride(), GUARD + offset), whole, (GUARD + offset, GUARD + offset + span)


def _written_inside(name, tensor, whole, span):
    assert bool(torch.isfinite(tensor).all()), f"{name}: elements left unwritten"
    mask = torch.ones(whole.numel(), dtype=torch.bool, device=DEV)
    mask[span[0]:span[1]] = False
    assert bool(torch.isnan(whole[mask]).all()), f"{name}: written outside the tensor"


def _x_layout(rows, shape, kind):
    """rows [B V, h w, C] -> x [B V, C, h, w]: 'nchw' contiguous, 'cl' the channels-last view, 'cl1' a channels-last view whose
    storage starts one element into its buffer (unit channel stride, not 16-byte aligned: the scalar path); and dx's (stride, offset)"""
    BV, C, h, w = shape
    x = rows.view(BV, h, w, C).permute(0, 3, 1, 2)
    if kind == "nchw":
        return x.contiguous(), None, 0
    if kind == "cl":
        return x, x.stride(), 0
    buf = torch.zeros(rows.numel() + 1, dtype=rows.dtype, device=rows.device)
    buf[1:] = rows.reshape(-1)
    return buf.as_strided((BV, C, h, w), x.stride(), 1), x.stride(), 1


class Device:
    """one case and regime on the device; every call through the public C ABI"""

    def __init__(self, case, regime, x_layout="cl"):
        (B, V, C, E, h, w, R), (img_w, img_h), _ = fc.CASES[case]
        t, _ = fc.inputs(case, regime)
        self.shape, self.S, self.CE = (B, V, C, E, h, w, R), R ** 3, C + E
        dev = lambda k: None if t[k] is None else t[k].to(DEV).contiguous()
        self.x, self.dx_stride, self.dx_offset = _x_layout(t["rows"].to(DEV), (B * V, C, h, w), x_layout)
        assert x_layout == "nchw" or (self.x.stride(1) == 1 and (self.x.data_ptr() % 16 == 0) == (x_layout == "cl"))
        self.args = [self.x, dev("rays"), dev("w2c"), dev("ixt"), fb.dense_grid(R).to(DEV), dev("ln_w"), dev("ln_b"), dev("mlp_w"),
                     dev("mlp_b")]
        self.embed = dev("embed")
        self.grad = t["grad"].to(DEV)                                                   # VOLUME layout [B, V, C + E, S]
        d = FeatvolDims()
        d.B, d.V, d.C, d.E, d.h, d.w, d.R, d.img_w, d.img_h, d.eps = B, V, C, E, h, w, R, img_w, img_h, fc.EPS
        for i, s in enumerate(self.x.stride()):
            d.x_stride[i] = s
        self.d = d

    def workspace(self, fill):
        return torch.full((query("lara_featvol_workspace_bytes", self.d),), fill, dtype=torch.uint8, device=DEV)

    def forward(self, layout, fill=0xFF):
        B, V, C, E, h, w, R = self.shape
        shape, dtype = ((B, V, self.CE, self.S), torch.float32) if layout == VOLUME else ((B * self.S, V, self.CE), torch.bfloat16)
        out, whole, span = _guarded(shape, dtype)
        call("lara_featvol_forward", DEV, self.d, *self.args, self.embed, layout, out, self.workspace(fill))
        torch.cuda.synchronize()
        _written_inside(f"out[{layout}]", out, whole, span)
        return out

    def backward(self, grad_layout=VOLUME, fill=0xFF, want_embed=True):
        """-> dict of the six gradients (d_view_embed None when E = 0 or not wanted), each checked against its guards"""
        B, V, C, E, h, w, R = self.shape
        grad = self.grad if grad_layout == VOLUME else self.grad.permute(0, 3, 1, 2).reshape(B * self.S, V, self.CE).contiguous()
        bufs = {"dx": _guarded(self.x.shape, torch.float32, self.dx_stride, self.dx_offset), "d_ln_w": _guarded((C,), torch.float32),
                "d_ln_b": _guarded((C,), torch.float32), "d_mlp_w": _guarded((2 * C, 32), torch.float32),
                "d_mlp_b": _guarded((2 * C,), torch.float32),
                "d_view_embed": _guarded((V, E), torch.float32) if (E and want_embed) else (None, None, None)}
        call("lara_featvol_backward", DEV, self.d, *self.args, grad, grad_layout, *(bufs[k][0] for k in fb.GRADS), self.workspace(fill))
        torch.cuda.synchronize()
        for k, (t, whole, span) in bufs.items():
            if t is not None:
                _written_inside(k, t, whole, span)
        assert bufs["dx"][0].stride() == self.x.stride()
        return {k: v[0] for k, v in bufs.items()}


# ---------------------------------------------------------------------------------------------- bounds (regime A)

def ulp_bf16(ref):
    _, e = torch.frexp(ref.abs().double())
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), e.clamp(min=-125) - 8)


def _gather(rows, idx, hw):
    """rows [BV, hw, C] at the taps idx [BV, S, 4] (-1: the zero padding) -> [BV, S, 4, C]"""
    BV, _, C = rows.shape
    pad = torch.cat([rows, rows.new_zeros(BV, 1, C)], 1).reshape(-1, C)
    return pad[torch.where(idx < 0, torch.full_like(idx, hw), idx) + (torch.arange(BV) * (hw + 1))[:, None, None]]


def _scatter(vals, idx, hw):
    """the transpose of _gather: vals [BV, S, 4, C] summed per texel -> [BV hw, C]"""
    BV, _, _, C = vals.shape
    rows = torch.where(idx < 0, torch.full_like(idx, hw), idx) + (torch.arange(BV) * (hw + 1))[:, None, None]
    out = vals.new_zeros(BV * (hw + 1), C).index_add_(0, rows.reshape(-1), vals.reshape(-1, C))
    return out.view(BV, hw + 1, C)[:, :hw].reshape(BV * hw, C)


def _bounds(case):
    """the reference's regime-A values and the fp32 error bound A of every element of out, dx, d_ln_w, d_ln_b"""
    (B, V, C, E, h, w, R), _, _ = fc.CASES[case]
    t, ref = fc.inputs(case, "A")
    fa, _ = fc.reference(case, "A")
    f = fa["fwd"]
    BV, hw, S, T = B * V, h * w, R ** 3, B * V * h * w
    g_w, eps = ref["ln_w"], ref["eps"]
    # LayerNorm, two-pass moments of C terms each
    xr = ref["x"].permute(0, 2, 3, 1).reshape(T, C)
    mean = xr.mean(-1, keepdim=True)
    c = xr - mean
    e_c = C * U * xr.abs().mean(-1, keepdim=True) + U * c.abs()
    var = (c * c).mean(-1, keepdim=True)
    d_var = (2 * c.abs() * e_c).mean(-1, keepdim=True) + (C + 2) * U * var
    rstd = f["rstd"]
    rel = d_var / (2 * (var + eps)) + 3 * U                              # relative error of rstd
    xh, n, opm, y = f["xh"], f["n"], f["opm"], f["y"]
    A_xh = rstd * e_c + xh.abs() * (rel + U)
    A_n = g_w.abs() * A_xh + U * (xh * g_w).abs() + U * n.abs()
    A_y = opm.abs() * A_n + U * (n * opm).abs() + U * y.abs()
    # bilinear weights: the fp32 position is within 2 * 2^-24 (|i| + 1) of the reference's; the weights' factors are exact
    ix, iy, idx, wgt = f["ix"], f["iy"], f["idx"], f["wgt"]
    e_x, e_y = 2 * U * (ix.abs() + 1), 2 * U * (iy.abs() + 1)
    fx, fy = torch.floor(ix), torch.floor(iy)
    A_w = torch.stack([e_x * (iy - fy if k >> 1 else fy + 1 - iy).abs() + e_y * (ix - fx if k & 1 else fx + 1 - ix).abs()
                       for k in range(4)], -1) + U * wgt.abs()
    inside = (idx >= 0)[..., None]
    # out = sum of 4 taps
    y_t, Ay_t = _gather(y.view(BV, hw, C), idx, hw), _gather(A_y.view(BV, hw, C), idx, hw)
    A_out = (inside * (wgt.abs()[..., None] * Ay_t + A_w[..., None] * y_t.abs() + 4 * U * (wgt[..., None] * y_t).abs())).sum(2)
    A_out = A_out.view(B, V, S, C).transpose(2, 3)
    # dY = sum over the texel's list
    g = t["grad"].double()[:, :, :C].permute(0, 1, 3, 2).reshape(BV, S, 1, C)
    L = _scatter(inside.double().expand(-1, -1, -1, 1), idx, hw)
    A_dy = _scatter(inside * A_w[..., None] * g.abs(), idx, hw) + L * U * _scatter(inside * (wgt[..., None] * g).abs(), idx, hw)
    dy = fa["dy"]
    dn = dy * opm
    A_dn = opm.abs() * A_dy + U * dn.abs()
    # gamma / beta: sums over the T token rows
    A_lnb = A_dn.sum(0) + T * U * dn.abs().sum(0)
    A_lnw = (A_dn * xh.abs() + dn.abs() * A_xh + U * (dn * xh).abs()).sum(0) + T * U * (dn * xh).abs().sum(0)
    # LayerNorm's backward: dx = rstd (dxh - mean(dxh) - xh mean(dxh xh))
    dxh = dn * g_w
    A_dxh = g_w.abs() * A_dn + U * dxh.abs()
    s1, s2 = dxh.mean(-1, keepdim=True), (dxh * xh).mean(-1, keepdim=True)
    A_s1 = A_dxh.mean(-1, keepdim=True) + (C + 1) * U * dxh.abs().mean(-1, keepdim=True)
    A_s2 = (A_dxh * xh.abs() + dxh.abs() * A_xh).mean(-1, keepdim=True) + (C + 2) * U * (dxh * xh).abs().mean(-1, keepdim=True)
    inner = dxh - s1 - xh * s2
    A_in = A_dxh + A_s1 + A_xh * s2.abs() + xh.abs() * A_s2 + 3 * U * (dxh.abs() + s1.abs() + (xh * s2).abs())
    A_dx = rstd * A_in + inner.abs() * rstd * rel + U * (rstd * inner).abs()
    A_dx = A_dx.view(BV, h, w, C).permute(0, 3, 1, 2)
    return {"out": (f["out"][:, :, :C], A_out), "tokens_pre": (f["tokens_pre"][:, :, :C], A_out.permute(0, 3, 1, 2).reshape(B * S, V, C)),
            "dx": (fa["dx"], A_dx), "d_ln_w": (fa["d_ln_w"], A_lnw), "d_ln_b": (fa["d_ln_b"], A_lnb), "empty": (L == 0).view(BV, h, w)}


def _embed_bound(case):
    (B, V, C, E, h, w, R), _, _ = fc.CASES[case]
    g = fc.inputs(case, "A")[0]["grad"].double()[:, :, C:]                  # [B, V, E, S]; the same in both regimes
    return g.sum((0, 3)), B * R ** 3 * U * g.abs().sum((0, 3))


def _check(fails, key, got, ref, A, bf16=False):
    d = (got.double().cpu() - ref).abs()
    lim = ulp_bf16(ref) + A if bf16 else 4 * A + 2.0 ** -23 * ref.abs()
    bad = d > lim
    worst = float(torch.where(lim > 0, d / lim, torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d))).max())
    _LOG["fp32"][key] = worst
    print(f"{key:24s} worst |diff| / limit = {worst:.3f}")
    if bad.any():
        fails.append(f"{key}: {int(bad.sum())} of {bad.numel()} elements beyond the limit; worst |diff| / limit = {worst:.3f}")


def _measure(fails, key, got, fa, un):
    e2, emax = fc.rel(got.cpu(), fa, un)
    n2, nmax = fc.rel(fa, un, un)
    _LOG["noise"][key] = {"E_l2": e2, "N_l2": n2, "ratio_l2": e2 / n2, "E_max": emax, "N_max": nmax, "ratio_max": emax / nmax}
    print(f"{key:24s} E {e2:.3e}  N {n2:.3e}  E/N {e2 / n2:.4f}   max-norm: E {emax:.3e}  N {nmax:.3e}  E/N {emax / nmax:.4f}")
    if not e2 <= BAR * n2:
        fails.append(f"{key}: E = {e2:.3e} > {BAR} * N = {BAR * n2:.3e}")
    if not emax <= BAR_MAX * nmax:
        fails.append(f"{key}: max-norm E = {emax:.3e} > {BAR_MAX} * N = {BAR_MAX * nmax:.3e}")


def _embedding_columns_exact(dv, vol, tok):
    B, V, C, E, h, w, R = dv.shape
    if not E:
        return
    assert torch.equal(vol[:, :, C:], dv.embed[None, :, :, None].expand(B, V, E, dv.S)), "embedding columns, VOLUME"
    assert torch.equal(tok[:, :, C:], dv.embed.to(torch.bfloat16)[None].expand(B * dv.S, V, E)), "embedding columns, TOKENS"


def _blind_views(case):
    kinds = fc.CASES[case][2]
    return [b * len(row) + v for b, row in enumerate(kinds) for v, kind in enumerate(row) if kind == "blind"]


# ---------------------------------------------------------------------------------------------- the tests

@pytest.mark.parametrize("case", list(fc.CASES))
def test_fp32_parts_element_by_element(hip_lib, case):
    """regime A: out (both layouts), dx, d_ln_w, d_ln_b, d_view_embed within the fp32 bound of each element; the Linear's
    gradients by the yardstick"""
    dv = Device(case, "A")
    B, V, C, E, h, w, R = dv.shape
    vol, tok, gr = dv.forward(VOLUME), dv.forward(TOKENS), dv.backward()
    bd, fails = _bounds(case), []
    _check(fails, f"{case}/A/out", vol[:, :, :C], *bd["out"])
    _check(fails, f"{case}/A/tokens", tok[:, :, :C].float(), *bd["tokens_pre"], bf16=True)
    for k in ("dx", "d_ln_w", "d_ln_b"):
        _check(fails, f"{case}/A/{k}", gr[k], *bd[k])
    if E:
        _check(fails, f"{case}/A/d_view_embed", gr["d_view_embed"], *_embed_bound(case))
    _embedding_columns_exact(dv, vol, tok)
    dx = gr["dx"].permute(0, 2, 3, 1).cpu()                                      # [B V, h, w, C]
    assert bool((dx[bd["empty"]] == 0).all()), "dx of a token with an empty list"
    for bv in _blind_views(case):
        assert bool((gr["dx"][bv] == 0).all()), f"dx of view {bv}, which sees nothing"
    for k, (fa, un) in fc.yardstick_tensors(case, "A").items():
        _measure(fails, f"{case}/A/{k}", gr[k], fa, un)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("case", list(fc.CASES))
def test_noise_bar(hip_lib, case):
    """regime B: every tensor within BAR x the bf16 noise of the reference; d_view_embed and the embedding columns as in A"""
    dv = Device(case, "B")
    B, V, C, E, h, w, R = dv.shape
    vol, tok, gr = dv.forward(VOLUME), dv.forward(TOKENS), dv.backward()
    got = dict(gr, out=vol, tokens=tok.float())
    fails = []
    for k, (fa, un) in fc.yardstick_tensors(case, "B").items():
        _measure(fails, f"{case}/B/{k}", got[k], fa, un)
    if E:
        _check(fails, f"{case}/B/d_view_embed", gr["d_view_embed"], *_embed_bound(case))
    _embedding_columns_exact(dv, vol, tok)
    for bv in _blind_views(case):
        assert bool((gr["dx"][bv] == 0).all()), f"dx of view {bv}, which sees nothing"
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("case", ["b", "c"])
def test_interface_branches_are_bitwise(hip_lib, case):
    """(the NaN sentinels around every output are checked inside Device.forward / .backward, in every test of this file)"""
    dv = Device(case, "B")
    vol, tok, gr = dv.forward(VOLUME), dv.forward(TOKENS), dv.backward(VOLUME)

    def same(a, b, what):
        for k in a:
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), f"{k}: {what}"
    # workspace content: 0xFF-filled (above) against zero-filled
    assert torch.equal(dv.forward(VOLUME, fill=0), vol) and torch.equal(dv.forward(TOKENS, fill=0), tok)
    same(dv.backward(VOLUME, fill=0), gr, "depends on the workspace's content")
    # the gradient through either layout; two runs
    same(dv.backward(TOKENS), gr, "grad_layout TOKENS differs from VOLUME")
    same(dv.backward(VOLUME), gr, "two runs differ")
    assert torch.equal(dv.forward(VOLUME), vol) and torch.equal(dv.forward(TOKENS), tok)
    # d_view_embed = NULL
    g0 = dv.backward(VOLUME, want_embed=False)
    assert g0.pop("d_view_embed") is None
    same(g0, {k: v for k, v in gr.items() if k != "d_view_embed"}, "changes when d_view_embed = NULL")
    # the three layouts of x; dx at x's strides
    for kind in ("nchw", "cl1"):
        other = Device(case, "B", kind)
        assert torch.equal(other.forward(VOLUME), vol) and torch.equal(other.forward(TOKENS), tok), f"out, x layout {kind}"
        go = other.backward(VOLUME)
        assert go["dx"].stride() == other.x.stride() and go["dx"].is_contiguous() == (kind == "nchw")
        same(go, gr, f"x layout {kind} differs from channels-last")
