"""The DINO ViT encoder (lara_amd/csrc/vit.hip, include/lara_vit.h) on the MI355X, stage by stage, against the bf16-faithful fp64
reference (oracle/vit_bf16.py: fp64 arithmetic, rounded to bf16 exactly where the kernels round; tests/test_vit_bf16.py holds that
reference to the restatement, to torch's bf16 cast and to a list of built-in defects, on the CPU).

The C ABI is driven directly (lara_amd._native) with buffers the test owns; the stages are read out of `save` through
lara_vit_save_offsets.  Cases (N, views, H, W, C, F, depth) -- tests/vit_cases.py -- reach what the ViT-B / ViT-S shapes of
test_dino_gpu.py never do:
    (1, 1,  16,  16,   64,   64, 1)   T = 2,   M = 2     one patch, one head, 126 padded rows
    (3, 1,  64, 128,  128,  192, 1)   T = 33,  M = 99    one live key in the last 32-key block, F != 4 C
    (2, 2, 112, 144,  320, 1280, 2)   T = 64 = Tp, M = 128 = Mp   no padding anywhere (every `if (Mp > M)` memset skipped), the strided
                                                         [B, V, H, W, 3] slice, two blocks, C = 320 (quad 1 of the LayerNorm lanes: 16 lanes)
    (3, 1, 128, 128, 1024,  256, 1)   T = 65,  M = 195   a lone query in the second 64-query block, the width limit, F < C
    (5, 1, 240, 240,   64,  128, 1)   T = 226, M = 1130  the second trip of ln_bwd_kernel's row loop, 8 key blocks

(a) forward, teacher-forced (tests/vit_cases.check_forward has the limits and their named terms): patches bitwise; every saved
    stage of every block, xfin, stf and out recomputed in fp64 from the DEVICE's saved inputs of that stage, every element within
    ulp_bf16 + A (bf16 stages) or 4 A + 2^-23 |ref| (fp32 stages); g = gelu(h), not saved, through xout; padded rows and padded
    tokens exactly zero.
(b) backward: all 6 + 12 depth gradients against the reference's autograd evaluated on the device's saved forward,
    E = ||device - faithful||_2 / ||unrounded||_2 <= BAR * N with N = ||faithful - unrounded||_2 / ||unrounded||_2 from the reference
    alone; the max-norm to a separate bar of 1.0.  norm.bias (the column sums of the fp32 output gradient, N = 0: no rounding lies in
    front of it) is held to the fp32 bound of such a sum instead.  Every E, N and ratio goes to vit_stage_errors.json in the
    directory LARA2DGS_TEST_OUT names (default: test_out/ in the repository root, kept out of git).
(c) memory discipline, forward and backward: save, workspace, out and every gradient buffer sit between guard zones that are intact
    afterwards; a run with save, workspace, out and the gradients prefilled with 0xFF bytes (bf16 and fp32 NaN) equals a run prefilled
    with zeros, bit for bit, in out and every gradient (lse[t >= T] and the dvec / lse loads of dead query lanes are read and must be
    discarded); two runs are bitwise; the inference form (save = NULL) gives the same out, bit for bit.

The backward bar.  Measured on an MI355X (first clean run, all five cases): the largest E / N is 0.227 (blocks.0.norm1.bias at the
two-block case (2, 2, 112, 144, 320, 1280, 2); 0.222 for patch_embed.proj.bias there).  Twice that is 0.454, above the 0.25 the bar
may not exceed: BAR = 0.25 (tests/vit_cases.py), 1.10 x the measured maximum.  Per case the largest ratio is 0.0002 (T = 2), 0.057
(T = 33), 0.227 (two blocks), 0.125 (C = 1024), 0.040 (T = 226).  Above 0.125 the stage where the ratio jumps was to be found: there is
none.  Along the backward chain of the two-block case the ratio is, in the order the backward runs, block 1: fc2 0.0001 - 0.0007,
fc1 0.002 - 0.003, norm2 0.008 - 0.010, proj 0.004 - 0.016, qkv 0.016 - 0.022, norm1 0.032 - 0.053; block 0: fc2 0.046 - 0.071,
fc1 0.074 - 0.091, norm2 0.098 - 0.124, proj 0.071 - 0.114, qkv 0.138 - 0.164, norm1 0.174 - 0.227; then the patch embedding 0.173 -
0.222 and pos_embed 0.157.  It grows by about the same factor per rounding point in the one-block cases too (they end at 0.04 - 0.125
where the second block starts): a deviation far below an ulp in front of a bf16 rounding (dy, dh twice, dxn, dob, dS, dqkv) comes out
as a few elements rounded the other way, each a whole ulp, so every rounding point multiplies what reached it, and twelve of them in
a row reach 0.23 where six reach 0.12.  In the max-norm the largest ratio is 0.273 (pos_embed at C = 1024; 0.26 - 0.27
for pos_embed at three cases), held to the separate bar of 1.0.  norm.bias: at most 0.003 of
its fp32 bound.  Forward: the worst |diff| / limit is 0.4995 on the bf16 stages (half an ulp: the correctly rounded value) and 0.4987
on the fp32 ones (x0's class row, one fp32 addition held to 2^-23 |ref|); about 10 % of the unsaved exponentials lie within
their (worst-case) error of a tie.

What these cases found.  In vit.hip, lara_amd/dino.py and the two GEMM entry points: nothing -- every stage of every case is the
correctly rounded value, every padded row and token is zero, NaN-prefilled buffers change no bit, and all four new shapes of the
products (N = 64, 192, 320, 960: partial 256-column tiles the ViT-B / ViT-S widths never produce) are right.  About the checks
themselves (tests/test_vit_bf16.py): norm.bias has no rounding noise to be measured against (N = 0), and a 1/8 scale on the other
side of a rounding is no defect (the same bits).
"""
import ctypes
import functools
import json
import os

import pytest
import torch

from lara_amd import _native
from oracle import vit_bf16 as vr
from tests import vit_cases as vc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = [vc.case_id(c) for c in vc.CASES]
GUARD = 1 << 16
GUARD_BYTE = 0xA5
_LOG, _FWD = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    if not _LOG:
        return
    out = os.environ.get("LARA2DGS_TEST_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_out")
    os.makedirs(out, exist_ok=True)
    l2 = [v["ratio_l2"] for v in _LOG.values() if "ratio_l2" in v]
    mx = [v["ratio_max"] for v in _LOG.values() if "ratio_max" in v]
    with open(os.path.join(out, "vit_stage_errors.json"), "w") as f:
        json.dump({"bar": vc.BAR, "max_ratio_l2": max(l2), "max_ratio_max": max(mx), "forward_worst": _FWD, "tensors": _LOG}, f, indent=1)


# ---------------------------------------------------------------------------------------------- device plumbing

class Guarded:
    """a buffer of the test's own between two guard zones"""

    def __init__(self, nbytes, fill):
        self.whole = torch.full((nbytes + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.buf = self.whole[GUARD:GUARD + nbytes]
        self.buf.fill_(fill)

    def intact(self):
        n = self.buf.numel()
        return bool((self.whole[:GUARD] == GUARD_BYTE).all()) and bool((self.whole[GUARD + n:] == GUARD_BYTE).all())

    def as_f32(self, shape):
        return self.buf.view(torch.float32).view(shape)


def _dims(case, strides):
    N, views, H, W, C, F_, depth = case
    d = _native.VitDims()
    d.N, d.views, d.H, d.W, d.C, d.heads, d.F, d.depth, d.eps = N, views, H, W, C, C // 64, F_, depth, vc.EPS
    for i, s in enumerate(strides):
        d.img_stride[i] = int(s)
    return d


@functools.lru_cache(maxsize=None)
def _device_inputs(case):
    c = vc.case_inputs(case)
    views = case[1]
    if views > 1:
        img = c["rgb"].to(DEV)                                    # [B, views + 1, H, W, 3]: the first `views` are read in place
        s = img.stride()
        strides = (s[0], s[1], s[4], s[2], s[3])
    else:
        img = c["images"].to(DEV)
        s = img.stride()
        strides = (s[0], 0, s[1], s[2], s[3])
    params = [v.to(DEV) for v in c["values"]]
    return {"img": img, "d": _dims(case, strides), "params": params, "ptrs": _native.host_array("p", params),
            "gout": c["gout"].to(DEV).contiguous()}


def _on_device(name, *args):
    """a checked call and a synchronisation; a device error ends the session (nothing run after it on this device would mean anything)"""
    try:
        _native.call(name, DEV, *args)
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{name}: {e}", returncode=3)


def run_device(case, fill, training=True, backward=True):
    """one lara_vit_forward (+ lara_vit_backward) on fresh guarded buffers prefilled with `fill` bytes; asserts the guards"""
    di = _device_inputs(case)
    d, geo = di["d"], vc.case_inputs(case)["geo"]
    ref = ctypes.byref(d)
    out = Guarded(geo["N"] * geo["hw"] * geo["C"] * 4, fill)
    ws = Guarded(_native.query("lara_vit_workspace_bytes", ref, 1 if training else 0), fill)
    save = Guarded(_native.query("lara_vit_save_bytes", ref), fill) if training else None
    bufs = {"out": out, "workspace": ws, "save": save}
    _on_device("lara_vit_forward", ref, di["img"], di["ptrs"], out.buf, save.buf if training else None, ws.buf)
    grads = None
    if training and backward:
        gb = [Guarded(p.numel() * 4, fill) for p in di["params"]]
        bufs.update({f"grads[{i}]": g for i, g in enumerate(gb)})
        _on_device("lara_vit_backward", ref, di["ptrs"], save.buf, di["gout"], _native.host_array("p", [g.buf for g in gb]), ws.buf)
        grads = [g.as_f32(p.shape).clone() for g, p in zip(gb, di["params"])]
    broken = [k for k, b in bufs.items() if b is not None and not b.intact()]
    assert not broken, f"guard zones written beside: {broken}"
    return {"out": out.as_f32((geo["N"], geo["hw"], geo["C"])).clone(), "grads": grads, "save": save.buf if training else None}


def read_save(case, save):
    """the stages of `save` (include/lara_vit.h) as fp64 CPU tensors, keyed as oracle.vit_bf16.forward keys them"""
    geo = vc.case_inputs(case)["geo"]
    d = _device_inputs(case)["d"]
    offs = (ctypes.c_int64 * 17)()
    _native.call("lara_vit_save_offsets", None, ctypes.byref(d), offs, 17)
    o = list(offs)
    M, Mp, C, F_, NH, Tp = geo["M"], geo["Mp"], geo["C"], geo["F"], geo["NH"], geo["Tp"]
    bf, f32 = torch.bfloat16, torch.float32

    def take(off, dt, shape):
        n = (4 if dt == f32 else 2)
        for v in shape:
            n *= v
        return save[off:off + n].view(dt).view(shape).cpu().double()
    got = {"patches": take(o[0], bf, (geo["Pp"], 768)), "xfin": take(o[1], f32, (M, C)), "stf": take(o[2], f32, (M, 2))}
    shapes = {"xin": (f32, (M, C)), "xn1": (bf, (Mp, C)), "st1": (f32, (M, 2)), "q": (bf, (NH, Tp, 64)), "k": (bf, (NH, Tp, 64)),
              "v": (bf, (NH, Tp, 64)), "o": (bf, (Mp, C)), "lse": (f32, (NH, Tp)), "xmid": (f32, (M, C)), "xn2": (bf, (Mp, C)),
              "st2": (f32, (M, 2)), "h": (bf, (Mp, F_))}
    for i in range(geo["depth"]):
        for name, off in zip(vr.BLOCK_STAGES, o[5:]):
            got[f"b{i}.{name}"] = take(o[3] + i * o[4] + off, *shapes[name])
    return got


_RUNS = {}


def device_run(case):
    """the 0xFF-prefilled training run of a case and its stages, shared by the tests of that case"""
    if case not in _RUNS:
        r = run_device(case, 0xFF)
        r["stages"] = read_save(case, r["save"])
        r["stages"]["out"] = r["out"].cpu().double()
        _RUNS[case] = r
    return _RUNS[case]


# ---------------------------------------------------------------------------------------------- (a) forward

@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_forward_stages_teacher_forced(hip_lib, case):
    ck = vc.check_forward(case, device_run(case)["stages"])
    _FWD[vc.case_id(case)] = ck.worst
    assert not ck.fails, "; ".join(ck.fails)


# ---------------------------------------------------------------------------------------------- (b) backward

@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_backward_against_the_faithful_reference(hip_lib, case):
    c = vc.case_inputs(case)
    r = device_run(case)
    _, faithful = vr.backward(c["images"], c["values"], c["geo"], c["gout"], vc.EPS, True, vc.forced_from(r["stages"], c["geo"]))
    got = [g.cpu().double() for g in r["grads"]]
    assert all(bool(torch.isfinite(g).all()) for g in got), "a gradient is not finite"
    failures, worst = vc.compare_gradients(case, got, faithful, _LOG)
    print(f"largest E / N = {worst:.4f}")
    assert not failures, "; ".join(failures)


# ---------------------------------------------------------------------------------------------- (c) memory discipline

@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_memory_discipline(hip_lib, case):
    a = device_run(case)                      # save, workspace, out, gradients prefilled with 0xFF; guards checked inside
    assert bool(torch.isfinite(a["out"]).all())
    names = vc.case_inputs(case)["names"]
    for label, fill in (("prefilled with zeros", 0x00), ("a second run", 0xFF)):
        b = run_device(case, fill)
        assert torch.equal(a["out"], b["out"]), f"out: {label} differs from the 0xFF-prefilled run"
        for n, x, y in zip(names, a["grads"], b["grads"]):
            assert torch.equal(x, y), f"{n}: {label} differs from the 0xFF-prefilled run"
    inf = run_device(case, 0xFF, training=False)
    assert torch.equal(a["out"], inf["out"]), "the inference form (save = NULL) differs from the training forward"
