"""The bf16-faithful fp64 reference of the DINO ViT encoder (oracle/vit_bf16.py) held to account, on the CPU, before the device is
held to it (tests/test_vit_stages_gpu.py).  Every assertion rests on the reference alone:

  * roundings off, it IS tests/dino_restate.RestatedViT in fp64: the tokens and every autograd gradient, to 1e-10, at every case;
  * its rounding markers agree bit for bit with torch's bf16 cast (ties, the denormal range, the overflow boundary);
  * the yardstick of the backward bar, N = ||faithful - unrounded|| / ||unrounded||, is bf16 noise (1e-3 <= N <= 5e-2) for every
    gradient of every case -- but one: norm.bias, the column sums of the fp32 output gradient, has N = 0 by construction (no
    rounding lies in front of it) and is held to the fp32 bound of such a sum instead of a multiple of N;
  * the reference passes its own stage checks (tests/vit_cases.check_forward), and every defect of oracle.vit_bf16.DEFECTS, built
    into a copy of the reference and treated exactly as the device is treated, is caught at one case at least: it breaks a
    per-element limit of the forward, or puts a gradient at E / N >= 2 BAR against the faithful reference run on its own forward.

What the defect list found about the list itself: "the 1/8 scale applied after the rounding" is no defect.  1/8 is a power of two,
so bf16(acc) / 8 and bf16(acc / 8) are the same bits unless the result is subnormal (|acc| < 2^-123); no case can tell them
apart and test_scale_and_rounding_commute asserts that.  The neighbouring mistake that does change values -- the scores rounded
to bf16 before the scale ("score_rounded") -- stands in the list beside it.
"""
import pytest
import torch

from oracle import vit_bf16 as vr
from oracle.voltrans_bf16 import rb, rf, round_bf16
from tests import vit_cases as vc
from tests.dino_restate import RestatedViT

IDS = [vc.case_id(c) for c in vc.CASES]


def test_markers_round_like_torch_bfloat16():
    f32 = torch.float32
    special = torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 1.0 + 2.0 ** -8 + 2.0 ** -20, 3.3895313892515355e38,
                            3.3961775292304601e38, -3.3961775292304601e38, 3.4028234663852886e38, 1e-40, -1e-40, 9.1835e-41, 4.5918e-41,
                            1.4e-45, 1.1754943508222875e-38, float("inf"), -float("inf")], dtype=f32)
    # ties of every parity around 1 and below 2, and the whole denormal range in half-ulp steps
    ties = torch.cat([1.0 + (torch.arange(64, dtype=f32) + 0.5) * 2.0 ** -7, 2.0 - (torch.arange(64, dtype=f32) + 0.5) * 2.0 ** -8,
                      torch.arange(1, 260, dtype=f32) * 2.0 ** -134])
    rnd = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * torch.logspace(-44, 30, 4096)
    v = torch.cat([special, ties, rnd.to(f32)])
    want = v.to(torch.bfloat16).to(f32)
    assert torch.equal(rf(v.double()).to(f32).view(torch.int32), want.view(torch.int32))
    assert torch.equal(round_bf16(v).view(torch.int32), want.view(torch.int32))
    assert torch.isnan(round_bf16(torch.tensor([float("nan")]))).all()
    fin = torch.isfinite(v)
    x = v[fin].double().requires_grad_(True)
    rb(x).backward(x.detach())                                   # rb: identity forward, rounded gradient
    assert torch.equal(x.grad.to(f32).view(torch.int32), want[fin].view(torch.int32))
    y = x.detach().clone().requires_grad_(True)
    rf(y).backward(torch.full_like(y, 1.0 + 2.0 ** -12))           # rf: rounded forward, gradient untouched
    assert torch.equal(y.grad, torch.full_like(y, 1.0 + 2.0 ** -12))
    assert torch.equal(rf(y, False), y) and torch.equal(rb(y, False), y)


@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_unrounded_reference_is_the_restatement(case):
    c = vc.case_inputs(case)
    geo = c["geo"]
    m = RestatedViT(geo["C"], geo["depth"], geo["heads"], geo["F"], (geo["h"], geo["w"]), vc.EPS).double()
    assert [n for n, _ in m.named_parameters()] == c["names"]
    with torch.no_grad():
        for (n, p), v in zip(m.named_parameters(), c["values"]):
            p.copy_(v.double().reshape(p.shape))
    out = m(c["images"].double())
    (out * c["gout"].double()).sum().backward()
    stages, grads = vc.reference(case, False)

    def close(got, ref, name):
        err = float((got.reshape(-1) - ref.reshape(-1)).abs().max() / ref.abs().max())
        assert err <= 1e-10, f"{name}: {err:.3e}"
    close(stages["out"], out.detach(), "out")
    for (n, p), g in zip(m.named_parameters(), grads):
        close(g, p.grad, n)


@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_yardstick_measures_bf16_noise(case):
    """outside [1e-3, 5e-2] the backward bar (a multiple of N) would not be measuring against rounding noise"""
    bad = []
    for name, (n2, _) in vc.yardstick(case).items():
        print(f"{name:28s} N = {n2:.3e}")
        if name == "norm.bias":
            # the final norm's beta gradient is the column sum of the fp32 `grad`: the one tensor no rounding reaches, whatever the
            # input scales.  It cannot be measured in units of N; tests/vit_cases.compare_gradients holds it to an fp32 sum's bound.
            assert n2 == 0.0
            continue
        if not 1e-3 <= n2 <= 5e-2:
            bad.append(f"{name}: N = {n2:.3e}")
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("case", vc.CASES, ids=IDS)
def test_reference_passes_its_own_stage_checks(case):
    """the bounds are derived, not fitted: the faithful reference itself (fp64 accumulation, the correctly rounded value everywhere)
    must sit at half an ulp of every bf16 stage and at zero of every fp32 stage"""
    ck = vc.check_forward(case, vr.device_layout(vc.reference(case, True)[0], vc.case_inputs(case)["geo"]))
    assert not ck.fails, "; ".join(ck.fails)
    assert ck.worst["bf16"] <= 0.5 + 1e-9 and ck.worst["fp32"] <= 1e-6


def _seen(defect, case):
    """the defective reference treated as the device is: (what the forward checks say, the largest E / N of its gradients against
    the faithful reference evaluated on the defective forward)"""
    c = vc.case_inputs(case)
    stages, grads = vc.reference(case, True, (defect,))
    got = vr.device_layout(stages, c["geo"], (defect,))
    ck = vc.check_forward(case, got)
    _, faithful = vr.backward(c["images"], c["values"], c["geo"], c["gout"], vc.EPS, True, vc.forced_from(got, c["geo"]))
    _, worst = vc.compare_gradients(case, grads, faithful, label=defect)
    return ck.fails, worst


@pytest.mark.parametrize("defect", [d for d in vr.DEFECTS if d != "scale_after_rounding"])
def test_defect_is_seen(defect):
    report = []
    for case in vc.CASES:
        fails, worst = _seen(defect, case)
        report.append(f"{vc.case_id(case)}: {len(fails)} forward stages fail, largest E / N = {worst:.3f}")
        if fails or worst >= 2 * vc.BAR:
            print(f"{defect} ({vr.DEFECTS[defect]}) seen at {report[-1]} {fails[:2]}")
            return
    pytest.fail(f"{defect} ({vr.DEFECTS[defect]}) passes every check: " + "; ".join(report))


@pytest.mark.parametrize("case", vc.CASES[:3], ids=IDS[:3])
def test_scale_and_rounding_commute(case):
    """module docstring: a power-of-two scale on either side of the rounding gives the same bits"""
    _, a = vc.reference(case, True)
    _, b = vc.reference(case, True, ("scale_after_rounding",))
    for n, x, y in zip(vc.case_inputs(case)["names"], a, b):
        assert torch.equal(x, y), n
