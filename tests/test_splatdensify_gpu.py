"""`lara_amd.splatdensify` on the device: every output of every case of tests/splatdensify_cases.py equals the host entries' as
integers (twice, on a side stream), but for the centres of split children, which lie within one fp32 spacing (the device's double exp
against the host's); outputs carved out of sentinel-filled buffers at odd offsets leave the sentinels; `refine` with a schedule on
the scene of tests/test_splatrefine_gpu.py; tools/refine_surfels.py with its --densify options.  The figures the tests print, as
measured at writing: profiles/splatdensify_parity.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import splatdensify_cases as C
from tests import splatdensify_restate as S
from tests.test_splatdensify import apply_into_carved, compare_round, fields, make_stats, run_accumulate, run_round

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------ kernel bits

@pytest.mark.parametrize("degree", C.DEGREES)
def test_the_kernels_equal_the_host_entries(hip_lib, degree):
    side = torch.cuda.Stream(DEV)
    off = total = rounds = 0
    for P, d, n, kind in C.round_cases():
        if d != degree:
            continue
        case = C.round_case(P, d, n, kind, seed=P + d + n)
        want = run_round(case)
        with torch.cuda.stream(side):
            first, second = run_round(case, DEV), run_round(case, DEV)
        a, b = compare_round(first, want, (P, d, n, kind))
        off, total, rounds = off + a, total + b, rounds + 1
        for k in ("action", "offset", "counts", "row_source", "row_child"):
            assert np.array_equal(first[k], second[k]), (P, d, n, kind, k)
        for group in ("params", "exp_avg", "exp_avg_sq"):                              # two calls: the same bits, the centres included
            assert all(np.array_equal(S.words(x), S.words(y)) for x, y in zip(first[group], second[group])), (P, d, n, kind, group)
        assert first["five"] == want["five"]
    share = off / max(total, 1)
    print(f"splatdensify parity, kernels against the host entries, SH degree {degree}, {rounds} rounds: {off} of {total} words of split "
          f"children's centres differ ({100.0 * share:.4f} %: the device's double exp against the host's), all within one fp32 spacing; "
          "every other word, action, offset, count and row equal, two calls on a side stream give the same bits")


def test_the_accumulation_kernel_equals_the_host_entry(hip_lib):
    side = torch.cuda.Stream(DEV)
    for P, V in C.accumulate_cases():
        arrays = C.accumulate_case(P, V, seed=P + V)
        want = run_accumulate(arrays)
        with torch.cuda.stream(side):
            for attempt in range(2):
                got = run_accumulate(arrays, DEV)
                assert np.array_equal(S.words(got[0]), S.words(want[0])), (P, V, attempt)
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (P, V, attempt)


def test_outputs_carved_out_of_sentinel_buffers_leave_every_sentinel(hip_lib):
    from lara_amd import _native, splatdensify as D
    from lara_amd._native import host_array
    for P, degree, n in ((1, 0, 2), (65, 1, 3), (257, 3, 2), (1025, 1, 2)):
        case = C.round_case(P, degree, n, "mix" if P > 1 else "split", seed=4)
        want = run_round(case)
        views, source, child, kept = apply_into_carved(case, DEV)
        assert kept, (P, degree, n)
        assert np.array_equal(source, want["row_source"]) and np.array_equal(child, want["row_child"])
        got = dict(want, params=views[0:5], exp_avg=views[5:10], exp_avg_sq=views[10:15])
        compare_round(got, want, (P, degree, n, "carved"))

        # the decision's three outputs and the three statistic rows, carved the same way
        params = fields(case["params"], DEV)
        action = torch.full((P + 11,), 0xEE, dtype=torch.uint8, device=DEV)
        offset = torch.full((3 * P + 11,), -7, dtype=torch.int32, device=DEV)
        counts = torch.full((5 + 6,), -7, dtype=torch.int64, device=DEV)
        st = make_stats(D, case, DEV)
        ws = torch.empty(_native.query("lara_splatdensify_workspace_bytes", P), dtype=torch.uint8, device=DEV)
        _native.call_on("lara_splatdensify_decide", DEV, host_array("d", [float(x) for x in case["plan"]]), P, params[2], params[3],
                        st.grad_sum, st.seen, st.max_radius, action[5:5 + P], offset[3:3 + 3 * P], counts[3:8], ws)
        torch.cuda.synchronize()
        assert np.array_equal(action[5:5 + P].cpu().numpy(), want["action"]) and np.array_equal(offset[3:3 + 3 * P].cpu().numpy(), want["offset"])
        assert np.array_equal(counts[3:8].cpu().numpy(), want["counts"])
        assert bool((action[:5] == 0xEE).all()) and bool((action[5 + P:] == 0xEE).all())
        assert bool((offset[:3] == -7).all()) and bool((offset[3 + 3 * P:] == -7).all())
        assert bool((counts[:3] == -7).all()) and bool((counts[8:] == -7).all())

        arrays = C.accumulate_case(P, 4, seed=P)
        ref = run_accumulate(arrays)
        wholes = [torch.full((P + 9,), -7, dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.int32)]
        st = D.DensifyStats(P, DEV)
        st.grad_sum, st.seen, st.max_radius = (w[3:3 + P] for w in wholes)
        for row, a in zip((st.grad_sum, st.seen, st.max_radius), arrays[2:]):
            row.copy_(torch.from_numpy(a))
        st.accumulate(torch.from_numpy(arrays[0]).to(DEV), torch.from_numpy(arrays[1]).to(DEV))
        torch.cuda.synchronize()
        for w, r in zip(wholes, ref):
            assert np.array_equal(S.words(w[3:3 + P].cpu().numpy()), S.words(r)), (P, "accumulate")
            assert bool((w[:3] == -7).all()) and bool((w[3 + P:] == -7).all()), (P, "accumulate")


def test_an_empty_cloud_launches_nothing_on_the_device(hip_lib):
    from lara_amd import splatdensify as D
    empty = C.round_case(0, 1, 2, "mix")
    params, m, v = (fields(empty[k], DEV) for k in ("params", "exp_avg", "exp_avg_sq"))
    stats = D.DensifyStats(0, DEV)
    stats.accumulate(torch.zeros(0, 3, device=DEV), torch.zeros(4, 0, dtype=torch.int32, device=DEV))
    p2, m2, v2, rep = D.densify(params, m, v, stats, empty["plan"])
    assert rep["P_out"] == 0 and rep["counts"].is_cuda and rep["counts"].tolist() == [0] * 5 and all(t.is_cuda and t.shape[0] == 0 for t in p2 + m2 + v2)


# ------------------------------------------------------------------------------------------------------------------ the loop

STEPS = 12


def _schedule(s, **kw):
    """Rounds after steps 2, 6 and 10 with a threshold of 0 (every surfel is hot); the size limit at the median of the cloud's larger
    log scale, so that a round both clones and splits."""
    from lara_amd import splatdensify as D
    median = float(torch.exp(s["cloud"].scales.max(1).values.median()))
    return D.DensifySchedule(**dict(dict(from_step=2, interval=4, grad_threshold=0.0, percent_dense=0.01, extent=median / 0.01, min_opacity=0.005), **kw))


def test_refine_with_a_schedule_densifies_the_cloud_and_carries_the_moments(hip_lib, monkeypatch):
    from lara_amd import splatrefine as R
    from lara_amd.renderer import Renderer
    from tests.test_splatrefine_gpu import _image, _mse, _perturbed, _scene, _words
    s = _scene()
    start = _perturbed(s)
    rounds = []
    inner = R.SurfelAdam.densify

    def watched(self, stats, plan, **kw):
        before = [t.detach().clone() for t in list(self.params()) + self.exp_avg + self.exp_avg_sq]
        seen = int((stats.seen > 0).sum())
        report = inner(self, stats, plan, **kw)
        rounds.append((before, report, [t.detach().clone() for t in list(self.params()) + self.exp_avg + self.exp_avg_sq], seen))
        return report
    monkeypatch.setattr(R.SurfelAdam, "densify", watched)
    refined, history = R.refine(start, s["cams"], s["rays"], s["targets"], steps=STEPS, sparse=True, renderer=s["renderer"], densify=_schedule(s))
    monkeypatch.undo()
    assert [e["step"] for e in history["densify"]] == [2, 6, 10] and len(rounds) == 3
    P = 1024
    for (before, report, after, seen), entry in zip(rounds, history["densify"]):
        counts = entry["counts"]
        assert counts.is_cuda and counts.dtype == torch.int64 and counts.tolist() == [report[k] for k in ("kept", "cloned", "split", "pruned", "P_out")]
        assert report["kept"] + report["cloned"] + report["split"] + report["pruned"] == P and not entry["capped"]
        assert report["cloned"] > 0 and report["split"] > 0 and seen > 100
        P_out, kept = report["P_out"], report["kept"] + report["cloned"]
        assert P_out == kept + report["cloned"] + 2 * report["split"]
        assert all(t.shape[0] == P_out and bool(torch.isfinite(t).all()) for t in after)           # P after the round, moments' shapes, finite
        assert [t.shape[1:] for t in after] == [t.shape[1:] for t in before]
        src = entry["row_source"].long()
        assert src.shape == (P_out,) and torch.equal(src, report["row_source"].long())
        for old, new in zip(before, after):                                                        # kept rows: parameters and moments travel
            assert np.array_equal(_words(old[src[:kept]]), _words(new[:kept]))
        for new in after[5:]:                                                                      # clones and children: zero moments
            assert not _words(new[kept:]).any()
        P = P_out
    assert refined.n_surfels == P and all(bool(torch.isfinite(t).all()) for t in refined.render_args())
    opt = history["optimiser"]
    assert all(t.shape == p.shape for ts in (opt.exp_avg, opt.exp_avg_sq) for t, p in zip(ts, opt.params())) and opt.steps == STEPS
    assert history["loss"].shape == (STEPS,) and bool(torch.isfinite(history["loss"]).all()) and int(history["skipped"]) == 0

    # no stale activation cache survives a change of P: the loop's renderer draws what a fresh one draws
    loop_image = _image(refined.render_args())
    assert torch.equal(loop_image, _image(refined.render_args(), Renderer(sh_degree=1, white_background=True)))

    control, _ = R.refine(start, s["cams"], s["rays"], s["targets"], steps=STEPS, sparse=True, renderer=s["renderer"])
    print(f"splatdensify parity, refine at 4 views of 64 x 64 from 1 024 surfels, {STEPS} sparse steps, rounds after steps 2, 6, 10 with "
          f"threshold 0: surfels {[r[1]['P_out'] for r in rounds]}, cloned {[r[1]['cloned'] for r in rounds]}, split "
          f"{[r[1]['split'] for r in rounds]}, pruned {[r[1]['pruned'] for r in rounds]}; image MSE start {_mse(start.render_args()):.4e}, "
          f"final {_mse(refined.render_args()):.4e}, control without densification {_mse(control.render_args()):.4e} (reported, not gated)")


def test_a_schedule_that_never_fires_changes_no_bit(hip_lib):
    from lara_amd import splatrefine as R
    from tests.test_splatrefine_gpu import _perturbed, _scene, _words
    s = _scene()
    start = _perturbed(s)
    plain, h0 = R.refine(start, s["cams"], s["rays"], s["targets"], steps=STEPS, sparse=True, renderer=s["renderer"])
    quiet, h1 = R.refine(start, s["cams"], s["rays"], s["targets"], steps=STEPS, sparse=True, renderer=s["renderer"],
                         densify=_schedule(s, from_step=STEPS + 1))
    assert h1["densify"] == [] and "densify" not in h0
    for a, b in zip(plain.render_args(), quiet.render_args()):
        assert np.array_equal(_words(a), _words(b))
    for k in ("loss", "mse", "skipped"):
        assert np.array_equal(_words(h0[k].float()), _words(h1[k].float())), k
    for a, b in zip(h0["optimiser"].exp_avg + h0["optimiser"].exp_avg_sq, h1["optimiser"].exp_avg + h1["optimiser"].exp_avg_sq):
        assert np.array_equal(_words(a), _words(b))


def test_max_surfels_and_the_opacity_reset_inside_refine(hip_lib):
    from lara_amd import splatrefine as R
    from tests.test_splatrefine_gpu import _perturbed, _scene
    s = _scene()
    refined, history = R.refine(_perturbed(s), s["cams"], s["rays"], s["targets"], steps=6, sparse=True, renderer=s["renderer"],
                                densify=_schedule(s, max_surfels=3000, opacity_reset_interval=6, min_opacity=0.0))
    first, second = history["densify"]
    assert not first["capped"] and first["counts"].tolist()[3:] == [0, 2048]      # every surfel is hot and none goes: each leaves two rows
    assert second["capped"] and int(second["counts"][1]) == int(second["counts"][2]) == 0
    assert refined.n_surfels == int(second["counts"][4]) <= int(first["counts"][4])
    assert float(refined.opacity.max()) <= np.float32(np.log(0.01 / 0.99))                         # the reset after step 6 is the last thing done


# ------------------------------------------------------------------------------------------------------------------ the tool

def test_refine_surfels_tool_densifies(hip_lib, tmp_path):
    from lara_amd import splatio
    from tests.test_splatrefine_gpu import FAR, FOV, NEAR, _perturbed, _scene
    s = _scene()
    start = _perturbed(s)
    ply, views, out = str(tmp_path / "start.ply"), str(tmp_path / "views.npz"), str(tmp_path / "refined.ply")
    splatio.write_ply(ply, start)
    np.savez(views, images=(s["targets"].cpu().numpy() * 255.0 + 0.5).astype(np.uint8), c2w=s["c2w"].numpy(), fovx=FOV, fovy=FOV,
             znear=NEAR, zfar=FAR)
    # a fresh child process under its own time limit; nothing below runs when it fails
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "refine_surfels.py"), ply, views,
                          "--steps", "8", "--out", out, "--densify-from", "2", "--densify-interval", "4", "--densify-grad-threshold", "0",
                          "--densify-extent", "1.0", "--densify-min-opacity", "0", "--densify-max-surfels", "4000"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    refined, _ = splatio.read_ply(out)
    with open(str(tmp_path / "refined.json")) as f:
        report = json.load(f)
    assert [r["step"] for r in report["densify_rounds"]] == [2, 6]
    # every surfel is hot and none is pruned: 2 048 rows after the first round; the second would make 4 096 and only prunes instead
    assert refined.n_surfels == report["densify_rounds"][-1]["P_out"] == report["n_surfels_after"] == 2048
    assert [r["capped"] for r in report["densify_rounds"]] == [False, True]
    assert report["n_surfels"] == 1024 and all(set(r) >= {"kept", "cloned", "split", "pruned", "P_out", "capped"} for r in report["densify_rounds"])
