"""`lara_amd.splatdensify` without a GPU: the ``*_host`` entries (the per-row functions of csrc/splatdensify_ops.h compiled for the
CPU) held to the numpy restatement (tests/splatdensify_restate.py) on every case of tests/splatdensify_cases.py -- actions, offsets,
counts, row sources and the statistics' integer rows exactly, grad_sum, copied words, zeroed moments and the children's log scales
bit for bit, the children's centres within one fp32 spacing --; the rows that sit on a limit; `plan`, `densify` with ``max_surfels``,
`reset_opacity`, `SurfelAdam.densify`; the refusals; the binding; the stand-alone sanitizer program."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import splatdensify_cases as C
from tests import splatdensify_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fields(d, device="cpu"):
    return [torch.from_numpy(d[k].copy()).to(device) for k in C.FIELDS]


def make_stats(D, case, device="cpu"):
    st = D.DensifyStats(case["P"], device)
    st.grad_sum, st.seen, st.max_radius = (torch.from_numpy(case[k].copy()).to(device) for k in ("grad_sum", "seen", "max_radius"))
    return st


def run_round(case, device="cpu"):
    """One round through the module's `decide` and `apply` on ``device``: a dict of numpy arrays (lists of five for the clouds)."""
    from lara_amd import splatdensify as D
    params, m, v = (fields(case[k], device) for k in ("params", "exp_avg", "exp_avg_sq"))
    action, offset, counts = D.decide(params, make_stats(D, case, device), case["plan"])
    noise = torch.from_numpy(case["noise"].copy()).to(device)
    p2, m2, v2, source, child, five = D.apply(params, m, v, action, offset, counts, case["plan"], noise=noise)
    cpu = lambda t: t.cpu().numpy()
    return {"action": cpu(action), "offset": cpu(offset), "counts": cpu(counts), "row_source": cpu(source), "row_child": cpu(child),
            "params": [cpu(t) for t in p2], "exp_avg": [cpu(t) for t in m2], "exp_avg_sq": [cpu(t) for t in v2], "five": five}


def within_one_spacing(got, want):
    """fp32 arrays: every |got - want| is at most the spacing of want (both finite)."""
    assert np.isfinite(got).all() and np.isfinite(want).all()
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all())


def compare_round(got, want, what):
    """``got`` against ``want`` (two `run_round` dicts, or a restatement put into that form): everything as integers but the split
    children's centres, which lie within one fp32 spacing.  Returns (children's centre words that differ, children's centre words)."""
    for k in ("action", "offset", "counts", "row_source", "row_child"):
        assert np.array_equal(got[k], want[k]), (what, k)
    is_child = want["row_child"] != S.NO_CHILD
    for group in ("params", "exp_avg", "exp_avg_sq"):
        for i, (a, b) in enumerate(zip(got[group], want[group])):
            assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (what, group, i)
            if group == "params" and i == 0:
                assert np.array_equal(S.words(a)[~is_child], S.words(b)[~is_child]), (what, "centers of rows that are no children")
                assert within_one_spacing(a[is_child], b[is_child]), (what, "children's centres")
            else:
                assert np.array_equal(S.words(a), S.words(b)), (what, group, i)
    return int((S.words(got["params"][0])[is_child] != S.words(want["params"][0])[is_child]).sum()), int(is_child.sum()) * 3


def restated_round(case):
    action, offset, counts = S.decide(case["plan"], case["params"]["opacity"], case["params"]["scales"], case["grad_sum"], case["seen"],
                                      case["max_radius"])
    p, m, v, source, child, _ = S.apply(case["plan"], case["params"], case["exp_avg"], case["exp_avg_sq"], action, offset, counts, case["noise"])
    return {"action": action, "offset": offset, "counts": counts, "row_source": source, "row_child": child,
            "params": [p[k] for k in C.FIELDS], "exp_avg": [m[k] for k in C.FIELDS], "exp_avg_sq": [v[k] for k in C.FIELDS]}


# ------------------------------------------------------------------------------------------------------------------ the rounds

def test_the_host_entries_equal_the_restatement_on_every_round(hip_lib):
    off = total = 0
    seen_actions = set()
    for P, degree, n, kind in C.round_cases():
        case = C.round_case(P, degree, n, kind, seed=P + degree + n)
        got, want = run_round(case), restated_round(case)
        a, b = compare_round(got, want, (P, degree, n, kind))
        off, total = off + a, total + b
        five = got["five"]
        assert five["P_out"] == got["row_source"].shape[0] == got["params"][0].shape[0]
        assert five["kept"] + five["cloned"] + five["split"] + five["pruned"] == P
        if P >= 1:
            pure = {"keep": "kept", "prune": "pruned", "clone": "cloned", "split": "split"}
            if kind in pure:
                assert five[pure[kind]] == P, (P, kind, five)
                assert five["P_out"] == {"keep": P, "prune": 0, "clone": 2 * P, "split": n * P}[kind]
            if kind == "no_clone":
                assert five["cloned"] == 0 and five["split"] > 0 and five["pruned"] > 0
            if kind == "no_split":
                assert five["split"] == 0 and five["cloned"] > 0 and five["pruned"] > 0
            if kind == "no_prune":
                assert five["pruned"] == 0 and five["cloned"] > 0 and five["split"] > 0
        if P >= 1000 and kind.startswith("mix"):
            assert min(five[k] for k in ("kept", "cloned", "split", "pruned")) > P // 50, five
        seen_actions |= set(got["action"].tolist())
    assert seen_actions == {0, 1, 2, 3}
    print(f"splatdensify parity, host entries against the float64 restatement, {len(C.round_cases())} rounds: {off} of {total} words of "
          f"split children's centres differ (the double exp before the one rounding), all within one fp32 spacing; every other word, "
          "action, offset, count and row equal")


def test_the_rows_on_a_limit_take_the_action_the_header_names(hip_lib):
    for kind, want in (("mix", [1, 1, 2, 0, 0, 1, 3, 3, 3, 3, 0, 3]), ("mix_screen", [1, 1, 2, 0, 0, 1, 3, 3, 3, 3, 0, 3]),
                       ("no_clone", [0, 0, 2, 0, 0, 0, 3, 3, 3, 3, 0, 3]), ("no_split", [1, 1, 0, 0, 0, 1, 3, 3, 3, 3, 0, 3]),
                       ("no_prune", [1, 1, 2, 0, 0, 1, 0, 0, None, None, 0, 0])):
        got = run_round(C.round_case(65, 1, 2, kind, seed=1))
        for row, (a, w) in enumerate(zip(got["action"][:C.N_EDGES].tolist(), want)):
            assert w is None or a == w, (kind, row, a, w)
    # the screen limit: a radius above it, and a scale above log_max_world, go; the same rows stay when it is off
    case = C.round_case(65, 1, 2, "mix_screen", seed=1)
    case["max_radius"][3], case["params"]["scales"][4] = 21, (-4.0, -9.0)
    assert run_round(case)["action"][[3, 4]].tolist() == [3, 3]
    case["max_radius"][3] = 20
    assert run_round(case)["action"][3] == 0
    case["plan"][3] = 0.0
    case["max_radius"][3] = 1000
    assert run_round(case)["action"][[3, 4]].tolist() == [0, 0]


def test_the_output_order_is_survivors_then_clones_then_children(hip_lib):
    case = C.round_case(1000, 0, 3, "mix", seed=7)
    got = run_round(case)
    five, src, child, action = got["five"], got["row_source"], got["row_child"], got["action"]
    a, b = five["kept"] + five["cloned"], five["kept"] + 2 * five["cloned"]
    assert np.array_equal(src[:a], np.flatnonzero((action == 0) | (action == 1)))
    assert np.array_equal(src[a:b], np.flatnonzero(action == 1))
    assert np.array_equal(src[b:], np.repeat(np.flatnonzero(action == 2), 3))
    assert (child[:b] == 255).all() and np.array_equal(child[b:], np.tile(np.arange(3, dtype=np.uint8), five["split"]))
    # a split child's log scales shrank by log(0.8 N), its centre moved inside a few sigma of its parent
    par = src[b:]
    assert np.allclose(got["params"][3][b:], case["params"]["scales"][par] - math.log(2.4), rtol=0, atol=1e-6)
    step = np.abs(got["params"][0][b:] - case["params"]["centers"][par]).max(1)
    sigma = np.exp(case["params"]["scales"][par]).max(1) * np.abs(case["noise"][par, child[b:]]).max(1)
    assert (step <= 1.5 * sigma + 1e-7).all() and (step > 0).mean() > 0.99


# ------------------------------------------------------------------------------------------------------------------ the statistics

def run_accumulate(arrays, device="cpu"):
    from lara_amd import splatdensify as D
    grad, radii, grad_sum, seen, max_radius = (torch.from_numpy(a.copy()).to(device) for a in arrays)
    st = D.DensifyStats(grad.shape[0], device)
    st.grad_sum, st.seen, st.max_radius = grad_sum, seen, max_radius
    st.accumulate(grad, radii)
    return [t.cpu().numpy() for t in (st.grad_sum, st.seen, st.max_radius)]


def test_the_host_accumulation_equals_the_restatement(hip_lib):
    for P, V in C.accumulate_cases():
        arrays = C.accumulate_case(P, V, seed=P + V)
        got, want = run_accumulate(arrays), S.accumulate(*arrays)
        assert np.array_equal(S.words(got[0]), S.words(want[0])), (P, V)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (P, V)
        if P >= 63:
            grad, radii, _, seen, _ = arrays
            unseen = ~(radii > 0).any(0)
            bad = ~(np.isfinite(grad[:, 0]) & np.isfinite(grad[:, 1]))
            assert unseen.any() and (bad & ~unseen).any() and (radii < 0).any()
            assert np.array_equal(S.words(got[0])[unseen | bad], S.words(arrays[2])[unseen | bad])           # their bits stay
            assert np.array_equal(got[1][unseen | bad], seen[unseen | bad]) and (got[1][~(unseen | bad)] == seen[~(unseen | bad)] + 1).all()
            assert (got[2][bad & ~unseen] >= arrays[4][bad & ~unseen]).all() and np.array_equal(got[2][unseen], arrays[4][unseen])


# ------------------------------------------------------------------------------------------------------------------ the surface

def test_the_plan_row():
    from lara_amd import splatdensify as D
    row = D.plan(2e-4, 0.01, 3.0, 0.005, 20, 3)
    assert row.dtype == np.float64 and row.shape == (D.PLAN,)
    assert row.tolist() == [2e-4, math.log(0.01 * 3.0), math.log(0.005 / 0.995), 20.0, math.log(0.1 * 3.0), math.log(0.8 * 3), 3.0, 7.0]
    assert D.plan(clone=False)[7] == 6.0 and D.plan(split=False)[7] == 5.0 and D.plan(prune=False)[7] == 3.0
    assert D.plan(min_opacity=0.0)[2] == -math.inf and D.plan()[6] == 2.0 and D.plan()[3] == 0.0
    for bad in (dict(n_split=0), dict(n_split=9), dict(n_split=2.5), dict(extent=0.0), dict(percent_dense=-1.0), dict(min_opacity=1.0),
                dict(grad_threshold=float("nan"))):
        with pytest.raises(ValueError, match=r"lara_amd\.splatdensify"):
            D.plan(**bad)
    s = D.DensifySchedule(from_step=2, interval=4, until_step=11, opacity_reset_interval=6)
    assert [t for t in range(1, 14) if s.fires(t)] == [2, 6, 10] and [t for t in range(1, 14) if s.resets(t)] == [6]
    with pytest.raises(ValueError, match=r"lara_amd\.splatdensify"):
        D.DensifySchedule(interval=0)


def test_densify_caps_at_max_surfels_by_only_pruning(hip_lib):
    from lara_amd import splatdensify as D
    case = C.round_case(1000, 1, 2, "mix", seed=3)
    params, m, v = (fields(case[k]) for k in ("params", "exp_avg", "exp_avg_sq"))
    free = D.densify(params, m, v, make_stats(D, case), case["plan"], seed=5)
    assert free[3]["P_out"] > 1000 and not free[3]["capped"] and free[3]["cloned"] > 0
    again = D.densify(params, m, v, make_stats(D, case), case["plan"], seed=5)                   # the seeded noise: the same bits
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(free[0] + free[1] + free[2], again[0] + again[1] + again[2]))
    other = D.densify(params, m, v, make_stats(D, case), case["plan"], seed=6)
    assert not torch.equal(free[0][0], other[0][0]) and torch.equal(free[0][1], other[0][1])
    p2, m2, v2, rep = D.densify(params, m, v, make_stats(D, case), case["plan"], max_surfels=1000)
    assert rep["capped"] and rep["cloned"] == rep["split"] == 0 and rep["pruned"] == free[3]["pruned"] and rep["P_out"] == 1000 - rep["pruned"]
    src = rep["row_source"].long()
    assert (rep["row_child"] == 255).all()
    for old, new in zip(params + m + v, p2 + m2 + v2):                                             # a pure gather, moments included
        assert torch.equal(old[src].view(torch.int32), new.view(torch.int32))
    assert rep["counts"].tolist() == [rep[k] for k in D.COUNT_KEYS]
    assert all(np.array_equal(S.words(a.numpy()), S.words(case["params"][k])) for a, k in zip(params, C.FIELDS))       # the inputs stay


def test_reset_opacity_clamps_the_logit_and_zeroes_its_moments(hip_lib):
    from lara_amd import splatdensify as D
    case = C.round_case(65, 1, 2, "keep", seed=2)
    params, m, v = (fields(case[k]) for k in ("params", "exp_avg", "exp_avg_sq"))
    params[2][0], params[2][1] = 3.0, -9.0
    params = [p.requires_grad_(True) for p in params]
    version = params[2]._version
    D.reset_opacity(params, m, v, ceiling=0.01)
    lim = math.log(0.01 / 0.99)
    assert params[2]._version > version and params[2].requires_grad and params[2].is_leaf
    now = params[2].detach()
    assert float(now.max()) == np.float32(lim) and float(now[1]) == -9.0 and float(now[0]) == np.float32(lim)
    assert not m[2].any() and not v[2].any() and m[0].any() and v[4].any()
    with pytest.raises(ValueError, match=r"lara_amd\.splatdensify"):
        D.reset_opacity(params, m, v, ceiling=1.0)


def test_surfel_adam_densifies_on_the_host_and_keeps_stepping(hip_lib):
    from lara_amd import splatdensify as D, splatio, splatrefine as R
    case = C.round_case(65, 1, 2, "mix", seed=4)
    opt = R.SurfelAdam(splatio.SurfelCloud(*fields(case["params"])))
    for p in opt.params():
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    before = [t.clone() for t in list(opt.params()) + opt.exp_avg + opt.exp_avg_sq]
    stats = make_stats(D, case)
    rep = opt.densify(stats, case["plan"], seed=1)
    P2 = rep["P_out"]
    assert P2 != 65 and opt.steps == 1 and all(p.shape[0] == P2 and p.is_leaf and p.requires_grad and p.grad is None for p in opt.params())
    assert all(t.shape == p.shape for ts in (opt.exp_avg, opt.exp_avg_sq) for t, p in zip(ts, opt.params()))
    kept = rep["kept"] + rep["cloned"]
    src = rep["row_source"].long()[:kept]
    for old, new in zip(before, list(opt.params()) + opt.exp_avg + opt.exp_avg_sq):
        assert torch.equal(old.detach()[src].view(torch.int32), new.detach()[:kept].view(torch.int32))
    assert all(not t[kept:].any() for t in opt.exp_avg + opt.exp_avg_sq)
    stats.reset(P2)
    assert stats.n_surfels == P2 and not stats.seen.any()
    for p in opt.params():
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    assert opt.steps == 2 and opt.cloud().n_surfels == P2
    opt.reset_opacity(0.01)
    assert float(opt.params()[2].max()) <= np.float32(math.log(0.01 / 0.99)) and not opt.exp_avg[2].any()


def test_the_module_refuses_what_the_kernels_cannot_take(hip_lib):
    from lara_amd import splatdensify as D
    case = C.round_case(8, 1, 2, "mix", seed=0)
    params, m, v = (fields(case[k]) for k in ("params", "exp_avg", "exp_avg_sq"))
    stats = make_stats(D, case)
    action, offset, counts = D.decide(params, stats, case["plan"])
    D.apply(params, m, v, action, offset, counts, case["plan"])
    bad_calls = [
        lambda: D.decide(params[:4], stats, case["plan"]),
        lambda: D.decide([params[0].double()] + params[1:], stats, case["plan"]),
        lambda: D.decide(params, D.DensifyStats(7, "cpu"), case["plan"]),
        lambda: D.decide(params, stats, case["plan"][:7]),
        lambda: D.decide(params, stats, np.array([0, 0, 0, 0, 0, 0, 9.0, 7.0])),
        lambda: D.decide(params, stats, np.array([0, 0, 0, 0, 0, 0, 2.0, 8.0])),
        lambda: D.apply(params, m[:4], v, action, offset, counts, case["plan"]),
        lambda: D.apply(params, m, [t[:7] for t in v], action, offset, counts, case["plan"]),
        lambda: D.apply(params, m, v, action[:7], offset, counts, case["plan"]),
        lambda: D.apply(params, m, v, action, offset.long(), counts, case["plan"]),
        lambda: D.apply(params, m, v, action, offset, counts.int(), case["plan"]),
        lambda: D.apply(params, m, v, action, offset, counts + 1, case["plan"]),
        lambda: D.apply(params, m, v, action, offset, counts, case["plan"], noise=torch.zeros(8, 3, 2)),
        lambda: D.apply(params, m, v, action, offset, counts, case["plan"], noise=torch.zeros(8, 2, 2, dtype=torch.float64)),
        lambda: stats.accumulate(torch.zeros(7, 3), torch.zeros(2, 8, dtype=torch.int32)),
        lambda: stats.accumulate(torch.zeros(8, 3), torch.zeros(2, 8, dtype=torch.int64)),
        lambda: stats.accumulate(torch.zeros(8, 3), torch.zeros(8, dtype=torch.int32)),
        lambda: stats.accumulate(torch.zeros(8, 3), torch.zeros(0, 8, dtype=torch.int32)),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError, match=r"lara_amd\.splatdensify: "):
            call()
            pytest.fail(f"call {i} was taken")


def test_an_empty_cloud_and_an_empty_result_launch_nothing(hip_lib, monkeypatch):
    from lara_amd import splatdensify as D
    gone = C.round_case(65, 1, 2, "prune", seed=0)
    params, m, v = (fields(gone[k]) for k in ("params", "exp_avg", "exp_avg_sq"))
    action, offset, counts = D.decide(params, make_stats(D, gone), gone["plan"])
    monkeypatch.setattr(D._native, "call_on", lambda name, *a: pytest.fail(f"{name} was called"))
    out = D.apply(params, m, v, action, offset, counts, gone["plan"])
    assert out[5]["P_out"] == 0 and out[5]["pruned"] == 65 and out[3].shape == (0,) and out[4].dtype == torch.uint8
    assert [tuple(t.shape) for t in out[0]] == [(0, 3), (0, 4, 3), (0, 1), (0, 2), (0, 4)]
    for degree in C.DEGREES:
        empty = C.round_case(0, degree, 2, "mix")
        params, m, v = (fields(empty[k]) for k in ("params", "exp_avg", "exp_avg_sq"))
        stats = D.DensifyStats(0, "cpu")
        stats.accumulate(torch.zeros(0, 3), torch.zeros(4, 0, dtype=torch.int32))
        p2, m2, v2, rep = D.densify(params, m, v, stats, empty["plan"])
        assert rep["P_out"] == 0 and rep["counts"].tolist() == [0] * 5 and all(t.shape[0] == 0 for t in p2 + m2 + v2)


def test_the_entry_points_refuse_bad_arguments(hip_lib):
    from tests.test_abi_cpu import header_functions_by_file
    case = C.round_case(8, 1, 2, "mix", seed=0)
    host = {n: getattr(hip_lib, n) for n in header_functions_by_file()["lara_splatdensify.h"]}
    row =(ctypes.c_double * 8)(*case["plan"])
    bufs = [case[g][k].copy() for g in ("params", "exp_avg", "exp_avg_sq") for k in C.FIELDS]
    outs = [np.zeros((40,) + b.shape[1:], np.float32) for b in bufs]
    ins_p, outs_p = (ctypes.c_void_p * 15)(*[b.ctypes.data for b in bufs]), (ctypes.c_void_p * 15)(*[b.ctypes.data for b in outs])
    gs, seen, mr = case["grad_sum"].copy(), case["seen"].copy(), case["max_radius"].copy()
    action, offset, counts = np.zeros(8, np.uint8), np.zeros(24, np.int32), np.zeros(5, np.int64)
    grad, radii = np.zeros((8, 3), np.float32), np.ones((2, 8), np.int32)
    src, child, noise = np.zeros(40, np.int32), np.zeros(40, np.uint8), case["noise"].copy()
    ptr = lambda a: a.ctypes.data
    acc = [8, 2, ptr(grad), ptr(radii), ptr(gs), ptr(seen), ptr(mr)]
    dec = [row, 8, ptr(bufs[2]), ptr(bufs[3]), ptr(gs), ptr(seen), ptr(mr), ptr(action), ptr(offset), ptr(counts), None]
    assert host["lara_splatdensify_accumulate_host"](*acc) == 0 and host["lara_splatdensify_decide_host"](*dec) == 0
    P_out, surv = int(counts[4]), int(counts[0] + counts[1])
    app = [row, 1, 8, P_out, surv, ptr(action), ptr(offset), ptr(noise), ins_p, outs_p, ptr(src), ptr(child)]
    assert host["lara_splatdensify_apply_host"](*app) == 0
    for name, good, nullable, tail in (("accumulate", acc, (), ()), ("decide", dec, (10,), ()), ("apply", app, (), ())):
        for fn, extra in ((host[f"lara_splatdensify_{name}_host"], ()), (host[f"lara_splatdensify_{name}"], (None,))):
            dev_entry = bool(extra)                     # (the device entry refuses before it touches a device)
            for k, a in enumerate(good):
                if (isinstance(a, int) and a < 4096) or (k in nullable and not dev_entry):
                    continue
                q = list(good)
                if dev_entry and name == "decide":
                    q[10] = ptr(offset)                 # (a workspace: any address, it is never reached)
                q[k] = None
                assert fn(*q, *extra) == -1, (name, k)
    bad_plan = (ctypes.c_double * 8)(*case["plan"])
    bad_plan[6] = 9.0
    assert host["lara_splatdensify_decide_host"](bad_plan, *dec[1:]) == -1 and host["lara_splatdensify_apply_host"](bad_plan, *app[1:]) == -1
    for change in ({1: -1}, {1: 2 ** 28}):
        q = list(dec)
        for k, val in change.items():
            q[k] = val
        assert host["lara_splatdensify_decide_host"](*q) == -1
    for change in ({1: 4}, {1: -1}, {2: -1}, {3: -1}, {3: 73}, {4: P_out + 1}, {4: 9}):
        q = list(app)
        for k, val in change.items():
            q[k] = val
        assert host["lara_splatdensify_apply_host"](*q) == -1, change
    assert host["lara_splatdensify_accumulate_host"](8, 0, *acc[2:]) == -1 and host["lara_splatdensify_accumulate_host"](-1, 2, *acc[2:]) == -1
    assert host["lara_splatdensify_workspace_bytes"](-1) == -1 and host["lara_splatdensify_workspace_bytes"](2 ** 28) == -1
    assert host["lara_splatdensify_workspace_bytes"](1025) >= (3 * 1025 + 4) * 4
    assert host["lara_splatdensify_accumulate"](0, 2, *acc[2:], None) == 0 and host["lara_splatdensify_apply"](row, 1, 0, 0, 0, *app[5:], None) == 0


def carved(arrays, offsets, rows, device="cpu"):
    """Sentinel-filled buffers of off + rows + 7 rows shaped like ``arrays``: (contiguous views of rows [off, off + rows), buffers)."""
    views, wholes = [], []
    for a, off in zip(arrays, offsets):
        whole = torch.from_numpy(np.full((off + rows + 7,) + tuple(a.shape[1:]), C.SENTINEL, np.uint32).view(np.float32)).to(device)
        wholes.append(whole)
        views.append(whole[off:off + rows])
    return views, wholes


def sentinels_kept(wholes, offsets, rows):
    for whole, off in zip(wholes, offsets):
        w = S.words(whole.cpu().numpy())
        if not ((w[:off] == C.SENTINEL).all() and (w[off + rows:] == C.SENTINEL).all()):
            return False
    return True


CARVE_OFFSETS = (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29)


def apply_into_carved(case, device="cpu"):
    """`decide`, then the apply entry writing into rows carved out of sentinel-filled buffers at odd offsets (the module's `apply`
    allocates its own outputs, so this goes through the shared binding): (the 15 views, row_source, row_child, all sentinels kept)."""
    from lara_amd import _native, splatdensify as D
    from lara_amd._native import host_array
    dev = torch.device(device)
    params, m, v = (fields(case[k], device) for k in ("params", "exp_avg", "exp_avg_sq"))
    action, offset, counts = D.decide(params, make_stats(D, case, device), case["plan"])
    five = dict(zip(D.COUNT_KEYS, counts.tolist()))
    P_out = five["P_out"]
    views, wholes = carved(params + m + v, CARVE_OFFSETS, P_out, device)
    rows_whole = torch.full((P_out + 11,), -7, dtype=torch.int32, device=dev)
    child_whole = torch.full((P_out + 11,), 77, dtype=torch.uint8, device=dev)
    noise = torch.from_numpy(case["noise"].copy()).to(dev)
    _native.call_on("lara_splatdensify_apply", dev, host_array("d", [float(x) for x in case["plan"]]), case["degree"], case["P"], P_out,
                    five["kept"] + five["cloned"], action, offset, noise, host_array("p", params + m + v), host_array("p", views),
                    rows_whole[3:3 + P_out], child_whole[5:5 + P_out])
    if dev.type == "cuda":
        torch.cuda.current_stream(dev).synchronize()
    kept = sentinels_kept(wholes, CARVE_OFFSETS, P_out)
    kept = kept and bool((rows_whole[:3] == -7).all()) and bool((rows_whole[3 + P_out:] == -7).all())
    kept = kept and bool((child_whole[:5] == 77).all()) and bool((child_whole[5 + P_out:] == 77).all())
    return [t.cpu().numpy() for t in views], rows_whole[3:3 + P_out].cpu().numpy(), child_whole[5:5 + P_out].cpu().numpy(), kept


def test_outputs_carved_out_of_sentinel_buffers_leave_every_sentinel(hip_lib):
    for P, degree, n in ((1, 0, 2), (65, 1, 3), (257, 3, 2)):
        case = C.round_case(P, degree, n, "mix" if P > 1 else "split", seed=4)
        want = run_round(case)
        views, source, child, kept = apply_into_carved(case)
        assert kept, (P, degree, n)
        assert np.array_equal(source, want["row_source"]) and np.array_equal(child, want["row_child"])
        for got, ref in zip(views, want["params"] + want["exp_avg"] + want["exp_avg_sq"]):
            assert np.array_equal(S.words(got), S.words(ref))


# ------------------------------------------------------------------------------------------------------------------ the binding, the build

def test_the_modules_binding_equals_the_headers_prototypes(hip_lib):
    """The header lies under include/ and its seven functions are rows of ``_native.SIGNATURES`` (tests/test_abi_cpu.py holds the rows
    to the prototypes, kind by kind): the library exports all, the stream is on the device entries alone, the unit is built with
    -ffp-contract=off, and the header's plan and span are the module's."""
    from lara_amd import _native, splatdensify as D
    from tests.test_abi_cpu import header_functions_by_file
    names = ["lara_splatdensify_accumulate", "lara_splatdensify_accumulate_host", "lara_splatdensify_apply", "lara_splatdensify_apply_host",
             "lara_splatdensify_decide", "lara_splatdensify_decide_host", "lara_splatdensify_workspace_bytes"]
    assert sorted(header_functions_by_file()["lara_splatdensify.h"]) == names
    assert set(names) <= set(_native._SIGS) and all(hasattr(hip_lib, n) for n in names)
    for name in names:
        assert _native._SIGS[name][2] == (not name.endswith(("_host", "_bytes"))), name
    text = open(os.path.join(ROOT, "lara_amd", "csrc", "Makefile")).read()
    assert "FLAGS_splatdensify := -ffp-contract=off\n" in text and " splatdensify" in text.split("OBJS")[1].splitlines()[0]
    header = open(os.path.join(ROOT, "include", "lara_splatdensify.h")).read()
    assert f"#define LARA_SPLATDENSIFY_PLAN {D.PLAN}\n" in header and f"#define LARA_SPLATDENSIFY_SPAN {D.SPAN}\n" in header
    assert "[RECALLED" in header and "PER RENDER CALL" in header and "leaves no descendants" in header


def test_nothing_on_the_default_routes_imports_the_module():
    code = ("import sys, lara_amd, lara_amd.renderer, lara_amd.loss, lara_amd.splatio, lara_amd.splatxform, lara_amd.splatrefine; "
            "print('lara_amd.splatdensify' in sys.modules)")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0 and run.stdout.strip() == "False", run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------------------------ the hostcheck

def test_the_stand_alone_host_program_ends_without_a_report():
    """csrc/splatdensify_ops.h and the host entries' loops as a stand-alone program under AddressSanitizer and UBSan (nothing
    loaded into python, no device): every integer and every word but the children's centres equal to the restatement's, those
    within one fp32 spacing, exit code 0, no report."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "splatdensify_hostcheck.py")], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "values off the restatement 0" in run.stdout and "centre words beyond one spacing 0" in run.stdout, run.stdout
    assert "sanitizer reports: none" in run.stdout, run.stdout
