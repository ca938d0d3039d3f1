"""`lara_amd.splatrefine` without a GPU: `adam_step` through ``lara_splatadam_step_host`` (the per-word function of
csrc/splatadam_ops.h compiled for the CPU) held to the numpy float64 restatement (tests/splatrefine_restate.py) as 32-bit words on
every case of tests/splatrefine_cases.py; the first dense step against ``torch.optim.Adam`` in float64; the gates; fields carved out
of sentinel-filled buffers; the refusals; `plan`, `SurfelAdam`'s bookkeeping; the binding; the stand-alone sanitizer program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import splatrefine_cases as C
from tests import splatrefine_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tensors(parts, device="cpu"):
    """The four dicts of a case as four lists of tensors (copies)."""
    return [[torch.from_numpy(d[k].copy()).to(device) for k in C.FIELDS] for d in parts]


def host_step(parts, row, visible=None, zero_grads=False):
    """One step through the module on the host: (the four lists of tensors after it, the counter's value)."""
    from lara_amd import splatrefine as R
    p, g, m, v = tensors(parts)
    vis = None if visible is None else torch.from_numpy(visible.copy())
    counters = R.adam_step(p, g, m, v, row, visible=vis, zero_grads=zero_grads)
    return (p, g, m, v), int(counters.item())


def off_words(got, want):
    """How many 32-bit words of the lists of tensors ``got`` differ from the dicts ``want``."""
    return sum(int((S.words(t.detach().numpy()) != S.words(d[k])).sum()) for ts, d in zip(got, want) for k, t in zip(C.FIELDS, ts))


# ------------------------------------------------------------------------------------------------------------------ the arithmetic

@pytest.mark.parametrize("degree", C.DEGREES)
def test_the_host_entry_equals_the_restatement_as_words(hip_lib, degree):
    """Both sides are the same sequence of correctly rounded IEEE operations: no word may differ, and the counts agree."""
    from lara_amd import splatrefine as R
    n_cases = 0
    for P, d, t, moments, sparse in C.all_cases():
        if d != degree:
            continue
        parts = C.case(P, d, moments, seed=P + d)
        row = R.plan(t, C.LRS)
        assert S.words(row).tolist() == S.words(S.plan(t, C.LRS)).tolist()
        visible = C.mask(P, seed=d) if sparse else None
        for zero in (False, True):
            *want, skipped = S.step(row, *parts, visible=visible, zero_grads=zero)
            got, counted = host_step(parts, row, visible, zero)
            assert off_words(got, want) == 0, (P, d, t, moments, sparse, zero)
            assert counted == skipped, (P, d, t, moments, sparse, zero)
            if P >= 63 and not sparse:
                assert skipped == 5 * C.N_NONFINITE                                # every field met every non-finite word
        n_cases += 1
    assert n_cases == len(C.SIZES) * len(C.STEPS) * 4


def test_the_plan_row():
    from lara_amd import splatrefine as R
    row = R.plan(3)
    assert row.dtype == np.float64 and row.shape == (R.PLAN,)
    assert row.tolist() == [0.9, 1.0 - 0.9, 0.999, 1.0 - 0.999, 1.0 - 0.9 ** 3, (1.0 - 0.999 ** 3) ** 0.5, 1e-15, 1.6e-4, 2.5e-3, 2.5e-3 / 20, 0.05,
                            5e-3, 1e-3]
    assert R.plan(10 ** 6)[4] == 1.0 and R.plan(10 ** 6)[5] == 1.0
    assert R.plan(1, {"opacity": 0.5})[7:13].tolist() == [1.6e-4, 2.5e-3, 2.5e-3 / 20, 0.5, 5e-3, 1e-3]
    assert R.plan(1, range(1, 7))[7:13].tolist() == [1, 2, 3, 4, 5, 6]
    for bad in (dict(step=0), dict(step=1, betas=(1.0, 0.999)), dict(step=1, eps=-1.0), dict(step=1, lrs={"colour": 1.0}), dict(step=1, lrs=[1.0] * 5)):
        with pytest.raises(ValueError, match="lara_amd.splatrefine"):
            R.plan(**bad)


def test_the_first_dense_step_is_within_one_spacing_of_torch_adam_in_float64(hip_lib):
    """``torch.optim.Adam`` (single tensor, float64, CPU) over the same values from zero moments, the SH tensor split into its
    coefficient 0 and the rest for the two rates.  torch orders the operations differently (addcdiv: (-step_size m) / denom), which
    can move the double by an ulp before the one rounding: every parameter within one fp32 spacing of torch's result rounded to fp32."""
    from lara_amd import splatrefine as R
    unequal = total = 0
    for degree in C.DEGREES:
        parts = C.case(1000, degree, moments=False, seed=degree, special=False)
        for k in C.FIELDS:                               # the finite special words only: torch has no gate
            at, what = C.special_slots(parts[1][k].size)
            keep = np.isfinite(what)
            parts[1][k].reshape(-1)[at[keep]] = what[keep]
        (p, _, _, _), counted = host_step(parts, R.plan(1, C.LRS, eps=1e-15))
        assert counted == 0
        params, grads = parts[0], parts[1]
        pieces = [("centers", slice(None), 0), ("shs", (slice(None), slice(0, 1)), 1), ("shs", (slice(None), slice(1, None)), 2),
                  ("opacity", slice(None), 3), ("scales", slice(None), 4), ("rotations", slice(None), 5)]
        leaves = []
        for k, sl, rate in pieces:
            leaf = torch.from_numpy(params[k][sl].astype(np.float64)).requires_grad_(True)
            leaf.grad = torch.from_numpy(grads[k][sl].astype(np.float64))
            leaves.append(leaf)
        opt = torch.optim.Adam([{"params": [leaf], "lr": C.LRS[rate]} for leaf, (_, _, rate) in zip(leaves, pieces)], betas=(0.9, 0.999),
                               eps=1e-15, foreach=False)
        opt.step()
        for leaf, (k, sl, _) in zip(leaves, pieces):
            if leaf.numel() == 0:
                continue
            got = p[C.FIELDS.index(k)].numpy()[sl].astype(np.float64)
            want = leaf.detach().numpy().astype(np.float32)
            assert (np.abs(got - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all(), (degree, k)
            unequal += int((S.words(np.ascontiguousarray(p[C.FIELDS.index(k)].numpy()[sl])) != S.words(np.ascontiguousarray(want))).sum())
            total += want.size
            assert (S.words(np.ascontiguousarray(want)) != S.words(np.ascontiguousarray(params[k][sl]))).mean() > 0.5      # a step was taken
    print(f"splatrefine parity, first dense step against torch.optim.Adam in float64: {unequal} of {total} parameter words unequal, "
          "all within one fp32 spacing")


# ------------------------------------------------------------------------------------------------------------------ the gates

def test_invisible_rows_keep_their_parameter_and_moment_words(hip_lib):
    from lara_amd import splatrefine as R
    parts = C.case(1000, 1, moments=True, seed=5)
    visible = C.mask(1000, seed=5)
    assert 300 < int((visible == 0).sum()) < 700
    (p, g, m, v), _ = host_step(parts, R.plan(7, C.LRS), visible)
    gone = visible == 0
    for k, t_p, t_g, t_m, t_v in zip(C.FIELDS, p, g, m, v):
        for got, before in ((t_p, parts[0][k]), (t_m, parts[2][k]), (t_v, parts[3][k])):
            assert np.array_equal(S.words(got.numpy())[gone], S.words(before)[gone]), k
            moved = S.words(got.numpy())[~gone] != S.words(before)[~gone]
            assert moved.mean() > 0.9, k
        assert np.array_equal(S.words(t_g.numpy()), S.words(parts[1][k])), k           # the gradients were read, not written


def test_non_finite_gradients_skip_their_elements_and_are_counted(hip_lib):
    from lara_amd import splatrefine as R
    parts = C.case(65, 3, moments=True, seed=9)
    (p, g, m, v), counted = host_step(parts, R.plan(2, C.LRS))
    n_bad = sum(int((~np.isfinite(parts[1][k])).sum()) for k in C.FIELDS)
    assert counted == n_bad == 5 * C.N_NONFINITE
    for k, t_p, t_m, t_v in zip(C.FIELDS, p, m, v):
        bad = ~np.isfinite(parts[1][k])
        for got, before in ((t_p, parts[0][k]), (t_m, parts[2][k]), (t_v, parts[3][k])):
            assert np.array_equal(S.words(got.numpy())[bad], S.words(before)[bad]), k
        assert np.isfinite(t_p.numpy()).all() and np.isfinite(t_m.numpy()).all(), k
        assert (np.isinf(t_v.numpy()) == (np.abs(parts[1][k]) == np.float32(1e30))).all(), k       # (1 - b2) g^2 beyond fp32, as in torch's fp32 Adam
    # the counter is added to, never zeroed; a masked row's non-finite gradient is not looked at
    ts = tensors(parts)
    counters = torch.tensor([100], dtype=torch.int64)
    hidden = torch.zeros(65, dtype=torch.uint8)
    assert R.adam_step(*ts, R.plan(2, C.LRS), counters=counters) is counters and int(counters) == 100 + n_bad
    R.adam_step(*tensors(parts), R.plan(2, C.LRS), visible=hidden, counters=counters)
    assert int(counters) == 100 + n_bad


def test_zero_grads_leaves_plus_zero_in_every_gradient_word_and_changes_nothing_else(hip_lib):
    from lara_amd import splatrefine as R
    parts = C.case(257, 1, moments=True, seed=2)
    for visible in (None, C.mask(257, seed=2), np.zeros(257, np.uint8)):
        plain, c0 = host_step(parts, R.plan(3, C.LRS), visible, zero_grads=False)
        zeroed, c1 = host_step(parts, R.plan(3, C.LRS), visible, zero_grads=True)
        assert c0 == c1
        for which in (0, 2, 3):
            for a, b in zip(plain[which], zeroed[which]):
                assert np.array_equal(S.words(a.numpy()), S.words(b.numpy()))
        for t in zeroed[1]:
            assert not S.words(t.numpy()).any()                                        # +0.0 is the all-zero word


def test_the_sh_rates_land_on_their_words(hip_lib):
    """With equal gradients from zero moments the first step moves every word by its rate (m' / sqrt(v') is 1 up to rounding)."""
    from lara_amd import splatrefine as R
    P = 70
    for degree in (1, 3):
        n = (degree + 1) ** 2
        parts = C.case(P, degree, moments=False, seed=1, special=False)
        for k in C.FIELDS:
            parts[0][k][...] = 0.0
            parts[1][k][...] = 0.25
        lrs = (1.0, 2.0, 4.0, 8.0, 16.0, 32.0)
        (p, _, _, _), _ = host_step(parts, R.plan(1, lrs, eps=0.0))
        want = {"centers": np.full((P, 3), -1.0), "opacity": np.full((P, 1), -8.0), "scales": np.full((P, 2), -16.0), "rotations": np.full((P, 4), -32.0),
                "shs": np.concatenate([np.full((P, 1, 3), -2.0), np.full((P, n - 1, 3), -4.0)], axis=1)}
        for k, t in zip(C.FIELDS, p):
            assert np.allclose(t.numpy(), want[k], rtol=1e-6, atol=0), (degree, k)


# ------------------------------------------------------------------------------------------------------------------ layout, refusals

def carved(arrays, offsets, device="cpu"):
    """Each array as a contiguous view of rows [off, off + P) of a sentinel-filled buffer of off + P + 7 rows: (views, buffers)."""
    views, wholes = [], []
    for a, off in zip(arrays, offsets):
        whole = np.full((off + a.shape[0] + 7,) + a.shape[1:], C.SENTINEL, np.uint32).view(np.float32)
        whole[off:off + a.shape[0]] = a
        whole = torch.from_numpy(whole).to(device)
        wholes.append(whole)
        views.append(whole[off:off + a.shape[0]])
    return views, wholes


def sentinels_kept(wholes, offsets, P):
    for whole, off in zip(wholes, offsets):
        w = S.words(whole.cpu().numpy())
        if not ((w[:off] == C.SENTINEL).all() and (w[off + P:] == C.SENTINEL).all()):
            return False
    return True


CARVE_OFFSETS = (1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 33, 35, 37, 39)


def test_fields_carved_out_of_sentinel_buffers_leave_every_sentinel(hip_lib):
    from lara_amd import splatrefine as R
    for P, degree in ((1, 0), (65, 1), (257, 3)):
        parts = C.case(P, degree, moments=True, seed=4)
        visible = C.mask(P, seed=4)
        row = R.plan(5, C.LRS)
        want, skipped = host_step(parts, row, visible, zero_grads=True)
        flat = [d[k] for d in parts for k in C.FIELDS]
        views, wholes = carved(flat, CARVE_OFFSETS)
        assert all(t.is_contiguous() and t.storage_offset() % 2 == 1 for t in views[2::5])          # (opacity: an odd word offset)
        counters = R.adam_step(views[0:5], views[5:10], views[10:15], views[15:20], row, visible=torch.from_numpy(visible), zero_grads=True)
        assert int(counters) == skipped
        for got, ref in zip(views, [t for ts in want for t in ts]):
            assert np.array_equal(S.words(got.numpy()), S.words(ref.numpy()))
        assert sentinels_kept(wholes, CARVE_OFFSETS, P)


def test_adam_step_refuses_what_the_kernel_cannot_take(hip_lib):
    from lara_amd import splatrefine as R
    parts = C.case(8, 1, moments=True, seed=0, special=False)
    row = R.plan(1)

    def call(change=None, **kw):
        ts = tensors(parts)
        if change:
            change(ts)
        return R.adam_step(*ts, kw.pop("plan", row), **kw)

    call()

    def put(which, field, value):
        def change(ts):
            ts[which][field] = value(ts[which][field])
        return change

    bad = [
        put(0, 0, lambda t: t.t().contiguous().t()), put(1, 1, lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)),      # not contiguous
        put(2, 4, lambda t: torch.zeros(8, 8)[:, ::2]), put(3, 3, lambda t: torch.zeros(8, 4)[:, ::2]),
        put(0, 2, lambda t: t.double()), put(1, 0, lambda t: t.half()), put(2, 1, lambda t: t.double()), put(3, 4, lambda t: t.to(torch.int32)),
        put(1, 0, lambda t: t[:7].contiguous()), put(2, 1, lambda t: t[:, :1].contiguous()), put(3, 2, lambda t: t.reshape(-1)),
        put(1, 3, lambda t: torch.zeros(8, 3)), put(0, 1, lambda t: torch.zeros(8, 5, 3)), put(0, 4, lambda t: torch.zeros(8, 3)),
        put(1, 0, lambda t: t.to("meta")), put(2, 2, lambda t: t.to("meta")), put(0, 3, lambda t: t.to("meta")),                 # mixed devices
    ]
    for change in bad:
        with pytest.raises(ValueError, match=r"lara_amd\.splatrefine: "):
            call(change)
    for kw in (dict(visible=torch.ones(7, dtype=torch.uint8)), dict(visible=torch.ones(8)), dict(visible=torch.ones(16, dtype=torch.uint8)[::2]),
               dict(visible=torch.ones(8, dtype=torch.uint8, device="meta")), dict(counters=torch.zeros(1, dtype=torch.int32)),
               dict(counters=torch.zeros(2, dtype=torch.int64)), dict(plan=row[:12]), dict(plan=np.zeros((13, 1)))):
        with pytest.raises(ValueError, match=r"lara_amd\.splatrefine: "):
            call(**kw)
    with pytest.raises(ValueError, match=r"lara_amd\.splatrefine: "):
        R.adam_step(tensors(parts)[0][:4], *tensors(parts)[1:], row)


def test_an_empty_cloud_launches_nothing(hip_lib, monkeypatch):
    from lara_amd import splatrefine as R
    for through in ("call_on", "call"):
        monkeypatch.setattr(R._native, through, lambda name, *a: pytest.fail(f"{name} was called for an empty cloud"))
    for degree in C.DEGREES:
        counters = R.adam_step(*tensors(C.case(0, degree, moments=False)), R.plan(1), visible=torch.zeros(0, dtype=torch.uint8), zero_grads=True)
        assert int(counters) == 0


def test_the_entry_points_refuse_bad_arguments(hip_lib):
    from lara_amd import splatrefine as R
    parts = C.case(4, 1, moments=True, special=False)
    bufs = [d[k].copy() for d in parts for k in C.FIELDS]
    p = [b.ctypes.data for b in bufs]
    row = (ctypes.c_double * 13)(*R.plan(1))
    count = np.zeros(1, np.int64)
    host, dev = hip_lib.lara_splatadam_step_host, hip_lib.lara_splatadam_step
    assert host(row, 1, 4, *p, None, 0, count.ctypes.data) == 0
    for fn, tail in ((host, ()), (dev, (None,))):          # (the device entry refuses before it touches a device)
        for k in range(20):
            q = list(p)
            q[k] = None
            assert fn(row, 1, 4, *q, None, 0, count.ctypes.data, *tail) == -1, k
        assert fn(None, 1, 4, *p, None, 0, count.ctypes.data, *tail) == -1
        assert fn(row, 1, 4, *p, None, 0, None, *tail) == -1
        for degree, P in ((-1, 4), (4, 4), (1, -1), (1, 2 ** 41)):
            assert fn(row, degree, P, *p, None, 0, count.ctypes.data, *tail) == -1, (degree, P)
    assert dev(row, 1, 0, *p, None, 0, count.ctypes.data, None) == 0                   # empty: nothing is launched


def test_the_device_entry_refuses_a_grid_beyond_the_launch_limit(hip_lib):
    """2^40 surfels at SH degree 3 are 2^40 * 48 / 256 workgroups of the shs field alone, far beyond the 2^31 - 1 a launch takes: the
    device entry passes its argument check (P <= 2^40, no null pointer) and refuses while it lays out the grid, before it touches a
    device.  The 22 addresses are never dereferenced.  This is the one route to that refusal: splatdensify caps P at 2^27."""
    from lara_amd import splatrefine as R
    row = (ctypes.c_double * 13)(*R.plan(1))
    addresses = [4096 * (k + 1) for k in range(22)]
    assert len(set(addresses)) == 22
    dev = hip_lib.lara_splatadam_step
    assert dev(row, 3, 2 ** 40, *addresses[:20], addresses[20], 0, addresses[21], None) == -1
    assert dev(row, 3, 0, *addresses[:20], addresses[20], 0, addresses[21], None) == 0


# ------------------------------------------------------------------------------------------------------------------ the optimiser object

def test_surfel_adam_on_the_host_steps_counts_and_restores(hip_lib):
    from lara_amd import splatio, splatrefine as R
    parts = C.case(65, 1, moments=False, seed=3, special=False)
    cloud = splatio.SurfelCloud(*(torch.from_numpy(parts[0][k]) for k in C.FIELDS))
    opt = R.SurfelAdam(cloud, lrs=dict(zip(R.LR_KEYS, C.LRS)))
    assert all(p.is_leaf and p.requires_grad and p.is_contiguous() for p in opt.params())
    assert all(p.data_ptr() != t.data_ptr() for p, t in zip(opt.params(), cloud.render_args()))
    with pytest.raises(RuntimeError, match="no gradient"):
        opt.step()
    visible = torch.from_numpy(C.mask(65, seed=3))
    exp = [{k: a.copy() for k, a in d.items()} for d in parts]
    for t in (1, 2, 3):
        for p, k in zip(opt.params(), C.FIELDS):
            p.grad = torch.from_numpy(parts[1][k].copy())
        versions = [p._version for p in opt.params()]
        opt.step(visible, zero_grads=(t == 2))
        assert all(p._version > v for p, v in zip(opt.params(), versions))             # the trap: every version advanced
        exp[0], _, exp[2], exp[3], _ = S.step(S.plan(t, C.LRS), exp[0], parts[1], exp[2], exp[3], visible=visible.numpy())
        assert (t == 2) == all(not S.words(p.grad.numpy()).any() for p in opt.params())
    assert opt.steps == 3 and int(opt.skipped) == 0
    assert off_words([list(opt.params()), opt.exp_avg, opt.exp_avg_sq], [exp[0], exp[2], exp[3]]) == 0
    snap = opt.cloud()
    assert not any(t.requires_grad for t in snap.render_args()) and snap.centers.data_ptr() != opt.params()[0].data_ptr()
    assert off_words([list(snap.render_args())], [exp[0]]) == 0
    state = opt.state()
    other = R.SurfelAdam(cloud, sparse=False)
    other.load_state(state)
    assert other.steps == 3 and other.sparse and other.lrs == opt.lrs
    for mine, theirs in ((other.params(), opt.params()), (other.exp_avg, opt.exp_avg), (other.exp_avg_sq, opt.exp_avg_sq)):
        assert all(torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)) for a, b in zip(mine, theirs))
    dense = R.SurfelAdam(cloud, sparse=False)                                          # sparse=False ignores the mask
    for p, k in zip(dense.params(), C.FIELDS):
        p.grad = torch.from_numpy(parts[1][k].copy())
    dense.step(torch.zeros(65, dtype=torch.uint8))
    assert all((S.words(p.detach().numpy()) != S.words(parts[0][k])).mean() > 0.9 for p, k in zip(dense.params(), C.FIELDS))
    opt.zero_grad()
    assert all(not S.words(p.grad.numpy()).any() for p in opt.params())


# ------------------------------------------------------------------------------------------------------------------ the binding, the build

def test_the_modules_binding_equals_the_headers_prototypes(hip_lib):
    """The header lies under include/ and its two functions are rows of ``_native.SIGNATURES`` (tests/test_abi_cpu.py holds the rows
    to the prototypes, kind by kind): the library exports both, the stream is on the device entry alone, the unit is built with
    -ffp-contract=off, and the header's plan and span are the module's."""
    from lara_amd import _native, splatrefine as R
    from tests.test_abi_cpu import header_functions_by_file
    names = ["lara_splatadam_step", "lara_splatadam_step_host"]
    assert sorted(header_functions_by_file()["lara_splatadam.h"]) == names
    assert set(names) <= set(_native._SIGS) and all(hasattr(hip_lib, n) for n in names)
    assert [_native._SIGS[n][2] for n in names] == [True, False]                       # the stream, on the device entry alone
    text = open(os.path.join(ROOT, "lara_amd", "csrc", "Makefile")).read()
    assert "FLAGS_splatadam := -ffp-contract=off\n" in text and " splatadam" in text.split("OBJS")[1].splitlines()[0]
    header = open(os.path.join(ROOT, "include", "lara_splatadam.h")).read()
    assert f"#define LARA_SPLATADAM_PLAN {R.PLAN}\n" in header and f"#define LARA_SPLATADAM_SPAN {R.SPAN}\n" in header


def test_nothing_on_the_default_routes_imports_the_module():
    code = "import sys, lara_amd, lara_amd.renderer, lara_amd.loss, lara_amd.splatio, lara_amd.splatxform; print('lara_amd.splatrefine' in sys.modules)"
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0 and run.stdout.strip() == "False", run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------------------------ the hostcheck

def test_the_stand_alone_host_program_ends_without_a_report():
    """csrc/splatadam_ops.h and the host entry's loop as a stand-alone program under AddressSanitizer and UBSan (nothing loaded
    into python, no device): 0 words off the restatement, exit code 0, no report."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "splatadam_hostcheck.py")], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "words off the restatement 0" in run.stdout and "another skipped count 0" in run.stdout and "sanitizer reports: none" in run.stdout, run.stdout
