"""`lara_amd.splatxform` without a GPU, through ``lara_splatxform_apply_host`` (the per-surfel function of csrc/splatxform_ops.h
compiled for the CPU), held to the float64 restatement (tests/splatxform_restate.py): the plan's layout and refusals; the SH
blocks against their defining identity, orthogonality, the group law and the restated fit; the host entry's words against the
restated arithmetic for every SH degree, size, row offset and in place, special rows included; equivariance of the colour (with
its tooth) and of the geometry in float64 of the fp32 outputs; the identity, the round trip, ``place``, ``with_sh_degree``, the
camera rule, ``align_to``'s refusal; the entry points' own refusals; the stand-alone sanitizer program."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lara_amd import splatio, splatxform as X
from tests import splatxform_cases as C
from tests import splatxform_restate as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = S.U


def _cloud(c, device="cpu"):
    return splatio.SurfelCloud(*(torch.from_numpy(c[k].copy()).to(device) for k in C.FIELDS))


def _words(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _same_words(cloud, c, what=""):
    for k, t in zip(C.FIELDS, cloud.render_args()):
        got, want = _words(t), np.ascontiguousarray(c[k]).view(np.uint32)
        assert got.shape == want.shape, (what, k)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, k, len(bad), bad[:4].tolist())


def _seeded_rotations(n=16):
    g = np.random.default_rng(11)
    return [S.rotation(g.uniform(0, 180), g.normal(size=3)) for _ in range(n)]


ROTATIONS = ([("seeded", R) for R in _seeded_rotations()] + [("axis", R) for R in S.axis_rotations()]
             + [("turn", S.rotation(180.0, a)) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 2, 3), (-2, 1, 0.5))])


# ------------------------------------------------------------------------------------------------------------------ the plan

def test_the_plan_lays_out_the_similarity():
    T = C.SIMILARITY
    plan = X.similarity(T)
    R, s, t, A = S.split(T)
    assert plan.shape == (100,) and plan.dtype == np.float64
    assert np.array_equal(plan[0:9], A.ravel()) and np.array_equal(plan[9:12], t)
    q = plan[12:16]
    assert abs(q @ q - 1.0) < 1e-15 and q[0] >= 0.0
    assert np.abs(S.build_rotation(q[None])[0] - R).max() < 1e-15
    assert abs(plan[16] - np.log(1.7)) < 1e-15
    for block, fit in zip((plan[17:26].reshape(3, 3), plan[26:51].reshape(5, 5), plan[51:100].reshape(7, 7)), S.fit_blocks(R)):
        assert np.abs(block - fit).max() < 1e-12
    eye = X.similarity(np.eye(4))
    assert eye[16] == 0.0 and not np.signbit(eye[16]) and np.array_equal(eye[12:16], [1.0, 0.0, 0.0, 0.0])
    assert X.similarity(torch.from_numpy(T)).tobytes() == plan.tobytes()
    # w == 0: the first non-zero of x, y, z is positive
    for M in (np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])):
        T = np.eye(4)
        T[:3, :3] = M          # exact half turns
        q = X.similarity(T)[12:16]
        assert q[0] == 0.0 and not np.signbit(q).any() and next(v for v in q[1:] if v != 0.0) > 0.0


def test_the_plan_refuses_what_is_no_similarity():
    shear = np.eye(4)
    shear[0, 1] = 0.01
    stretched = np.diag([1.0, 1.0, 1.01, 1.0])
    mirror = np.diag([1.0, 1.0, -1.0, 1.0])
    nan = np.eye(4)
    nan[1, 3] = np.nan
    row = np.eye(4)
    row[3, 0] = 1e-3
    for name, T in (("shear", shear), ("scale", stretched), ("reflection", mirror), ("nan", nan), ("last row", row)):
        with pytest.raises(ValueError, match="lara_amd.splatxform"):
            X.similarity(T)
    with pytest.raises(ValueError):
        X.similarity(np.eye(3))
    X.similarity(np.diag([2.0, 2.0, 2.0, 1.0]))          # one scale is a similarity
    c = _cloud(C.cloud(5, 1))
    for T in (shear, mirror, nan):
        with pytest.raises(ValueError):
            X.transform(c, T)


# ------------------------------------------------------------------------------------------------------------------ sh_rotation

def test_sh_rotation_of_the_identity_is_the_exact_identity():
    for l, D in enumerate(X.sh_rotation(np.eye(3)), 1):
        assert D.shape == (2 * l + 1, 2 * l + 1) and D.tobytes() == np.eye(2 * l + 1).tobytes()
    assert [b.shape for b in X.sh_rotation(np.eye(3), 2)] == [(3, 3), (5, 5)] and X.sh_rotation(np.eye(3), 0) == []


@pytest.mark.parametrize("kind,R", ROTATIONS, ids=[f"{k}{i}" for i, (k, _) in enumerate(ROTATIONS)])
def test_sh_rotation_meets_its_definition(kind, R):
    D = X.sh_rotation(R)
    d = S.directions(2000, 3)
    Y0, Y1 = S.basis(d), S.basis(d @ R.T)
    g = np.random.default_rng(5)
    assert np.array_equal(D[0], S.permutation_block(R))                              # D1 = P R P^T, as bits
    for l, (Dl, fit) in enumerate(zip(D, S.fit_blocks(R)), 1):
        a, b = l * l, (l + 1) ** 2
        c = g.normal(size=(8, b - a))
        lhs = np.einsum("km,dm->kd", c @ Dl.T, Y1[:, a:b])                           # sum_m (D c)_m Y_m(R d)
        rhs = np.einsum("km,dm->kd", c, Y0[:, a:b])
        bound = 1e-13 * np.einsum("km,dm->kd", np.abs(c), np.abs(Y0[:, a:b]))
        assert (np.abs(lhs - rhs) <= bound).all(), l          # (a band's sum of Y_m^2 is constant: the bound never vanishes)
        assert np.abs(Dl @ Dl.T - np.eye(b - a)).max() < 1e-13, l
        assert np.abs(Dl - fit).max() < 1e-12, l
    R2 = S.rotation(71.0, (0.3, -1.0, 0.2))
    for Dab, Da, Db in zip(X.sh_rotation(R @ R2), D, X.sh_rotation(R2)):
        assert np.abs(Dab - Da @ Db).max() < 1e-13


# ------------------------------------------------------------------------------------------------------------------ the host entry

@pytest.mark.parametrize("degree", C.DEGREES)
def test_the_host_entry_equals_the_restated_arithmetic(hip_lib, degree):
    """Every size, every row offset (into a larger output whose other rows keep a sentinel) and in place; the restated
    arithmetic is fed the module's own plan, which the sh_rotation and plan tests hold separately."""
    plan = X.similarity(C.SIMILARITY)
    for P in C.SIZES:
        c = C.cloud(P, degree, seed=P + degree)
        want = C.restated(P, degree, "similarity", plan)
        _same_words(X.transform(_cloud(c), C.SIMILARITY), want, f"P={P}")
        _same_words(X.transform(_cloud(c), plan), want, f"planned once, P={P}")
        inplace = _cloud(c)
        assert X.transform(inplace, C.SIMILARITY, out=inplace) is inplace
        _same_words(inplace, want, f"in place, P={P}")
        other = _cloud(C.cloud(P, degree, seed=99))
        X.transform(_cloud(c), C.SIMILARITY, out=other)
        _same_words(other, want, f"out, P={P}")
        for row0 in C.ROW_OFFSETS:
            rows = row0 + P + 7
            n = (degree + 1) ** 2
            outs = [torch.from_numpy(np.full((rows,) + shape, C.SENTINEL, np.uint32).view(np.float32))
                    for shape in ((3,), (n, 3), (1,), (2,), (4,))]
            X._apply(plan, _cloud(c), outs, row0, rows)
            for k, t in zip(C.FIELDS, outs):
                w = _words(t)
                assert np.array_equal(w[row0:row0 + P], want[k].view(np.uint32)), (P, row0, k)
                assert (w[:row0] == C.SENTINEL).all() and (w[row0 + P:] == C.SENTINEL).all(), (P, row0, k)


def test_special_rows_are_in_the_cases_and_propagate(hip_lib):
    c = C.cloud(257, 3, seed=260)
    out = X.transform(_cloud(c), C.SIMILARITY)
    assert np.isnan(c["centers"][0, 0]) and _words(out.centers)[0].tolist() == [0x7FC00000] * 3      # a NaN is the canonical word
    assert np.isinf(out.centers[1].numpy()).any() and np.isinf(out.shs[1, 9:].numpy()).any()
    assert not out.rotations[2].numpy().any()                                                        # a zero quaternion stays zero
    assert _words(out.opacity)[5, 0] == 0x7FC00001 and _words(out.shs)[5, 0, 1] == 0x7F800001       # copied words keep their payload
    assert np.isnan(out.shs[5, 1:, 0].numpy()).all() and not np.isfinite(out.rotations[6].numpy()).any()
    assert np.isposinf(out.scales[6, 0].item()) and np.isnan(out.centers[256].numpy()).any()          # inf - inf


def test_partial_overlap_and_mismatched_outputs_are_refused(hip_lib):
    c = _cloud(C.cloud(64, 1))
    with pytest.raises(ValueError, match="surfels"):
        X.transform(c, C.RIGID, out=_cloud(C.cloud(65, 1)))
    with pytest.raises(ValueError, match="degree"):
        X.transform(c, C.RIGID, out=_cloud(C.cloud(64, 2)))
    base = torch.zeros(66, 3)
    shifted = splatio.SurfelCloud(base[1:65], c.shs.clone(), c.opacity.clone(), c.scales.clone(), c.rotations.clone())
    inside = splatio.SurfelCloud(base[0:64], c.shs, c.opacity, c.scales, c.rotations)
    with pytest.raises(ValueError, match="overlaps"):
        X.transform(inside, C.RIGID, out=shifted)
    # an output that lies in another field of the input
    crossed = splatio.SurfelCloud(torch.zeros(64, 3), torch.zeros(64, 4, 3), torch.zeros(64, 1), c.shs.view(-1)[:128].view(64, 2),
                                  torch.zeros(64, 4))
    with pytest.raises(ValueError, match="overlaps"):
        X.transform(c, C.RIGID, out=crossed)
    strided = splatio.SurfelCloud(torch.zeros(64, 6)[:, :3], torch.zeros(64, 4, 3), torch.zeros(64, 1), torch.zeros(64, 2), torch.zeros(64, 4))
    with pytest.raises(ValueError, match="contiguous"):
        X.transform(c, C.RIGID, out=strided)


def test_the_modules_binding_equals_the_headers_prototypes(hip_lib):
    """The header lies under include/ and its two functions are rows of ``_native.SIGNATURES`` (tests/test_abi_cpu.py holds the rows
    to the prototypes, kind by kind): the library exports both, the stream is on the device entry alone, the unit is built with
    -ffp-contract=off, and the header's plan and span are the module's."""
    from lara_amd import _native
    from tests.test_abi_cpu import header_functions_by_file
    names = ["lara_splatxform_apply", "lara_splatxform_apply_host"]
    assert sorted(header_functions_by_file()["lara_splatxform.h"]) == names
    assert set(names) <= set(_native._SIGS) and all(hasattr(hip_lib, n) for n in names)
    assert [_native._SIGS[n][2] for n in names] == [True, False]                              # the stream, on the device entry alone
    text = open(os.path.join(ROOT, "lara_amd", "csrc", "Makefile")).read()
    assert "FLAGS_splatxform := -ffp-contract=off\n" in text and " splatxform " in text.split("OBJS")[1].splitlines()[0]
    header = open(os.path.join(ROOT, "include", "lara_splatxform.h")).read()
    assert f"#define LARA_SPLATXFORM_PLAN {X.PLAN}\n" in header and f"#define LARA_SPLATXFORM_SPAN {X.SPAN}\n" in header


def test_the_entry_points_refuse_bad_arguments(hip_lib):
    plan = (ctypes.c_double * 100)(*X.similarity(C.RIGID))
    c = C.cloud(4, 1)
    bufs = [np.ascontiguousarray(c[k]) for k in C.FIELDS] + [np.zeros_like(c[k]) for k in C.FIELDS]
    ptrs = [b.ctypes.data for b in bufs]
    host, dev = hip_lib.lara_splatxform_apply_host, hip_lib.lara_splatxform_apply
    assert host(plan, 1, 4, *ptrs, 0, 4) == 0
    for fn, tail in ((host, ()), (dev, (None,))):          # (the device entry refuses before it touches a device)
        assert fn(None, 1, 4, *ptrs, 0, 4, *tail) == -1
        for k in range(10):
            assert fn(plan, 1, 4, *(ptrs[:k] + [None] + ptrs[k + 1:]), 0, 4, *tail) == -1, k
        for degree in (-1, 4):
            assert fn(plan, degree, 4, *ptrs, 0, 4, *tail) == -1
        assert fn(plan, 1, -1, *ptrs, 0, 4, *tail) == -1
        assert fn(plan, 1, 4, *ptrs, 1, 4, *tail) == -1 and fn(plan, 1, 4, *ptrs, -1, 4, *tail) == -1
        assert fn(plan, 1, 4, *ptrs, 2 ** 62, 2 ** 62 + 3, *tail) == -1
        assert fn(plan, 1, 0, *ptrs, 4, 4, *tail) == 0          # P = 0: nothing to do, nothing launched
    assert hip_lib.lara2dgs_error_string(-1) == b"invalid argument"


# ------------------------------------------------------------------------------------------------------------------ equivariance

@pytest.mark.parametrize("degree", C.DEGREES)
def test_the_colour_turns_with_the_cloud_and_not_without_the_blocks(hip_lib, degree):
    c = C.cloud(257, degree, seed=21, special=False)
    R, _, _, _ = S.split(C.SIMILARITY)
    d = S.directions(50, 9)
    base, mag = S.colour(c, d)
    moved = X.transform(_cloud(c), C.SIMILARITY)
    got, _ = S.colour({"shs": moved.shs.numpy()}, d @ R.T)
    assert (np.abs(got - base) <= 8 * U * mag).all()
    # the tooth: the same plan with identity blocks leaves the coefficients unrotated
    plan = X.similarity(C.SIMILARITY)
    plan[17:26], plan[26:51], plan[51:100] = np.eye(3).ravel(), np.eye(5).ravel(), np.eye(7).ravel()
    outs = X._empty_like_rows(_cloud(c), 257)
    X._apply(plan, _cloud(c), outs, 0, 257)
    flat, _ = S.colour({"shs": outs[1].numpy()}, d @ R.T)
    miss = np.abs(flat - base).max()
    if degree == 0:
        assert miss == 0.0
    else:
        assert miss > 0.1 * mag.max(), (miss, mag.max())


@pytest.mark.parametrize("name", sorted(C.TRANSFORMS))
def test_the_tangent_frame_turns_and_scales_with_the_cloud(hip_lib, name):
    T = C.TRANSFORMS[name]
    c = C.cloud(257, 1, seed=22, special=False)
    moved = X.transform(_cloud(c), T)
    R, s, _, A = S.split(T)
    want = A @ (S.build_rotation(c["rotations"]) * np.exp(c["scales"].astype(np.float64))[:, None, [0, 1, 1]])[:, :, :2]
    got = (S.build_rotation(moved.rotations.numpy()) * np.exp(moved.scales.numpy().astype(np.float64))[:, None, [0, 1, 1]])[:, :, :2]
    err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)          # per tangent axis, relative
    print(f"{name}: tangent axes off by {err.max() / U:.2f} u at most")
    assert (err <= 8 * U).all(), err.max() / U
    # |q'| = |q|: the norm of the unnormalised quaternion is carried through
    n0, n1 = np.linalg.norm(c["rotations"].astype(np.float64), axis=1), np.linalg.norm(moved.rotations.numpy().astype(np.float64), axis=1)
    assert (np.abs(n1 - n0) <= 2 * U * n0).all()


# ------------------------------------------------------------------------------------------------------------------ identities

@pytest.mark.parametrize("degree", C.DEGREES)
def test_identity_round_trip_and_centres(hip_lib, degree):
    c = C.cloud(257, degree, seed=23, special=False)
    same = X.transform(_cloud(c), np.eye(4))
    for k, t in zip(C.FIELDS, same.render_args()):
        assert (t.numpy() == c[k]).all(), k
    for name, T in C.TRANSFORMS.items():
        R, s, t, A = S.split(T)
        there = X.transform(_cloud(c), T)
        assert np.array_equal(_words(there.centers), S.transform_points(A, t, c["centers"]).view(np.uint32)), name
        Ti = np.linalg.inv(T)
        back = X.transform(there, Ti)
        Ai, ti = Ti[:3, :3], Ti[:3, 3]
        # a centre's magnitude terms: what the forward sum adds up, carried through the inverse sum, and the inverse's own
        m1 = np.abs(c["centers"].astype(np.float64)) @ np.abs(A).T + np.abs(t)
        m2 = m1 @ np.abs(Ai).T + np.abs(ti)
        assert (np.abs(back.centers.numpy().astype(np.float64) - c["centers"]) <= 4 * U * m2).all(), name
        for l in range(1, degree + 1):
            a, b = l * l, (l + 1) ** 2
            norm = np.linalg.norm(c["shs"][:, a:b].astype(np.float64), axis=1, keepdims=True)
            assert (np.abs(back.shs.numpy()[:, a:b].astype(np.float64) - c["shs"][:, a:b]) <= 4 * U * norm).all(), (name, l)
        qn = np.linalg.norm(c["rotations"].astype(np.float64), axis=1, keepdims=True)
        assert (np.abs(back.rotations.numpy().astype(np.float64) - c["rotations"]) <= 4 * U * qn).all(), name
        assert (np.abs(back.scales.numpy().astype(np.float64) - c["scales"])
                <= 4 * U * (np.abs(c["scales"].astype(np.float64)) + abs(np.log(s)))).all(), name
        assert np.array_equal(_words(back.opacity), c["opacity"].view(np.uint32))
        assert np.array_equal(_words(back.shs)[:, 0], c["shs"].view(np.uint32)[:, 0])


# ------------------------------------------------------------------------------------------------------------------ the helpers

def test_place_equals_the_concatenated_transforms(hip_lib):
    parts = [C.cloud(P, 2, seed=30 + P) for P in (257, 0, 1, 300)]
    Ts = [C.ROTATION, C.RIGID, np.eye(4), C.SIMILARITY]
    clouds = [_cloud(p) for p in parts]
    got = X.place(clouds, Ts)
    want = splatio.concatenate([X.transform(c, T) for c, T in zip(clouds, Ts)])
    assert got.n_surfels == 558 and got.sh_degree == 2
    for a, b in zip(got.render_args(), want.render_args()):
        assert np.array_equal(_words(a), _words(b))
    with pytest.raises(ValueError, match="SH degrees"):
        X.place([clouds[0], _cloud(C.cloud(4, 1))], Ts[:2])
    with pytest.raises(ValueError):
        X.place(clouds, Ts[:3])
    with pytest.raises(ValueError):
        X.place([], [])
    mixed = X.place([clouds[0], X.with_sh_degree(_cloud(C.cloud(4, 1)), 2)], Ts[:2])
    assert mixed.n_surfels == 261 and mixed.sh_degree == 2


@pytest.mark.parametrize("old", C.DEGREES)
@pytest.mark.parametrize("new", C.DEGREES)
def test_with_sh_degree_copies_words(old, new):
    c = C.cloud(65, old, seed=40)
    got = X.with_sh_degree(_cloud(c), new)
    assert got.sh_degree == new
    _same_words(got, S.with_sh_degree(c, new))
    if new > old:
        assert (_words(got.shs)[:, (old + 1) ** 2:] == 0).all()          # +0.0
    with pytest.raises(ValueError):
        X.with_sh_degree(_cloud(c), 4)


def test_cameras_move_with_the_cloud():
    from lara_amd import cameras
    c2w = cameras.turntable_c2w(3, elevation_deg=20.0)
    cams = cameras.make_cameras(c2w, 64, 48, 0.75, 0.6, 0.5, 2.5)
    for name, T in C.TRANSFORMS.items():
        R, s, t, A = S.split(T)
        new = X.transform_cameras(cams, T)
        poses = X.transform_c2w(c2w, T)
        assert poses.dtype == torch.float64 and poses.shape == (3, 4, 4)
        for i, (cam, old) in enumerate(zip(new, cams)):
            pose = np.linalg.inv(old.world_view_transform.double().numpy().T)          # the pose the camera itself holds
            want = S.moved_camera(pose, old.camera_center.numpy(), 0.5, 2.5, 0.75, 0.6, T)
            assert (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy) == (64, 48, 0.75, 0.6)
            assert abs(cam.znear - want["znear"]) <= 4 * U * want["znear"] and abs(cam.zfar - want["zfar"]) <= 4 * U * want["zfar"]
            for key in ("world_view_transform", "full_proj_transform", "camera_center"):
                got, ref = getattr(cam, key).double().numpy(), want[key]
                assert getattr(cam, key).dtype == torch.float32
                assert (np.abs(got - ref) <= 4 * U * np.abs(ref).max()).all(), (name, i, key)
            # moved as a point: NOT the sic rebuilt from the new pose (they differ by 2 t and more)
            rebuilt = -want["c2w"][:3, 3]
            if name != "rotation":
                assert np.abs(cam.camera_center.double().numpy() - rebuilt).max() > 0.1
            ref_pose = S.moved_camera(c2w[i].double().numpy(), old.camera_center.numpy(), 0.5, 2.5, 0.75, 0.6, T)["c2w"]
            assert np.abs(poses[i].numpy() - ref_pose).max() <= 1e-15 * 4
            assert np.array_equal(poses[i].numpy()[3], [0.0, 0.0, 0.0, 1.0])


def test_align_to_refuses_cpu_tensors_as_meshalign_does():
    from lara_amd import meshalign
    c = _cloud(C.cloud(300, 1, seed=50, special=False))
    target = torch.from_numpy(C.cloud(200, 0, seed=51, special=False)["centers"])
    kept, _ = splatio.select(c, min_opacity=0.005)
    with pytest.raises(Exception) as theirs:
        meshalign.icp(kept.centers, target, max_dist=0.3, estimation="point")
    with pytest.raises(type(theirs.value)) as ours:
        X.align_to(c, target, max_dist=0.3, estimation="point")
    assert str(ours.value) == str(theirs.value)


def test_nothing_on_the_default_routes_imports_the_module():
    code = ("import sys, lara_amd, lara_amd.pipeline, lara_amd.renderer, lara_amd.rasterizer, lara_amd.splatio, lara_amd.evaluate;"
            "assert 'lara_amd.splatxform' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------------------------------------------------------ the hostcheck

def test_the_stand_alone_host_program_ends_without_a_report(tmp_path):
    """csrc/splatxform_ops.h and the host entry's loop as a stand-alone program under AddressSanitizer and UBSan (nothing loaded
    into python, no device): 0 words off the restatement, exit code 0, no report."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "splatxform_hostcheck.py")], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "words off the restatement 0" in run.stdout and "sanitizer reports: none" in run.stdout, run.stdout
