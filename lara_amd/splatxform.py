"""Moving and composing predicted surfel clouds (include/lara_splatxform.h, csrc/splatxform.hip): a similarity T = [[sR, t], [0, 1]]
applied to a ``splatio.SurfelCloud`` -- centres, log scales, the quaternion, and the SH coefficients of bands 1..3 rotated in the
rasteriser's own basis (csrc/preprocess.hip: the 3DGS constants and signs), so that the moved cloud seen from cameras moved with it
renders as the original did.  Opt-in like every module here, imported by nothing on the default routes; ``splatio`` is untouched.

  * ``similarity``        the plan of a 4x4: 100 doubles (A, t, the unit quaternion of R, log s, the SH blocks D1, D2, D3);
  * ``sh_rotation``       the blocks: Y_l(R d) = D_l Y_l(d) in the rasteriser's basis, in closed form, float64 on the host;
  * ``transform``         one kernel launch, no host read; ``out`` may be another cloud or the cloud itself (in place);
  * ``place``             several clouds, each under its transform, into ONE allocation: one launch per cloud at its row offset;
  * ``with_sh_degree``    bands truncated or padded with +0.0 (words copied), so that clouds of different degrees can be placed;
  * ``transform_c2w``, ``transform_cameras``  the cameras that go with a moved cloud;
  * ``align_to``          ``meshalign.icp`` on the cloud's visible centres, then ``transform``.

How the blocks are built.  Band l of the basis is Y_m = C_m p_m with p_m a homogeneous harmonic polynomial of degree l with integer
coefficients (the expressions of preprocess.hip) and C_m the constant in front of it.  Under the inner product of homogeneous
polynomials in which the monomials are orthogonal and <x^a y^b z^c, x^a y^b z^c> = a! b! c! (Fischer's; it is invariant under
rotations, so the p_m of a band are orthogonal in it), D_ij = (C_i / C_j) <p_i o R, p_j> / <p_j, p_j>, where p_i o R is p_i with
the rows of R put in for x, y, z and multiplied out.  For R = I every product and sum is one of small integers: the blocks are the
exact identity.  D1 = P R P^T with P: (x, y, z) -> (-y, z, -x), as bits.

Tensors on the GPU go through the kernel.  Tensors on the host go through ``lara_splatxform_apply_host``, the same per-surfel
function compiled for the CPU (csrc/splatxform_ops.h): the reference the kernel is held to bit for bit, not a fast path.

Out of scope: reflections and non-uniform scale (refused), gradients through the transform, SH bands above 3.  ``rend_dist`` of a
render is NOT invariant under a scale s != 1: the rasteriser's distortion term rests on its absolute near and far constants.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import splatio
from . import _native
from ._native import host_array

PLAN = 100                               # include/lara_splatxform.h
SPAN = 256
_WHO = "lara_amd.splatxform"
_ORTHO_TOL = 1e-6

# ---------------------------------------------------------------------------------------------------------- the SH blocks

_X, _Y, _Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
       -0.5900435899266435)
# band l: (C_m, p_m as {(a, b, c): integer coefficient of x^a y^b z^c}) in the rasteriser's order
_BANDS = {
    1: ((-_C1, {_Y: 1}), (_C1, {_Z: 1}), (-_C1, {_X: 1})),
    2: ((_C2[0], {(1, 1, 0): 1}), (_C2[1], {(0, 1, 1): 1}), (_C2[2], {(0, 0, 2): 2, (2, 0, 0): -1, (0, 2, 0): -1}),
        (_C2[3], {(1, 0, 1): 1}), (_C2[4], {(2, 0, 0): 1, (0, 2, 0): -1})),
    3: ((_C3[0], {(2, 1, 0): 3, (0, 3, 0): -1}), (_C3[1], {(1, 1, 1): 1}), (_C3[2], {(0, 1, 2): 4, (2, 1, 0): -1, (0, 3, 0): -1}),
        (_C3[3], {(0, 0, 3): 2, (2, 0, 1): -3, (0, 2, 1): -3}), (_C3[4], {(1, 0, 2): 4, (3, 0, 0): -1, (1, 2, 0): -1}),
        (_C3[5], {(2, 0, 1): 1, (0, 2, 1): -1}), (_C3[6], {(3, 0, 0): 1, (1, 2, 0): -3})),
}


def _times(p, q):
    out = {}
    for (a, b, c), u in p.items():
        for (d, e, f), v in q.items():
            k = (a + d, b + e, c + f)
            out[k] = out.get(k, 0.0) + u * v
    return out


def _rotated(poly, rows):
    """``poly`` with the linear forms ``rows`` (x, y, z of R d, as polynomials in d) put in and multiplied out."""
    out = {}
    for (a, b, c), coef in poly.items():
        term = {(0, 0, 0): float(coef)}
        for form, power in zip(rows, (a, b, c)):
            for _ in range(power):
                term = _times(term, form)
        for k, v in term.items():
            out[k] = out.get(k, 0.0) + v
    return out


def _fischer(p, q):
    return sum(v * q[k] * (math.factorial(k[0]) * math.factorial(k[1]) * math.factorial(k[2])) for k, v in p.items() if k in q)


def sh_rotation(R, degree=3):
    """The blocks [D1, .., D_degree] (float64, (2l+1) x (2l+1)) of the rotation ``R`` in the rasteriser's SH basis:
    sum_m (D_l c)_m Y_m(R d) = sum_m c_m Y_m(d) for every unit d, i.e. Y_l(R d) = D_l Y_l(d).  Orthogonal for an orthogonal R; the
    exact identity for R = I."""
    R = np.asarray(R, np.float64)
    if R.shape != (3, 3) or int(degree) not in (0, 1, 2, 3):
        raise ValueError(f"{_WHO}: sh_rotation takes a 3x3 rotation and a degree 0..3")
    rows = [{_X: float(R[i, 0]), _Y: float(R[i, 1]), _Z: float(R[i, 2])} for i in range(3)]
    blocks = []
    for l in range(1, int(degree) + 1):
        band = _BANDS[l]
        moved = [_rotated(p, rows) for _, p in band]
        D = np.empty((2 * l + 1, 2 * l + 1))
        for j, (cj, pj) in enumerate(band):
            nj = float(_fischer(pj, pj))
            for i, (ci, _) in enumerate(band):
                D[i, j] = (ci / cj) * (_fischer(moved[i], pj) / nj)
        blocks.append(D + 0.0)               # (-0.0 -> +0.0)
    return blocks


# ---------------------------------------------------------------------------------------------------------- the plan

def _quaternion(R):
    """The unit quaternion (w, x, y, z) of a rotation, by the largest-component branch; w >= 0, and for w == 0 the first non-zero of
    x, y, z positive."""
    t = (R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2])
    k = int(np.argmax(t))
    if k == 0:
        w = 0.5 * math.sqrt(1.0 + t[0])
        q = [w, (R[2, 1] - R[1, 2]) / (4.0 * w), (R[0, 2] - R[2, 0]) / (4.0 * w), (R[1, 0] - R[0, 1]) / (4.0 * w)]
    else:
        i = k - 1
        j, m = (i + 1) % 3, (i + 2) % 3
        u = 0.5 * math.sqrt(1.0 + R[i, i] - R[j, j] - R[m, m])
        q = [0.0, 0.0, 0.0, 0.0]
        q[0] = (R[m, j] - R[j, m]) / (4.0 * u)
        q[1 + i], q[1 + j], q[1 + m] = u, (R[j, i] + R[i, j]) / (4.0 * u), (R[m, i] + R[i, m]) / (4.0 * u)
    q = np.array(q, np.float64)
    q = q / math.sqrt(float(q @ q))
    lead = next((v for v in q if v != 0.0), 1.0)
    return (-q if lead < 0.0 else q) + 0.0


def similarity(T):
    """The plan of the 4x4 similarity ``T`` = [[sR, t], [0, 1]] as 100 float64 (numpy): [0:9] A = T's 3x3 block row-major, [9:12] t,
    [12:16] the unit quaternion of R (w, x, y, z as ``build_rotation`` reads it), [16] log s (exactly 0.0 for s == 1.0), [17:26],
    [26:51], [51:100] the SH blocks D1, D2, D3 row-major.  s = det(A)^(1/3) as ``meshalign`` takes it; R = A / s made orthonormal by
    its polar factor.  ValueError: a non-finite entry, a last row other than (0, 0, 0, 1), det <= 0 (a reflection),
    max |A^T A / s^2 - I| > 1e-6 (shear or non-uniform scale)."""
    T = np.array(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{_WHO}: a transformation is a 4x4 matrix")
    if not np.isfinite(T).all():
        raise ValueError(f"{_WHO}: a transformation needs finite entries")
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"{_WHO}: a transformation's last row is (0, 0, 0, 1), got {T[3].tolist()}")
    A = T[:3, :3]
    det = float(np.linalg.det(A))
    if not det > 0.0:
        raise ValueError(f"{_WHO}: a transformation needs a 3x3 block of positive determinant (a reflection cannot be applied), got {det:g}")
    s = det ** (1.0 / 3.0)
    off = float(np.abs(A.T @ A / (s * s) - np.eye(3)).max())
    if not off <= _ORTHO_TOL:
        raise ValueError(f"{_WHO}: the 3x3 block is no rotation times one scale (shear or non-uniform scale): "
                         f"max |A^T A / s^2 - I| = {off:.3g} > {_ORTHO_TOL:g}")
    U, _, Vt = np.linalg.svd(A / s)
    R = U @ Vt
    plan = np.empty(PLAN, np.float64)
    plan[0:9], plan[9:12], plan[12:16] = A.ravel(), T[:3, 3], _quaternion(R)
    plan[16] = 0.0 if s == 1.0 else math.log(s)
    D1, D2, D3 = sh_rotation(R, 3)
    plan[17:26], plan[26:51], plan[51:100] = D1.ravel(), D2.ravel(), D3.ravel()
    return plan


def _plan_of(T):
    """``T`` as a plan: a 4x4 goes through ``similarity``; the 100 doubles ``similarity`` returned are taken as they are, so that a
    transform applied many times is planned once."""
    if isinstance(T, np.ndarray) and T.shape == (PLAN,) and T.dtype == np.float64:
        return T
    return similarity(T)


def _rotation_scale(T):
    """(R, s, t, 4x4) of ``T`` as the plan takes them."""
    plan = similarity(T)
    A = plan[0:9].reshape(3, 3)
    s = float(np.linalg.det(A)) ** (1.0 / 3.0)
    U, _, Vt = np.linalg.svd(A / s)
    return U @ Vt, s, plan[9:12].copy(), A


# ---------------------------------------------------------------------------------------------------------- clouds

def _extent(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _check_overlap(ins, outs):
    """An output may be its own input (same address: in place); every other overlap of an output with an input is refused."""
    for i, a in enumerate(ins):
        a0, a1 = _extent(a)
        for j, b in enumerate(outs):
            b0, b1 = _extent(b)
            if a0 < b1 and b0 < a1 and not (i == j and a0 == b0):
                raise ValueError(f"{_WHO}: out.{splatio.SurfelCloud.FIELDS[j]} overlaps {splatio.SurfelCloud.FIELDS[i]} of the input "
                                 "partly; out is another cloud or the cloud itself")


def _apply(plan, cloud, outs, row0, out_rows):
    """One launch (one host loop for host tensors): ``cloud`` under ``plan`` into rows [row0, row0 + P) of ``outs``."""
    ins = [t.contiguous() for t in cloud.render_args()]
    for name, a, b in zip(splatio.SurfelCloud.FIELDS, ins, outs):          # the kernel writes rows [row0, row0 + P) of out_rows: hold it to that
        if (tuple(b.shape) != (int(out_rows),) + tuple(a.shape[1:]) or b.dtype != torch.float32 or b.device != a.device
                or not b.is_contiguous() or not 0 <= int(row0) <= int(out_rows) - cloud.n_surfels):
            raise ValueError(f"{_WHO}: the output for {name} must be a contiguous fp32 [{int(out_rows)}, ...] tensor on {a.device} "
                             f"with room for rows {int(row0)}..{int(row0) + cloud.n_surfels}, got {tuple(b.shape)} {b.dtype} on {b.device}")
    _check_overlap(ins, outs)
    if cloud.n_surfels == 0:                 # (an empty tensor has no address to hand over; the entry points launch nothing for P = 0)
        return
    _native.call_on("lara_splatxform_apply", cloud.device, host_array("d", [float(v) for v in plan]), cloud.sh_degree, cloud.n_surfels,
                    *ins, *outs, int(row0), int(out_rows))


def _empty_like_rows(cloud, rows):
    n = cloud.shs.shape[1]
    return [torch.empty(rows, *shape, dtype=torch.float32, device=cloud.device) for shape in ((3,), (n, 3), (1,), (2,), (4,))]


@torch.no_grad()
def transform(cloud, T, *, out=None):
    """``cloud`` moved by the 4x4 similarity ``T``: a new ``SurfelCloud``, or ``out`` -- a cloud of the same size, SH degree and
    device with contiguous tensors, which may be ``cloud`` itself (in place).  One kernel launch, no host read; the plan travels in
    the kernel's arguments.  ``T`` may be the plan ``similarity`` returned."""
    plan = _plan_of(T)
    if out is None:
        outs = _empty_like_rows(cloud, cloud.n_surfels)
    else:
        if (out.n_surfels, out.sh_degree, out.device) != (cloud.n_surfels, cloud.sh_degree, cloud.device):
            raise ValueError(f"{_WHO}: out has {out.n_surfels} surfels of SH degree {out.sh_degree} on {out.device}, the cloud "
                             f"{cloud.n_surfels} of degree {cloud.sh_degree} on {cloud.device}")
        outs = list(out.render_args())
        if not all(t.is_contiguous() for t in outs):
            raise ValueError(f"{_WHO}: the tensors of out must be contiguous")
    _apply(plan, cloud, outs, 0, cloud.n_surfels)
    return out if out is not None else splatio.SurfelCloud(*outs)


@torch.no_grad()
def place(clouds, transforms):
    """ONE cloud of ``clouds[k]`` moved by ``transforms[k]``, rows in the order given: one allocation of the whole, one launch per
    cloud at its row offset.  The bits of ``splatio.concatenate([transform(c, T) ...])``.  The clouds share a device and an SH
    degree (``with_sh_degree`` makes them).  A transform may be a 4x4 or a plan."""
    clouds, transforms = list(clouds), list(transforms)
    if not clouds or len(clouds) != len(transforms):
        raise ValueError(f"{_WHO}: place takes as many transforms as clouds, and at least one")
    if len({c.sh_degree for c in clouds}) != 1:
        raise ValueError(f"{_WHO}: the clouds have SH degrees {[c.sh_degree for c in clouds]}; they must share one (with_sh_degree)")
    if len({c.device for c in clouds}) != 1:
        raise ValueError(f"{_WHO}: the clouds lie on {sorted({str(c.device) for c in clouds})}; they must share one device")
    plans = [_plan_of(T) for T in transforms]
    total = sum(c.n_surfels for c in clouds)
    outs = _empty_like_rows(clouds[0], total)
    row0 = 0
    for c, plan in zip(clouds, plans):
        _apply(plan, c, outs, row0, total)
        row0 += c.n_surfels
    return splatio.SurfelCloud(*outs)


@torch.no_grad()
def with_sh_degree(cloud, degree):
    """``cloud`` at SH degree ``degree``: the bands above it dropped, or the missing ones filled with +0.0.  Words are copied."""
    d = int(degree)
    if d not in (0, 1, 2, 3):
        raise ValueError(f"{_WHO}: SH degree 0..3, got {degree!r}")
    n_old, n_new = cloud.shs.shape[1], (d + 1) ** 2
    words = torch.zeros(cloud.n_surfels, n_new, 3, dtype=torch.int32, device=cloud.device)
    k = min(n_old, n_new)
    words[:, :k] = cloud.shs.contiguous().view(torch.int32)[:, :k]
    return splatio.SurfelCloud(cloud.centers, words.view(torch.float32), cloud.opacity, cloud.scales, cloud.rotations)


# ---------------------------------------------------------------------------------------------------------- cameras

def transform_c2w(c2w, T):
    """The camera-to-world matrices ``c2w`` [..., 4, 4] of cameras moved with a cloud by ``T``: [[R R_c, sR p + t], [0, 1]] -- the
    axes turn, the position moves as a point, the scale stays out of the axes.  float64 (a tensor on ``c2w``'s device)."""
    R, _, t, A = _rotation_scale(T)
    src = torch.as_tensor(c2w)
    c = src.detach().cpu().double().numpy()
    if c.shape[-2:] != (4, 4):
        raise ValueError(f"{_WHO}: c2w is [..., 4, 4]")
    out = np.zeros_like(c)
    out[..., :3, :3] = R @ c[..., :3, :3]
    out[..., :3, 3] = c[..., :3, 3] @ A.T + t
    out[..., 3, 3] = 1.0
    return torch.from_numpy(out).to(src.device)


def _c2w_of(cam):
    c2w = getattr(cam, "view_world_transform", None)
    if c2w is None:
        c2w = torch.linalg.inv(cam.world_view_transform.detach().double().T)
    return torch.as_tensor(c2w).detach().double().cpu()


def transform_cameras(cams, T):
    """New ``cameras.Camera``s that see the cloud moved by ``T`` as ``cams`` saw the original: the pose by ``transform_c2w``,
    znear and zfar times s, ``world_view_transform`` and ``full_proj_transform`` rebuilt from the new pose in float64 and rounded
    once, and ``camera_center' = sR camera_center + t`` -- moved as a point, NOT rebuilt from the new pose: ``make_cameras`` keeps
    the reference's ``camera_center = -c2w[:3, 3]`` (sic), the SH direction is normalize(mean - camera_center), and only the moved
    point keeps that direction turning with R.  A camera that carries ``view_world_transform`` (its c2w, the rays' pose) gets the
    new one."""
    from . import cameras as _cameras
    _, s, t, A = _rotation_scale(T)
    out = []
    for cam in cams:
        dev = cam.world_view_transform.device
        c2w = transform_c2w(_c2w_of(cam), T)
        wvt = torch.linalg.inv(c2w).T.contiguous()
        znear, zfar = float(cam.znear) * s, float(cam.zfar) * s
        PT = _cameras.projection_matrix(znear, zfar, float(cam.FoVx), float(cam.FoVy), dtype=torch.float64).T.contiguous()
        center = cam.camera_center.detach().double().cpu().numpy() @ A.T + t
        center = torch.nn.functional.pad(torch.from_numpy(center).float(), (0, 1)).to(dev)[:3]      # (a 16-byte row, as make_cameras)
        new = _cameras.Camera(int(cam.image_width), int(cam.image_height), float(cam.FoVx), float(cam.FoVy), znear, zfar,
                              wvt.float().to(dev), PT.float().to(dev), (wvt @ PT).float().contiguous().to(dev), center)
        if getattr(cam, "view_world_transform", None) is not None:
            new.view_world_transform = c2w.float().to(dev)
        out.append(new)
    return out


# ---------------------------------------------------------------------------------------------------------- alignment

@torch.no_grad()
def align_to(cloud, target, *, min_opacity=0.005, **icp_kwargs):
    """``cloud`` taken into ``target``'s frame: ``meshalign.icp`` with the centres of the rows ``splatio.select(min_opacity=...)``
    keeps as the source point set (``target`` and ``icp_kwargs`` as there; ``max_dist`` is required), then ``transform`` by the
    registration's 4x4.  Returns (the moved cloud, the registration dict)."""
    from . import meshalign
    kept, _ = splatio.select(cloud, min_opacity=min_opacity)
    result = meshalign.icp(kept.centers, target, **icp_kwargs)
    return transform(cloud, result["transformation"]), result
