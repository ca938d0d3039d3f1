"""`lara_amd.splatxform` restated in numpy float64, independently of the module: the rasteriser's SH basis from its constants, the
rotation blocks by a least-squares fit of their defining identity over seeded directions, the per-surfel arithmetic in the order
include/lara_splatxform.h writes, ``transform_points``, ``with_sh_degree`` and the camera rule.  numpy's elementwise float64
products and sums are single IEEE operations (nothing is contracted), so the restated words are the header's."""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                               # the unit roundoff of fp32

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)
QNAN = np.uint32(0x7FC00000)


def basis(d):
    """Y [..., 16] at the unit directions d [..., 3]: the 16 functions as csrc/preprocess.hip evaluates them (signs and order)."""
    d = np.asarray(d, F64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return np.stack([
        np.full_like(x, SH_C0),
        -SH_C1 * y, SH_C1 * z, -SH_C1 * x,
        SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy),
        SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
        SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
        SH_C3[6] * x * (xx - 3.0 * yy)], axis=-1)


def directions(n, seed):
    g = np.random.default_rng([seed, n])
    d = g.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def fit_blocks(R, degree=3, n=64, seed=7):
    """[D1, .., D_degree] with Y_l(R d) = D_l Y_l(d), fitted over n seeded directions."""
    d = directions(n, seed)
    Y0, Y1 = basis(d), basis(d @ np.asarray(R, F64).T)
    out = []
    for l in range(1, degree + 1):
        a, b = l * l, (l + 1) * (l + 1)
        Dt, *_ = np.linalg.lstsq(Y0[:, a:b], Y1[:, a:b], rcond=None)
        out.append(Dt.T)
    return out


def permutation_block(R):
    """D1 = P R P^T, P: (x, y, z) -> (-y, z, -x)."""
    P = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    return P @ np.asarray(R, F64) @ P.T


def rotation(angle_deg, axis):
    """Rodrigues' formula."""
    a = np.asarray(axis, F64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = np.deg2rad(angle_deg)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def similarity_matrix(angle_deg, axis, s=1.0, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3] = s * rotation(angle_deg, axis)
    T[:3, 3] = t
    return T


def axis_rotations():
    """The 24 proper rotations that permute the axes."""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in np.ndindex(2, 2, 2):
            M = np.zeros((3, 3))
            for i in range(3):
                M[i, perm[i]] = -1.0 if signs[i] else 1.0
            if np.linalg.det(M) > 0:
                out.append(M)
    assert len(out) == 24
    return out


def fl32(v):
    """The one rounding of the header: float64 -> fp32, a NaN as the word 0x7FC00000."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(v, F64).astype(F32)
    w = f.view(np.uint32).copy()
    w[np.isnan(f)] = QNAN
    return w.view(F32)


def transform_points(A, t, pts):
    """((A_i0 x + A_i1 y) + A_i2 z) + t_i, rounded once, NaN payloads as they fall (lara_meshalign_transform keeps them)."""
    p = np.asarray(pts, F32).astype(F64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((A[i, 0] * x + A[i, 1] * y) + A[i, 2] * z) + t[i] for i in range(3)], axis=1).astype(F32)


def apply(plan, c):
    """The cloud ``c`` (dict of fp32 arrays) under the 100 doubles ``plan``, in the header's order; returns a new dict."""
    plan = np.asarray(plan, F64)
    A, t, r, log_s = plan[0:9].reshape(3, 3), plan[9:12], plan[12:16], plan[16]
    D = {1: plan[17:26].reshape(3, 3), 2: plan[26:51].reshape(5, 5), 3: plan[51:100].reshape(7, 7)}
    out = {}
    with np.errstate(all="ignore"):
        p = c["centers"].astype(F64)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        out["centers"] = fl32(np.stack([((A[i, 0] * x + A[i, 1] * y) + A[i, 2] * z) + t[i] for i in range(3)], axis=1))
        q = c["rotations"].astype(F64)
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        out["rotations"] = fl32(np.stack([((r[0] * w - r[1] * x) - r[2] * y) - r[3] * z,
                                          ((r[0] * x + r[1] * w) + r[2] * z) - r[3] * y,
                                          ((r[0] * y - r[1] * z) + r[2] * w) + r[3] * x,
                                          ((r[0] * z + r[1] * y) - r[2] * x) + r[3] * w], axis=1))
        out["scales"] = fl32(c["scales"].astype(F64) + log_s)
        out["opacity"] = c["opacity"].copy()
        shs = c["shs"].copy()
        n = shs.shape[1]
        src = c["shs"].astype(F64)
        l = 1
        while (l + 1) ** 2 <= n:
            a, width = l * l, 2 * l + 1
            for i in range(width):
                acc = D[l][i, 0] * src[:, a, :]
                for j in range(1, width):
                    acc = acc + D[l][i, j] * src[:, a + j, :]
                shs[:, a + i, :] = fl32(acc)
            l += 1
        out["shs"] = shs
    return out


def with_sh_degree(c, degree):
    n = (degree + 1) ** 2
    words = np.zeros((c["shs"].shape[0], n, 3), np.uint32)
    k = min(n, c["shs"].shape[1])
    words[:, :k] = c["shs"].view(np.uint32)[:, :k]
    return dict(c, shs=words.view(F32))


def build_rotation(q):
    """R [P,3,3] of the quaternions q [P,4] (w, x, y, z), normalised first: csrc/preprocess.hip's quat_to_rotmat in float64."""
    q = np.asarray(q, F64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def colour(c, d):
    """(sum_m c_m Y_m(d) [P, D, 3], sum_m |c_m| |Y_m(d)| [P, D, 3]) of the cloud's coefficients (read as float64) along d [D, 3]."""
    n = c["shs"].shape[1]
    Y = basis(d)[:, :n]
    s = c["shs"].astype(F64)
    return np.einsum("pmc,dm->pdc", s, Y), np.einsum("pmc,dm->pdc", np.abs(s), np.abs(Y))


def split(T):
    """(R, s, t, A) of a similarity, R by the polar factor."""
    T = np.asarray(T, F64)
    A = T[:3, :3]
    s = np.linalg.det(A) ** (1.0 / 3.0)
    Uu, _, Vt = np.linalg.svd(A / s)
    return Uu @ Vt, s, T[:3, 3], A


def projection(znear, zfar, fovx, fovy):
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2] = 1.0 / np.tan(fovx / 2.0), 1.0 / np.tan(fovy / 2.0), 1.0
    P[2, 2], P[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)
    return P


def moved_camera(c2w, center, znear, zfar, fovx, fovy, T):
    """The camera rule: c2w' = [[R R_c, sR p + t], [0, 1]]; near and far times s; world_view = inverse(c2w')^T, full = that P^T;
    the centre moved as a point."""
    R, s, t, A = split(T)
    c2w = np.asarray(c2w, F64)
    new = np.eye(4)
    new[:3, :3] = R @ c2w[:3, :3]
    new[:3, 3] = A @ c2w[:3, 3] + t
    wvt = np.linalg.inv(new).T
    return {"c2w": new, "znear": znear * s, "zfar": zfar * s, "world_view_transform": wvt,
            "full_proj_transform": wvt @ projection(znear * s, zfar * s, fovx, fovy).T, "camera_center": A @ np.asarray(center, F64) + t}
