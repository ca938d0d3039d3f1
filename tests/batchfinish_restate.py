"""The arithmetic of include/lara_batchfinish.h restated in numpy float32, independent of the C code: every operation is one numpy
float32 operation on float32 arrays (numpy rounds each once and contracts nothing), in the order the header writes.  The division is
numpy's own correctly rounded float32 division, not the header's reciprocal-and-correction form.  Shared by tests/test_batchfinish.py,
tests/test_batchfinish_gpu.py and tools/batchfinish_hostcheck.py."""
import numpy as np

F = np.float32
U = 2.0 ** -24


def unit(u8):
    """(float)u8 / 255.0f"""
    return np.asarray(u8, np.uint8).astype(F) / F(255.0)


def colour(rgba, bg):
    """rgba uint8 [B,V,H,W,4], bg float32 [B,V,3] -> (rgb float32 [B,V,H,W,3], msk uint8 [B,V,H,W])."""
    rgba = np.asarray(rgba, np.uint8)
    f = unit(rgba)
    a = f[..., 3:4]
    back = np.asarray(bg, F)[:, :, None, None, :] * (F(1.0) - a)
    front = f[..., :3] * a
    rgb = front + back
    assert rgb.dtype == F
    return rgb, (rgba[..., 3] > 0).astype(np.uint8)


def decode(n_u8):
    """n = (float)u8 / 255.0f * 2.0f - 1.0f"""
    return unit(n_u8) * F(2.0) - F(1.0)


def normals(n_u8, rot):
    """n_u8 uint8 [B,V,H,W,3], rot float32 [B,3,3] -> float32 [B,H,V*W,3]: nrm_j = (n_0 R[j][0] + n_1 R[j][1]) + n_2 R[j][2], pixel
    (b, v, h, w) at [b, h, v*W + w]."""
    n = decode(n_u8)
    B, V, H, W, _ = n.shape
    R = np.asarray(rot, F)[:, None, None, None]                      # [B,1,1,1,3,3]
    out = np.empty((B, V, H, W, 3), F)
    for j in range(3):
        p0, p1, p2 = n[..., 0] * R[..., j, 0], n[..., 1] * R[..., j, 1], n[..., 2] * R[..., j, 2]
        out[..., j] = (p0 + p1) + p2
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3, 4)).reshape(B, H, V * W, 3)


def normal_bound(n_u8, rot):
    """8 u sum_k |n_k R[j][k]| per output word, in the layout of `normals`: the issue's bound on the distance between two fp32
    evaluations of the 3-term sum in different orders (each is within gamma_3 of the exact sum of the rounded products)."""
    n = np.abs(decode(n_u8).astype(np.float64))
    B, V, H, W, _ = n.shape
    R = np.abs(np.asarray(rot, np.float64))
    mag = np.einsum("bvhwk,bjk->bvhwj", n, R)
    return 8.0 * U * np.ascontiguousarray(mag.transpose(0, 2, 1, 3, 4)).reshape(B, H, V * W, 3)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a
