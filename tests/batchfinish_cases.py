"""The raw batches tests/test_batchfinish_gpu.py and tools/batchfinish_hostcheck.py share: seeded uint8 images and normals in which
every code 0..255 occurs in every channel (from 256 pixels on), backgrounds of the loader's three colours and one seeded, and a
seeded finite 3x3 per scene that is no rotation."""
import numpy as np

# (B, V, H, W): one pixel; a short quad; H W and W odd; two scenes of odd views; whole quads in short rows; W a multiple of 4 with
# H W not one of 16; one long row span -- then a flat pixel count on either side of one workgroup's span of 4 x 256, and shapes whose
# colour half may go wide while the normals may not (H W % 4 == 0, W % 4 != 0), over more than one workgroup
SHAPES = ((1, 1, 1, 1), (1, 1, 1, 3), (1, 3, 2, 5), (2, 2, 5, 7), (1, 8, 4, 4), (2, 4, 3, 8), (1, 1, 16, 64),
          (1, 1, 1, 1023), (1, 1, 1, 1024), (1, 1, 1, 1025), (1, 1, 33, 31), (1, 1, 32, 32), (1, 1, 41, 25),
          (1, 2, 2, 6), (2, 3, 10, 18), (3, 2, 36, 20))


def batch(shape, seed=0):
    """{'rgba', 'bg', 'n_u8', 'rot'} of one shape."""
    B, V, H, W = shape
    g = np.random.default_rng(1000 + seed)
    rgba = g.integers(0, 256, (B, V, H, W, 4), dtype=np.uint8)
    n_u8 = g.integers(0, 256, (B, V, H, W, 3), dtype=np.uint8)
    n = B * V * H * W
    codes = (np.arange(n, dtype=np.int64) % 256).astype(np.uint8).reshape(B, V, H, W)
    for c in range(4):
        rgba[..., c] = np.where(g.random((B, V, H, W)) < 0.5, np.roll(codes.ravel(), 37 * c).reshape(codes.shape), rgba[..., c])
    for c in range(3):
        n_u8[..., c] = np.where(g.random((B, V, H, W)) < 0.5, np.roll(codes.ravel(), 11 * c + 5).reshape(codes.shape), n_u8[..., c])
    flat = rgba.reshape(-1, 4)                                        # (a view: rgba is contiguous)
    flat[::5, 3] = 0                                                  # clear and opaque pixels in every shape that has room
    flat[2::7, 3] = 255
    bg = g.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(B, V, 1)).repeat(3, axis=2)
    bg[-1, -1] = g.random(3, dtype=np.float32)
    rot = g.normal(size=(B, 3, 3)).astype(np.float32)
    return {"rgba": rgba, "bg": np.ascontiguousarray(bg, np.float32), "n_u8": n_u8, "rot": rot}
