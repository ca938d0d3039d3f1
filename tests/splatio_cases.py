"""Seeded surfel clouds for tests/test_splatio.py and tests/test_splatio_gpu.py, as dicts of float32 numpy arrays in the layout
``Renderer.render_img`` takes (pre-activation)."""
import numpy as np

# two quiet NaNs with different payloads, a signalling NaN, a negative NaN, the infinities, -0.0, +0.0, the smallest and the
# largest denormal and a negative one
SPECIAL_WORDS = np.array([0x7FC00001, 0x7FC12345, 0x7F800001, 0xFFC00ABC, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                          0x00000001, 0x007FFFFF, 0x80000400], np.uint32)
FIELDS = ("centers", "shs", "opacity", "scales", "rotations")


def cloud(P, degree, seed=0, special=False):
    """P surfels of SH degree ``degree`` with the decoder's statistics.  ``special``: every field gets all of SPECIAL_WORDS
    (as many as it has room for), spread over its rows and columns."""
    n = (degree + 1) ** 2
    g = np.random.default_rng([seed, P, degree])
    c = {"centers": g.uniform(-0.5, 0.5, (P, 3)), "shs": g.normal(0, 0.5, (P, n, 3)), "opacity": g.normal(-2.2, 1.0, (P, 1)),
         "scales": g.normal(-5.0, 0.3, (P, 2)), "rotations": g.normal(0, 1, (P, 4))}
    c = {k: np.ascontiguousarray(v, np.float32) for k, v in c.items()}
    if special:
        for k in FIELDS:
            flat = c[k].reshape(-1).view(np.uint32)
            m = min(flat.size, SPECIAL_WORDS.size)
            at = np.linspace(0, flat.size - 1, m).astype(np.int64)      # (distinct: the spacing is at least 1)
            flat[at] = SPECIAL_WORDS[:m]
    return c


def numbered(P, degree):
    """shs[p, k, c] = 100 p + 10 k + c, everything else from ``cloud``: each word of the file says where it came from."""
    c = cloud(P, degree, seed=3)
    n = (degree + 1) ** 2
    p, k, ch = np.meshgrid(np.arange(P), np.arange(n), np.arange(3), indexing="ij")
    c["shs"] = (100 * p + 10 * k + ch).astype(np.float32)
    return c
