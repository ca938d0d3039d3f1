"""The inputs of tests/test_meshio.py and tests/test_meshio_gpu.py: fp32 bit patterns at every edge of "%.9g", mesh sizes around the
256-line workgroup, the widest and the narrowest lines, indices on every digit-count crossing, colours on the edges of the uchar rule.
All numpy, seeded; nothing here needs a device."""
import functools

import numpy as np

# (Nv, T): one thread, one line short of a workgroup, a full one, one line into the next, several with a ragged last one
SIZES = [(0, 0), (1, 0), (0, 1), (3, 1), (255, 254), (256, 256), (257, 300), (1000, 2100)]
MAX_INDEX = 2 ** 31 - 2
# rounding carries into the next power of ten (the first two round up onto it, the others down onto it)
CARRY_CASES = (0x19416d9a, 0x56b5e621, 0x0da24260, 0x0f4ad2f8, 0x10fd87b6, 0x26901d7d)
LONGEST = np.float32(-7.77995488e+32)          # a token of 15 characters
N_TIES = 1200


def bits_of(x):
    return np.asarray(x, np.float32).view(np.uint32)


def ties():
    """Bit patterns of exact ties at the tenth digit: (8 I + f) / 8 with a 7-digit I (< 2^21, so the value is an fp32) and odd f."""
    rng = np.random.default_rng(20240)
    whole = rng.integers(1000000, 2 ** 21, N_TIES)
    eighths = 2 * rng.integers(0, 4, N_TIES) + 1
    v = (whole * 8 + eighths).astype(np.float64) / 8.0
    f = v.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), v)
    return bits_of(f)


@functools.lru_cache(None)
def _float_specials():
    s = [0x00000000, 0x80000000,                       # +-0
         0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff,      # the smallest and the largest denormal, FLT_MIN, FLT_MAX
         0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff]      # +-inf, NaNs of both signs
    s += [int(b) for b in bits_of(np.ldexp(1.0, np.arange(-149, 128)).astype(np.float32))]      # every power of two
    for k in range(-45, 39):                           # the nearest float to 10^k and two neighbours on either side
        b = int(bits_of(np.float32(float("1e%d" % k))))
        s += [b + d for d in (-2, -1, 0, 1, 2) if 0 < b + d < 0x7f800000]
    # both sides of the notation switches: 1e-4 and 1e9 (999999936 is the largest float below it)
    s += [int(bits_of(np.float32(1e-4))) + d for d in (-1, 0, 1)]
    s += [int(bits_of(np.float32(999999936.0))), int(bits_of(np.float32(1e9)))]
    s += [int(b) for b in ties()]
    s += [int(bits_of(LONGEST)), int(bits_of(np.float32(-0.000123456789))), int(bits_of(np.float32(123456.789)))]
    out = np.array(s, np.uint32)
    return np.concatenate([out, out[12:] | np.uint32(0x80000000)])      # and the negatives of the finite ones


def float_specials():
    """fp32 bit patterns (uint32) at the edges of the formatting routine."""
    return _float_specials().copy()


def specials_mesh():
    """(vertices, triangles, colors): as many vertices as there are special values; column j holds them rotated by 7 j places, so
    every one of them lands in every position of a line."""
    s = float_specials().view(np.float32)
    cols = [np.roll(s, 7 * j) for j in range(6)]
    n = len(s)
    t = np.stack([np.arange(n), np.roll(np.arange(n), 1), np.roll(np.arange(n), 2)], axis=1)[: n - 5].astype(np.int64)
    return np.stack(cols[:3], axis=1), t, np.stack(cols[3:], axis=1)


def mesh(nv, nt, seed=0):
    """(vertices, triangles int64, colors, normals) of the sizes asked for: coordinates of mixed magnitudes and signs, indices of
    mixed digit counts (not bounded by nv: the writers do not compare them)."""
    rng = np.random.default_rng(1000 * nv + nt + seed)
    v = (rng.standard_normal((nv, 3)) * 10.0 ** rng.integers(-6, 7, (nv, 3))).astype(np.float32)
    c = rng.random((nv, 3)).astype(np.float32)
    n = rng.standard_normal((nv, 3)).astype(np.float32)
    t = (rng.integers(0, 10, (nt, 3)) ** rng.integers(1, 9, (nt, 3))).astype(np.int64) if nt else np.zeros((0, 3), np.int64)
    t = np.minimum(t, MAX_INDEX)
    return v, t, c, n


def widest():
    """256 vertex lines of 98 bytes and 256 face lines of 35 bytes: a workgroup's LDS span exactly full."""
    v = np.full((256, 3), LONGEST, np.float32)
    t = np.full((256, 3), MAX_INDEX, np.int64)
    return v, t, v.copy()


def narrowest():
    """`v 0 0 0` and `f 1 1 1`."""
    return np.zeros((300, 3), np.float32), np.zeros((300, 3), np.int64), None


def index_crossings():
    """0-based indices whose 1-based text sits on both sides of every digit-count change, and the largest index."""
    vals = [10 ** k + d for k in range(1, 10) for d in (-2, -1, 0)] + [MAX_INDEX, 0]
    return np.array(vals, np.int64)


def crossing_mesh():
    vals = index_crossings()
    t = np.stack([vals, np.roll(vals, 1), np.roll(vals, 2)], axis=1)
    return np.linspace(-1, 1, 12, dtype=np.float32).reshape(4, 3), t, None


def color_edges():
    """Colours [n, 3] around every edge of the uchar rule."""
    c = [-1.0, -0.0, 0.0, 1.0, 2.0, np.nan, -np.nan, np.inf, -np.inf, 1e-8, 0.5, np.nextafter(np.float32(1), np.float32(0))]
    for k in (0, 1, 2, 63, 126, 127, 128, 200, 253, 254):
        mid = np.float32((k + 0.5) / 255.0)
        c += [np.nextafter(mid, np.float32(-1)), mid, np.nextafter(mid, np.float32(2))]
    c = np.array(c, np.float32)
    c = np.concatenate([c, c[: (-len(c)) % 3]])
    return np.stack([c, np.roll(c, 1), np.roll(c, 2)], axis=1)
