"""The cases tests/test_splatxform.py and tests/test_splatxform_gpu.py share: seeded clouds with special rows, the sizes, the row
offsets and the transforms.  The restated answers are computed once per case and kept."""
import numpy as np

from tests import splatio_cases
from tests import splatxform_restate as S

FIELDS = splatio_cases.FIELDS
DEGREES = (0, 1, 2, 3)
# the edges of a wave (64) and of the kernel's span of 256 rows (LARA_SPLATXFORM_SPAN: the issue's sizes as they stand), and 1 000
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
ROW_OFFSETS = (0, 1, 300)
SENTINEL = np.uint32(0xDEADBEEF)

# the three transforms of the issue's experiment
ROTATION = S.similarity_matrix(37.0, (1.0, 2.0, 3.0))
RIGID = S.similarity_matrix(37.0, (1.0, 2.0, 3.0), t=(0.3, -0.2, 0.1))
SIMILARITY = S.similarity_matrix(111.0, (-2.0, 1.0, 0.5), s=1.7, t=(0.3, -0.2, 0.1))
TRANSFORMS = {"rotation": ROTATION, "rigid": RIGID, "similarity": SIMILARITY}


def _word(x):
    return np.array([x], np.uint32).view(np.float32)[0]


NAN_A, NAN_B, SNAN = _word(0x7FC12345), _word(0x7FC00001), _word(0x7F800001)
INF, NEG_ZERO = np.float32(np.inf), np.float32(-0.0)
DEN_MIN, DEN_MAX, DEN_NEG = _word(0x00000001), _word(0x007FFFFF), _word(0x80000400)


def cloud(P, degree, seed=0, special=True):
    """P surfels with the decoder's statistics.  ``special`` rows, as far as P reaches: 0 a NaN centre coordinate; 1 an infinite
    centre coordinate and an infinite coefficient of the last band; 2 a zero quaternion; 3 -0.0 in every field; 4 denormals in
    every field; 5 NaNs with payloads in the opacity, band 0 (a signalling one) and a whole channel; 6 infinities of both signs in
    the quaternion and an infinite scale; the last row (P > 8) an all-infinite centre, whose sums are inf - inf."""
    c = splatio_cases.cloud(P, degree, seed=seed)
    if not special:
        return c
    n = (degree + 1) ** 2

    def put(row, field, index, value):
        if row < P:
            c[field][(row,) + index] = value
    put(0, "centers", (0,), NAN_A)
    put(1, "centers", (1,), INF)
    put(1, "shs", (n - 1, 2), -INF)
    for k in range(4):
        put(2, "rotations", (k,), np.float32(0.0))
    put(3, "centers", (2,), NEG_ZERO)
    put(3, "scales", (0,), NEG_ZERO)
    put(3, "rotations", (1,), NEG_ZERO)
    put(3, "shs", (0, 0), NEG_ZERO)
    put(3, "shs", (n - 1, 1), NEG_ZERO)
    put(4, "centers", (0,), DEN_MIN)
    put(4, "scales", (1,), DEN_MIN)
    put(4, "rotations", (3,), DEN_NEG)
    put(4, "shs", (n - 1, 1), DEN_MAX)
    put(4, "opacity", (0,), DEN_NEG)
    put(5, "opacity", (0,), NAN_B)
    put(5, "shs", (0, 1), SNAN)
    for k in range(n):
        put(5, "shs", (k, 0), NAN_A if k % 2 else NAN_B)
    put(6, "rotations", (0,), INF)
    put(6, "rotations", (2,), -INF)
    put(6, "scales", (0,), INF)
    if P > 8:
        for k in range(3):
            put(P - 1, "centers", (k,), INF if k != 1 else -INF)
    return c


_kept = {}


def restated(P, degree, name, plan):
    """``S.apply(plan, cloud(P, degree))``, computed once per (P, degree, transform name)."""
    key = (P, degree, name)
    if key not in _kept:
        _kept[key] = S.apply(plan, cloud(P, degree, seed=P + degree))
    return _kept[key]
