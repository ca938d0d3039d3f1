"""The cases tests/test_splatrefine.py, tests/test_splatrefine_gpu.py and tools/splatadam_hostcheck.py share: seeded clouds with
gradients that carry every special word, zero and non-zero incoming moments, the sizes, the steps and a seeded visibility mask."""
import itertools

import numpy as np

from tests import splatio_cases

FIELDS = splatio_cases.FIELDS
DEGREES = (0, 1, 3)
# the edges of a wave (64: the ballot), one word up to several workgroups per field, and 1 000
SIZES = (0, 1, 63, 64, 65, 1000)
STEPS = (1, 10 ** 6)                         # t = 10^6: both bias corrections are 1 to the last bit
LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3)
SENTINEL = np.uint32(0xDEADBEEF)


def _word(x):
    return np.array([x], np.uint32).view(np.float32)[0]


# +-0.0, the smallest, the largest and a negative denormal, 1e+-30 of both signs, the infinities, a quiet NaN with a payload, a
# signalling NaN, a negative NaN
SPECIAL = np.array([0.0, _word(0x80000000), _word(0x00000001), _word(0x007FFFFF), _word(0x80000400), 1e30, -1e30, 1e-30, -1e-30,
                    np.inf, -np.inf, _word(0x7FC12345), _word(0x7F800001), _word(0xFFC00ABC)], np.float32)
N_NONFINITE = 5


def special_slots(size):
    """Where the special words go in a field of ``size`` words, and which: distinct places, the non-finite ones first so that the
    smallest fields (opacity of one surfel) still meet one."""
    m = min(size, SPECIAL.size)
    order = np.concatenate([np.arange(SPECIAL.size - N_NONFINITE, SPECIAL.size), np.arange(SPECIAL.size - N_NONFINITE)])[:m]
    return np.linspace(0, size - 1, m).astype(np.int64), SPECIAL[order]


def case(P, degree, moments, seed=0, special=True):
    """(params, grads, exp_avg, exp_avg_sq): four dicts of float32 arrays in a cloud's shapes.  ``moments``: incoming moments with
    the sizes a run leaves behind, or zeros.  ``special``: every field's gradient carries SPECIAL, as far as it has room."""
    params = splatio_cases.cloud(P, degree, seed=seed)
    g = np.random.default_rng([seed, P, degree, 77])
    grads, m, v = {}, {}, {}
    for k in FIELDS:
        shape = params[k].shape
        grads[k] = (g.normal(0, 1, shape) * 10.0 ** g.uniform(-6, -1, shape)).astype(np.float32)
        if moments:
            m[k] = (g.normal(0, 1, shape) * 1e-3).astype(np.float32)
            v[k] = (g.uniform(0, 1, shape) ** 2 * 1e-5).astype(np.float32)
        else:
            m[k], v[k] = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        if special:
            at, what = special_slots(grads[k].size)
            grads[k].reshape(-1).view(np.uint32)[at] = what.view(np.uint32)
    return params, grads, m, v


def mask(P, seed=0):
    """A seeded visibility mask, about half of the rows; bytes other than 1 count as seen too."""
    g = np.random.default_rng([seed, P, 99])
    vis = (g.random(P) < 0.5).astype(np.uint8)
    vis[vis != 0] = g.choice(np.array([1, 2, 255], np.uint8), int((vis != 0).sum()))
    return vis


def all_cases():
    """(P, degree, step, incoming moments?, sparse?) of every case."""
    return list(itertools.product(SIZES, DEGREES, STEPS, (False, True), (False, True)))


def copies(parts):
    return [{k: a.copy() for k, a in d.items()} for d in parts]
