"""The cases tests/test_splatdensify.py, tests/test_splatdensify_gpu.py and tools/splatdensify_hostcheck.py share: seeded clouds with
moments, statistics that make every action occur, the plan rows of every kind of round, the rows that sit exactly on a limit, the
noise of the split children, and the render calls of the accumulation."""
import math

import numpy as np

from tests import splatrefine_cases

FIELDS = splatrefine_cases.FIELDS
DEGREES = (0, 1, 3)
CHILDREN = (2, 3)
# the edges of a wave, 1 000, 1 025 (3 P crosses a 1 024-element workgroup of the scan) and 100 003 (3 P passes 256 workgroups of the
# scan: the second level's second lap)
SIZES = (0, 1, 63, 64, 65, 1000, 1025)
LARGE = 100003
VIEWS = (1, 4, 8)
SENTINEL = np.uint32(0xDEADBEEF)
THRESHOLD = 0.5                              # a power of two: avg = 1.5 / 3 meets it exactly
LOG_DENSE = -5.0                             # the median of the clouds' log scales, and an fp32: a scale can sit exactly on it
KINDS = ("keep", "prune", "clone", "split", "mix", "mix_screen", "no_clone", "no_split", "no_prune")
N_EDGES = 12


def _word(x):
    return np.array([x], np.uint32).view(np.float32)[0]


def plan_row(kind, n_split):
    """The 8 doubles of a round of ``kind``, written out here (not through the module): [0] threshold, [1] log_dense, [2] the opacity
    logit below which a surfel goes, [3] the screen limit, [4] log_max_world, [5] log(0.8 N), [6] N, [7] the flags."""
    row = np.array([THRESHOLD, LOG_DENSE, -3.5, 0.0, -4.4, math.log(0.8 * n_split), float(n_split), 7.0], np.float64)
    if kind == "keep":
        row[0], row[2] = 2.0, -math.inf
    elif kind == "prune":
        row[2] = math.inf
    elif kind == "clone":
        row[0], row[1], row[2] = 0.0, 50.0, -math.inf
    elif kind == "split":
        row[0], row[1], row[2] = 0.0, -50.0, -math.inf
    elif kind == "mix_screen":
        row[3] = 20.0
    elif kind == "no_clone":
        row[7] = 6.0
    elif kind == "no_split":
        row[7] = 5.0
    elif kind == "no_prune":
        row[7] = 3.0
    return row


def round_case(P, degree, n_split, kind, seed=0):
    """One round: {"params", "exp_avg", "exp_avg_sq"} (dicts of float32 arrays), the three statistic rows, the plan row, the noise
    [P, N, 2].  The kinds other than the four pure ones carry, from 63 surfels on, ``N_EDGES`` rows that sit on a limit (``edges``)."""
    params, _, m, v = splatrefine_cases.case(P, degree, moments=True, seed=seed, special=False)
    g = np.random.default_rng([seed, P, degree, n_split, 555])
    seen = g.integers(0, 6, P).astype(np.int32)
    grad_sum = (g.uniform(0, 1, P) * np.maximum(seen, 1)).astype(np.float32)
    max_radius = g.integers(0, 41, P).astype(np.int32)
    noise = g.normal(0, 1, (P, n_split, 2)).astype(np.float32)
    if kind in ("clone", "split"):
        seen = np.maximum(seen, 1)
    if kind == "mix_screen" and P:
        params["scales"][g.random(P) < 0.05] += np.float32(1.5)                   # some larger than log_max_world
    if kind not in ("keep", "prune", "clone", "split") and P >= 63:
        edges(params, grad_sum, seen, max_radius)
    return {"params": params, "exp_avg": m, "exp_avg_sq": v, "grad_sum": grad_sum, "seen": seen, "max_radius": max_radius,
            "plan": plan_row(kind, n_split), "noise": noise, "degree": degree, "P": P, "kind": kind}


def edges(params, grad_sum, seen, max_radius):
    """Rows 0 .. 11 put on the limits.  With every flag on and the screen limit off: 0 avg exactly at the threshold and small: clone;
    1 the same, smax exactly at log_dense: clone; 2 just above log_dense: split; 3 seen = 0 with a large grad_sum: keep; 4 a NaN
    grad_sum: keep; 5 an infinite grad_sum: hot; 6 .. 9 NaN / inf in opacity or a scale: prune; 10 opacity exactly at the logit
    limit: stays; 11 just below it: prune."""
    op, sc = params["opacity"], params["scales"]
    op[:N_EDGES, 0] = 0.0
    sc[:N_EDGES] = (-6.0, -7.0)
    grad_sum[:N_EDGES], seen[:N_EDGES], max_radius[:N_EDGES] = 0.0, 1, 3
    grad_sum[0], seen[0] = 1.5, 3
    grad_sum[1], seen[1], sc[1] = 1.5, 3, (LOG_DENSE, -6.0)
    grad_sum[2], seen[2], sc[2] = 1.5, 3, (-6.0, np.nextafter(np.float32(LOG_DENSE), np.float32(0)))
    grad_sum[3], seen[3] = 100.0, 0
    grad_sum[4], seen[4] = np.nan, 2
    grad_sum[5], seen[5] = np.inf, 2
    op[6, 0] = _word(0x7FC12345)
    op[7, 0] = np.inf
    sc[8] = (_word(0xFFC00ABC), -6.0)
    sc[9] = (-6.0, -np.inf)
    op[10, 0] = np.float32(-3.5)
    op[11, 0] = np.nextafter(np.float32(-3.5), np.float32(-10))


def round_cases():
    """(P, degree, N, kind) of every round the tests run: every size with the mix at every degree and N, every kind at 1 000 and at
    65, the empty cloud and the single surfel under every pure kind, and the large one once."""
    out = [(P, d, n, "mix") for P in SIZES for d in DEGREES for n in CHILDREN]
    out += [(P, 1, n, kind) for P in (65, 1000) for n in CHILDREN for kind in KINDS if kind != "mix"]
    out += [(P, 0, 2, kind) for P in (0, 1) for kind in ("keep", "prune", "clone", "split")]
    out += [(1025, 3, 3, "mix_screen"), (LARGE, 1, 2, "mix")]
    return out


def accumulate_case(P, V, seed=0):
    """One render call on incoming statistics: grad_means2D [P,3] with non-finite words in some rows, radii [V,P] with zeros and
    negative words (a surfel no view saw has no positive one), and the three rows as earlier calls left them."""
    g = np.random.default_rng([seed, P, V, 777])
    grad = (g.normal(0, 1, (P, 3)) * 10.0 ** g.uniform(-6, -1, (P, 3))).astype(np.float32)
    flat = grad.reshape(-1).view(np.uint32)
    special = np.array([0x7FC12345, 0x7F800000, 0xFF800000, 0xFFC00ABC, 0x7F800001, 0x80000000, 0x00000001, 0x7F7FFFFF], np.uint32)
    if P:
        at = g.choice(3 * P, min(3 * P, 3 * special.size), replace=False)
        flat[at] = np.resize(special, at.size)
    radii = g.integers(-3, 31, (V, P)).astype(np.int32)
    radii[g.random((V, P)) < 0.5] = 0
    unseen = g.random(P) < 0.25                                                   # a quarter of the surfels: no positive radius
    radii[:, unseen] = np.minimum(radii[:, unseen], 0)
    grad_sum = g.uniform(0, 3, P).astype(np.float32)
    seen = g.integers(0, 9, P).astype(np.int32)
    max_radius = g.integers(0, 25, P).astype(np.int32)
    return grad, radii, grad_sum, seen, max_radius


def accumulate_cases():
    return [(P, V) for P in SIZES + (LARGE,) for V in VIEWS if P != LARGE or V == 4]
