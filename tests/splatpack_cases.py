"""The cases tests/test_splatpack.py, tests/test_splatpack_gpu.py and tools/splatpack_hostcheck.py share: seeded clouds built like
``splatxform_cases.cloud`` with the rows the formats' edges need, and the float64 restatement's answers, computed once per case and
kept."""
import numpy as np

from tests import splatpack_restate as S
from tests import splatxform_cases

FIELDS = S.FIELDS
THICKNESS = 1e-3
# the edges of a chunk of 256 rows, a partial chunk, an empty cloud, and 1 000
SIZES = (0, 1, 255, 256, 257, 1000)
DEGREES = (0, 1, 3)
SENTINEL = 0xA5
ROW_OFFSETS = (1, 3)


def cloud(P, degree, kind="mixed", seed=0):
    """``mixed``: ``splatxform_cases.cloud`` with its special rows -- 0, 1, 2, 5, 6 and the last (P > 8) hold NaNs, infinities or a zero
    quaternion and are dropped; 3 (-0.0) and 4 (denormals, the opacity aside) are kept -- and, as far as P reaches: 7 log scales beyond +-20; 8 a
    quaternion with two equal largest components; 9 one whose largest component is negative; 10 an f_dc that takes k outside [0, 1];
    11 two largest components equal in size and opposite in sign; 12 an opacity whose alpha rounds to 0 and 13 one whose alpha
    rounds to 255.  ``plain``: no special row.  ``coincident``: every centre the same point (max == min in every chunk).
    ``all_invalid``: a NaN in every row."""
    c = splatxform_cases.cloud(P, degree, seed=seed, special=kind == "mixed")

    def put(row, field, values):
        if row < P and not (P > 8 and row == P - 1):              # (the last row of a mixed cloud stays all-infinite)
            c[field][row] = np.asarray(values, np.float32).reshape(c[field][row].shape)
    if kind == "mixed":
        put(4, "opacity", (-1.5,))               # (a denormal logit is alpha = 1/2 exactly, 128.0 before the floor: ON a rounding boundary)
        put(7, "scales", (25.0, -30.0))
        put(8, "rotations", (0.5, 0.5, 0.1, 0.2))
        put(9, "rotations", (0.1, -0.9, 0.2, 0.1))
        if P > 11:
            c["shs"][10, 0, :] = (3.0, -3.0, 2.5)
        put(11, "rotations", (-0.5, 0.5, 0.25, 0.0))
        put(12, "opacity", (-30.0,))
        put(13, "opacity", (40.0,))
    elif kind == "coincident":
        c["centers"][:] = np.float32([0.25, -0.125, 0.0625])
    elif kind == "all_invalid":
        c["opacity"][0::2, 0] = np.float32(np.nan)
        c["scales"][1::2, 1] = np.float32(np.inf)
    return c


def cases():
    """(P, degree, kind) of every case."""
    out = [(P, d, "mixed") for P in SIZES for d in DEGREES]
    out += [(1, 1, "plain"), (256, 3, "plain"), (257, 1, "coincident"), (600, 3, "coincident"), (300, 1, "all_invalid")]
    return out


_kept = {}


def case(P, degree, kind):
    """The case's cloud and the restatement's answers, computed once: a dict with ``cloud``, ``plan``, ``valid``, ``box``,
    ``dropped``, ``morton_keys``, ``order`` (Morton), ``chunks``, ``words``, ``sh``, ``decoded`` (float64, before rounding),
    ``importance_keys``, ``splat_order``, ``splat`` ([P_out,8] uint32), ``splat_decoded``, ``alpha_pre``, ``importance_pre``."""
    key = (P, degree, kind)
    if key not in _kept:
        c = cloud(P, degree, kind, seed=P + degree)
        pl = S.plan(THICKNESS)
        valid, box, dropped = S.bounds(c)
        mk = S.morton_keys(c, valid, box)
        order = S.order_of(mk, dropped)
        chunks, words, sh = S.encode(c, order, pl)
        ik = S.importance_keys(c, valid, pl)
        so = S.order_of(ik, dropped)
        splat = S.splat_encode(c, so, pl)
        _kept[key] = dict(cloud=c, plan=pl, valid=valid, box=box, dropped=dropped, morton_keys=mk, order=order, chunks=chunks, words=words,
                          sh=sh, decoded=S.decode(chunks, words, sh, degree), importance_keys=ik, splat_order=so, splat=splat,
                          splat_decoded=S.splat_decode(splat), alpha_pre=S.alpha_pre(c), importance_pre=S.importance_pre(c, pl))
    return _kept[key]


def near_boundary(pre):
    """Rows whose ``pre`` (a value about to be floored after + 0.5 was added) lies within 2^-30 of an integer."""
    with np.errstate(invalid="ignore"):
        return np.abs(pre - np.round(pre)) <= 2.0 ** -30


def near_fp32_boundary(pre):
    """Rows whose double ``pre`` lies within 2^-30 fp32 spacings of the midpoint of two neighbouring fp32 values."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = S.f32(pre).astype(np.float64)
        ulp = np.spacing(np.abs(S.f32(pre))).astype(np.float64)
        return np.abs(np.abs(pre - f) - 0.5 * ulp) <= 2.0 ** -30 * ulp


# ---- the comparisons both test files make ------------------------------------------------------------------------------------------

def exempt_bytes(got, want, pre):
    """The alpha bytes ``got`` against ``want`` (the reference): equal, or one apart where the restatement's value before the floor,
    ``pre``, lies within 2^-30 of an integer; the share of such rows is capped at 1e-3 (a condition).  Returns how many differ."""
    d = got.astype(np.int64) - want.astype(np.int64)
    differ = d != 0
    assert (np.abs(d) <= 1).all(), np.flatnonzero(np.abs(d) > 1)[:8]
    assert not (differ & ~near_boundary(pre)).any(), np.flatnonzero(differ & ~near_boundary(pre))[:8]
    assert differ.sum() <= 1e-3 * max(differ.size, 1)
    return int(differ.sum())


def exempt_keys(got, want, pre, valid):
    """Importance keys ``got`` against ``want``: equal, or -- for a valid row whose importance before the rounding lies within 2^-30
    fp32 spacings of a rounding boundary -- importance bits one apart; the same cap.  Returns how many differ."""
    differ = got != want
    d = (got >> 31) - (want >> 31)
    assert ((got & 0x7FFFFFFF) == (want & 0x7FFFFFFF)).all()
    assert (np.abs(d) <= 1).all()
    allowed = (valid != 0) & near_fp32_boundary(pre)
    assert not (differ & ~allowed).any(), np.flatnonzero(differ & ~allowed)[:8]
    assert differ.sum() <= 1e-3 * max(differ.size, 1)
    return int(differ.sum())


def spacing_off(got, want):
    """fp32 arrays: (words beyond one fp32 spacing of ``want`` -- must be 0 --, words that differ at all).  Equal bits always pass."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    same = g.view(np.uint32) == w.view(np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.abs(g.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)
    return int((~same & ~near).sum()), int((~same).sum())
