"""The rules of include/lara_splatdensify.h restated in numpy, float64 and integers: the statistics of a render call, every surfel's
action with the exclusive offsets and the counts, and the output cloud with its moments -- the same formulas in the same operation
order, each one correctly rounded IEEE operation on arrays, one rounding to float32 per store.  Written from the header, without
the module.  The one step that is not correctly rounded on either side is the float64 exp of a split child's centre."""
import numpy as np

FIELDS = ("centers", "shs", "opacity", "scales", "rotations")
QNAN = np.uint32(0x7FC00000)
KEEP, CLONE, SPLIT, PRUNE, NO_CHILD = 0, 1, 2, 3, 255


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _round(x):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(x, np.float64).astype(np.float32)
    w = f.view(np.uint32).copy()
    w[np.isnan(f)] = QNAN
    return w.view(np.float32)


def accumulate(grad, radii, grad_sum, seen, max_radius):
    """(grad_sum', seen', max_radius') after one render call; the inputs are left as they are."""
    any_seen = (radii > 0).any(0)
    most = np.maximum(radii.max(0), 0) if radii.shape[1] else np.zeros(0, np.int32)
    finite = np.isfinite(grad[:, 0]) & np.isfinite(grad[:, 1])
    with np.errstate(all="ignore"):
        gx, gy = grad[:, 0].astype(np.float64), grad[:, 1].astype(np.float64)
        n = np.sqrt(gx * gx + gy * gy)
        new_sum = _round(grad_sum.astype(np.float64) + n)
    take = any_seen & finite
    out_sum = words(grad_sum).copy()
    out_sum[take] = words(new_sum)[take]
    out_seen = seen + take.astype(np.int32)
    out_max = np.where(any_seen, np.maximum(max_radius, most), max_radius).astype(np.int32)
    return out_sum.view(np.float32), out_seen, out_max


def decide(row, opacity, scales, grad_sum, seen, max_radius):
    """(action [P] uint8, offset [3 P] int32, counts [5] int64) under the plan ``row``."""
    P = opacity.shape[0]
    n_split, flags = int(row[6]), int(row[7])
    op, s0, s1 = opacity.reshape(P).astype(np.float64), scales[:, 0].astype(np.float64), scales[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        avg = np.where(seen > 0, grad_sum.astype(np.float64) / np.maximum(seen, 1), 0.0)
        hot = avg >= row[0]
        smax = np.where(s0 > s1, s0, s1)
        gone = np.zeros(P, bool)
        if flags & 4:
            gone = (op < row[2]) | ~np.isfinite(op) | ~np.isfinite(s0) | ~np.isfinite(s1)
            if row[3] > 0.0:
                gone |= (max_radius.astype(np.float64) > row[3]) | (smax > row[4])
        split = ~gone & hot & (smax > row[1])
        clone = ~gone & hot & (smax <= row[1])
    action = np.full(P, KEEP, np.uint8)
    action[clone & bool(flags & 1)] = CLONE
    action[split & bool(flags & 2)] = SPLIT
    action[gone] = PRUNE
    first = ((action == KEEP) | (action == CLONE)).astype(np.int64)
    second = (action == CLONE).astype(np.int64)
    third = (action == SPLIT).astype(np.int64) * n_split
    flat = np.concatenate([first, second, third])
    offset = (np.cumsum(flat) - flat).astype(np.int32)
    a, b, c = int(first.sum()), int(second.sum()), int(third.sum())
    counts = np.array([a - b, b, c // n_split, P - a - c // n_split, a + b + c], np.int64)
    return action, offset, counts


def rows(action, offset, counts, n_split):
    """(row_source [P_out] int32, row_child [P_out] uint8): the surviving originals ascending, the clones ascending by source, the
    split children ascending by source, child 0 .. N - 1 -- built from the order itself, not from ``offset``."""
    idx = np.arange(action.shape[0], dtype=np.int32)
    survive = idx[(action == KEEP) | (action == CLONE)]
    clones = idx[action == CLONE]
    parents = idx[action == SPLIT]
    source = np.concatenate([survive, clones, np.repeat(parents, n_split)]).astype(np.int32)
    child = np.concatenate([np.full(survive.size + clones.size, NO_CHILD, np.uint8), np.tile(np.arange(n_split, dtype=np.uint8), parents.size)])
    assert source.size == int(counts[4])
    return source, child


def child_centers(centers, scales, rotations, z):
    """[M,3] float64 before the one rounding: c + R(q / |q|) (exp(s0) z0, exp(s1) z1, 0) in the header's operation order."""
    c, s, q, z = (a.astype(np.float64) for a in (centers, scales, rotations, z))
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    with np.errstate(all="ignore"):
        n2 = ((qw * qw + qx * qx) + qy * qy) + qz * qz
        inv = 1.0 / np.sqrt(n2)
        w, x, y, zz = qw * inv, qx * inv, qy * inv, qz * inv
        r0 = np.stack([1.0 - 2.0 * (y * y + zz * zz), 2.0 * (x * y + w * zz), 2.0 * (x * zz - w * y)], 1)
        r1 = np.stack([2.0 * (x * y - w * zz), 1.0 - 2.0 * (x * x + zz * zz), 2.0 * (y * zz + w * x)], 1)
        u = np.exp(s[:, 0]) * z[:, 0]
        v = np.exp(s[:, 1]) * z[:, 1]
        return c + (r0 * u[:, None] + r1 * v[:, None])


def apply(row, params, exp_avg, exp_avg_sq, action, offset, counts, noise):
    """(params', exp_avg', exp_avg_sq', row_source, row_child, centres64): dicts of new float32 arrays; ``centres64`` is the float64
    value of every split child's centre before its rounding ([children, 3]; the rows where row_child != 255)."""
    n_split = int(row[6])
    source, child = rows(action, offset, counts, n_split)
    survivors = int(counts[0] + counts[1])
    is_child = child != NO_CHILD
    out_p = {k: params[k][source].copy() for k in FIELDS}
    out_m = {k: exp_avg[k][source].copy() for k in FIELDS}
    out_v = {k: exp_avg_sq[k][source].copy() for k in FIELDS}
    for d in (out_m, out_v):
        for k in FIELDS:
            d[k][survivors:] = 0.0
    src = source[is_child]
    with np.errstate(all="ignore"):
        out_p["scales"][is_child] = _round(params["scales"][src].astype(np.float64) - row[5])
    centres64 = child_centers(params["centers"][src], params["scales"][src], params["rotations"][src], noise[src, child[is_child]])
    out_p["centers"][is_child] = _round(centres64)
    return out_p, out_m, out_v, source, child, centres64
