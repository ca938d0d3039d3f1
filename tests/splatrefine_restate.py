"""The update of include/lara_splatadam.h restated in numpy float64: the same formula in the same operation order, each operation one
correctly rounded IEEE operation on arrays, one rounding to float32 per store.  The plan is built here from the step, the betas, eps
and the six rates, without the module."""
import math

import numpy as np

FIELDS = ("centers", "shs", "opacity", "scales", "rotations")
QNAN = np.uint32(0x7FC00000)


def plan(step, lrs, betas=(0.9, 0.999), eps=1e-15):
    b1, b2 = float(betas[0]), float(betas[1])
    return np.array([b1, 1.0 - b1, b2, 1.0 - b2, 1.0 - b1 ** int(step), math.sqrt(1.0 - b2 ** int(step)), float(eps)] + [float(v) for v in lrs],
                    np.float64)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def rates(row, field, shape):
    """The learning rate of every word of a field, float64, in the field's shape."""
    lr = row[7:13]
    if field == "shs":
        out = np.full(shape, lr[2], np.float64)
        out[:, 0, :] = lr[1]
        return out
    return np.full(shape, lr[{"centers": 0, "opacity": 3, "scales": 4, "rotations": 5}[field]], np.float64)


def _round(x):
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
    w = f.view(np.uint32).copy()
    w[np.isnan(f)] = QNAN
    return w.view(np.float32)


def step(row, params, grads, exp_avg, exp_avg_sq, visible=None, zero_grads=False):
    """(params', grads', exp_avg', exp_avg_sq', skipped): dicts of new float32 arrays; the inputs are left as they are."""
    out_p, out_g, out_m, out_v, skipped = {}, {}, {}, {}, 0
    for k in FIELDS:
        p, g, m, v = params[k], grads[k], exp_avg[k], exp_avg_sq[k]
        seen = np.ones(p.shape[0], bool) if visible is None else np.asarray(visible) != 0
        seen = seen.reshape((-1,) + (1,) * (p.ndim - 1))
        finite = np.isfinite(g)
        skipped += int((seen & ~finite).sum())
        take = seen & finite
        with np.errstate(all="ignore"):
            gd = np.where(finite, g, np.float32(0)).astype(np.float64)          # (the skipped words' results are not taken)
            md, vd, pd = m.astype(np.float64), v.astype(np.float64), p.astype(np.float64)
            m1 = md + (gd - md) * row[1]
            v1 = row[2] * vd + (row[3] * gd) * gd
            denom = np.sqrt(v1) / row[5] + row[6]
            p1 = pd - (rates(row, k, p.shape) / row[4]) * (m1 / denom)
        for old, new, out in ((p, p1, out_p), (m, m1, out_m), (v, v1, out_v)):
            w = words(old).copy()
            w[take] = _round(new).view(np.uint32)[take]
            out[k] = w.view(np.float32)
        out_g[k] = np.zeros_like(g) if zero_grads else g.copy()
    return out_p, out_g, out_m, out_v, skipped
