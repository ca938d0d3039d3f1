"""Densifying a cloud of surfels under refinement (include/lara_splatdensify.h, csrc/splatdensify.hip): the other half of the
Gaussian-splatting optimisation loop beside ``splatrefine``'s Adam step.  Surfels whose screen-space gradient is high are cloned (the
small ones) or split into ``N`` children (the large ones), the transparent and the oversized are pruned, and the Adam moments travel
with the rows that survive.  Opt-in like every module here, imported by nothing on the default routes (``splatrefine`` imports it
when a schedule is given).

  * ``plan``            the float64 row of one round: threshold, the size limits as logs, the opacity limit as a logit, N, three flags;
  * ``DensifyStats``    the three statistic rows of a cloud, ``accumulate(grad_means2D, radii)`` after each backward, ``reset(P)``;
  * ``decide``          action [P], the exclusive offsets [3 P] and the five counts, all on the tensors' device;
  * ``apply``           the new cloud and its moments from the decision: reads the counts (the ONE host read of a round, needed to
                        allocate), two launches;
  * ``densify``         decide + apply, with ``max_surfels``;
  * ``reset_opacity``   3DGS's opacity reset: the logit clamped to ``logit(ceiling)``, the opacity moments zeroed (torch operators);
  * ``DensifySchedule`` what ``splatrefine.refine(..., densify=...)`` takes.

The rules are 3DGS's / 2DGS's ``densify_and_prune`` as recalled [RECALLED: neither code base is in the build image; nothing pins them;
the defaults below are their training arguments as recalled: densify_grad_threshold 2e-4, percent_dense 0.01, min opacity 0.005,
opacity reset to 0.01, children 2 shrunk by 0.8 N].  One deliberate difference: 3DGS applies its prune test after the new rows exist,
with a zero screen radius for them; here a row that fails the test leaves no descendants.

The statistic is PER RENDER CALL, not per view: ``render_views`` sums the screen-space gradient over the views of a call, so one call
of V views adds one norm and one count to the surfels any of its views saw.  ``views_per_step=1`` gives 3DGS's per-view statistic.

The output order is fixed, and it is 3DGS's: the surviving originals ascending, then the clones ascending by source, then the split
children ascending by source, child 0 .. N - 1.  A split child's centre is its parent's plus R(q / |q|) (exp(s0) z0, exp(s1) z1, 0) with
z from a caller-supplied ``noise`` [P,N,2] (``torch.randn`` under a seeded generator when None): no random-number generator runs in
the kernel, so a round is reproducible.

Tensors on the GPU go through the kernels.  Tensors on the host go through the ``*_host`` entries, the same per-row functions compiled
for the CPU (csrc/splatdensify_ops.h): the reference the kernels are held to, not a fast path.  Either way through
``_native.call_on``: the seven functions are rows of ``_native.SIGNATURES`` like every other.

Out of scope: learning-rate schedules, 3DGS's prune-after-append ordering, absolute-gradient statistics, per-view statistics inside a
multi-view call, merging of surfels.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import splatio
from . import splatrefine
from . import _native
from ._native import host_array

PLAN = 8                                 # include/lara_splatdensify.h
SPAN = 256
MAX_SURFELS = 1 << 27
KEEP, CLONE, SPLIT, PRUNE = 0, 1, 2, 3
NO_CHILD = 255
ALLOW_CLONE, ALLOW_SPLIT, ALLOW_PRUNE = 1, 2, 4
COUNT_KEYS = ("kept", "cloned", "split", "pruned", "P_out")
FIELDS = splatio.SurfelCloud.FIELDS
_WHO = "lara_amd.splatdensify"
_workspace = _native.StreamWorkspace()


# ---------------------------------------------------------------------------------------------------------- the plan

def plan(grad_threshold=2e-4, percent_dense=0.01, extent=1.0, min_opacity=0.005, max_screen_radius=0, n_split=2, clone=True, split=True,
         prune=True):
    """The plan of one round as 8 float64 (numpy): [0] grad_threshold, [1] log(percent_dense extent), [2] logit(min_opacity),
    [3] max_screen_radius (<= 0: the screen and world limits are off), [4] log(0.1 extent), [5] log(0.8 n_split), [6] n_split (the
    children per split, 1..8), [7] 1 (clone allowed) + 2 (split allowed) + 4 (prune allowed).  ``extent`` is the scene's radius, as
    3DGS's ``cameras_extent``.  Every value is computed in float64 on the host; the kernels run no exp, log or sigmoid on it."""
    n = int(n_split)
    m, e, d = float(min_opacity), float(extent), float(percent_dense)
    if n != n_split or not 1 <= n <= 8 or not e > 0.0 or not d > 0.0 or not 0.0 <= m < 1.0 or math.isnan(float(grad_threshold)):
        raise ValueError(f"{_WHO}: a plan needs n_split in 1..8, extent > 0, percent_dense > 0, min_opacity in [0, 1) and a threshold "
                         f"that is a number, got {n_split!r}, {extent!r}, {percent_dense!r}, {min_opacity!r}, {grad_threshold!r}")
    row = np.empty(PLAN, np.float64)
    row[:] = (float(grad_threshold), math.log(d * e), -math.inf if m == 0.0 else math.log(m / (1.0 - m)), float(max_screen_radius),
              math.log(0.1 * e), math.log(0.8 * n), float(n),
              float((ALLOW_CLONE if clone else 0) | (ALLOW_SPLIT if split else 0) | (ALLOW_PRUNE if prune else 0)))
    return row


def _plan_row(plan):
    row = np.asarray(plan, np.float64)
    if row.shape != (PLAN,) or not (1.0 <= row[6] <= 8.0 and row[6] == int(row[6]) and 0.0 <= row[7] <= 7.0 and row[7] == int(row[7])):
        raise ValueError(f"{_WHO}: a plan is {PLAN} doubles (splatdensify.plan) with n_split in 1..8 and flags in 0..7")
    return row


def _row(what, t, shape, dtype, dev):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{_WHO}: {what} is a contiguous {dtype} tensor {list(shape)} on {dev}")
    return t


# ---------------------------------------------------------------------------------------------------------- the statistics

class DensifyStats:
    """The statistics of ``P`` surfels on ``device``: ``grad_sum`` (fp32, the sum of the screen-space gradient norms), ``seen``
    (int32, the render calls that saw the surfel and handed back a finite gradient) and ``max_radius`` (int32, the largest screen
    radius any view gave it), all [P]."""

    def __init__(self, P, device):
        self.device = torch.device(device)
        self.reset(P)

    def reset(self, P):
        """Fresh zero rows for ``P`` surfels (after a round: the new count)."""
        self.grad_sum = torch.zeros(int(P), dtype=torch.float32, device=self.device)
        self.seen = torch.zeros(int(P), dtype=torch.int32, device=self.device)
        self.max_radius = torch.zeros(int(P), dtype=torch.int32, device=self.device)

    @property
    def n_surfels(self):
        return self.grad_sum.shape[0]

    @torch.no_grad()
    def accumulate(self, grad_means2D, radii):
        """One render call: ``grad_means2D`` [P,3] fp32 is the gradient of ``render_views``' ``means2D`` argument after ``backward``
        (summed over the call's views by the rasteriser), ``radii`` [V,P] int32 the rasteriser's own (``raster_out[0][1]``).  A
        surfel with a positive radius in any view adds the norm of its first two gradient words (in double, rounded once) and one to
        its count, unless a word is not finite; its largest radius is kept either way.  One launch, no host read."""
        P, dev = self.n_surfels, self.device
        _row("grad_means2D", grad_means2D, (P, 3), torch.float32, dev)
        if not isinstance(radii, torch.Tensor) or radii.dim() != 2 or radii.shape[0] < 1:
            raise ValueError(f"{_WHO}: radii is an int32 tensor [V,{P}] with V >= 1")
        _row("radii", radii, (radii.shape[0], P), torch.int32, dev)
        if P:
            _native.call_on("lara_splatdensify_accumulate", dev, P, radii.shape[0], grad_means2D, radii, self.grad_sum, self.seen,
                            self.max_radius)


# ---------------------------------------------------------------------------------------------------------- the decision

@torch.no_grad()
def decide(params, stats, plan):
    """(action [P] uint8, offset [3 P] int32, counts [5] int64), on the tensors' device: every surfel's action (``KEEP``, ``CLONE``,
    ``SPLIT``, ``PRUNE``) from its stored opacity and scales and its statistics under ``plan``, the exclusive scan of
    [1 per keep or clone | 1 per clone | N per split], and the counts ``COUNT_KEYS``: kept, cloned, split parents, pruned, P_out.
    No host read."""
    params = splatio.check_fields(_WHO, "params", [p.detach() for p in params])
    dev, P = params[0].device, params[0].shape[0]
    row = _plan_row(plan)
    if not isinstance(stats, DensifyStats) or stats.n_surfels != P or stats.device != dev:
        raise ValueError(f"{_WHO}: stats is a DensifyStats of {P} surfels on {dev}")
    if P > MAX_SURFELS:
        raise ValueError(f"{_WHO}: at most 2^27 surfels, got {P}")
    action = torch.empty(P, dtype=torch.uint8, device=dev)
    offset = torch.empty(3 * P, dtype=torch.int32, device=dev)
    counts = torch.zeros(5, dtype=torch.int64, device=dev)
    if P == 0:                               # (an empty tensor has no address to hand over; nothing is launched)
        return action, offset, counts
    ws = None
    if dev.type == "cuda":
        ws = _workspace(dev, _native.query("lara_splatdensify_workspace_bytes", P))
    _native.call_on("lara_splatdensify_decide", dev, host_array("d", row.tolist()), P, params[2], params[3], stats.grad_sum, stats.seen,
                    stats.max_radius, action, offset, counts, ws)
    return action, offset, counts


# ---------------------------------------------------------------------------------------------------------- the application

def _noise(noise, P, n, dev, seed):
    if noise is None:
        g = torch.Generator(device=dev).manual_seed(int(seed))
        return torch.randn((P, n, 2), dtype=torch.float32, device=dev, generator=g)
    return _row("noise", noise, (P, n, 2), torch.float32, dev)


@torch.no_grad()
def apply(params, exp_avg, exp_avg_sq, action, offset, counts, plan, noise=None, seed=0):
    """The cloud after the round ``decide`` described: (params', exp_avg', exp_avg_sq', row_source [P_out] int32, row_child [P_out]
    uint8, the five counts as a dict of ints).  Reads ``counts`` on the host -- the one host read of a round, needed to allocate --
    then two launches: the rows' sources, and the gather over the 15 arrays.  Kept and cloned rows carry their parameter words bit
    for bit, kept rows their moment words too; clones and split children start from zero moments; a split child's scales shrink by
    0.8 N and its centre moves by ``noise`` [P,N,2] (None: ``torch.randn`` under a generator seeded with ``seed``).  ``row_child``
    is ``NO_CHILD`` (255) for rows that are not split children.  The inputs are left as they are."""
    params = splatio.check_fields(_WHO, "params", [p.detach() for p in params])
    exp_avg, exp_avg_sq = (splatio.check_fields(_WHO, w, ts, like=params) for w, ts in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)))
    dev, P, n_coeffs = params[0].device, params[0].shape[0], params[1].shape[1]
    row = _plan_row(plan)
    n = int(row[6])
    _row("action", action, (P,), torch.uint8, dev)
    _row("offset", offset, (3 * P,), torch.int32, dev)
    _row("counts", counts, (5,), torch.int64, dev)
    noise = _noise(noise, P, n, dev, seed)
    five = dict(zip(COUNT_KEYS, (int(v) for v in counts.tolist())))
    P_out, survivors = five["P_out"], five["kept"] + five["cloned"]
    if min(five.values()) < 0 or P_out != survivors + five["cloned"] + n * five["split"] or survivors + five["split"] + five["pruned"] != P:
        raise ValueError(f"{_WHO}: counts {five} do not describe a round of {P} surfels with {n} children per split")
    outs = [[t.new_empty((P_out,) + tuple(t.shape[1:])) for t in ts] for ts in (params, exp_avg, exp_avg_sq)]
    row_source = torch.empty(P_out, dtype=torch.int32, device=dev)
    row_child = torch.empty(P_out, dtype=torch.uint8, device=dev)
    if P and P_out:
        _native.call_on("lara_splatdensify_apply", dev, host_array("d", row.tolist()), splatio.SH_COEFFS[n_coeffs], P, P_out, survivors,
                        action, offset, noise, host_array("p", params + exp_avg + exp_avg_sq), host_array("p", outs[0] + outs[1] + outs[2]),
                        row_source, row_child)
    return outs[0], outs[1], outs[2], row_source, row_child, five


def densify(params, exp_avg, exp_avg_sq, stats, plan, noise=None, seed=0, max_surfels=None):
    """One round: ``decide`` and ``apply``.  Returns (params', exp_avg', exp_avg_sq', report); ``report`` holds the five counts
    (``COUNT_KEYS``, ints), ``counts`` (the same as the int64 device tensor), ``row_source`` and ``row_child`` (so a caller can carry
    per-surfel data of its own) and ``capped``.  ``max_surfels``: if P_out would exceed it, the round is decided again with clone and
    split off, so it only prunes, and ``capped`` is True (one more host read)."""
    row = _plan_row(plan)
    action, offset, counts = decide(params, stats, row)
    capped = False
    if max_surfels is not None and int(counts[4]) > int(max_surfels):
        row = row.copy()
        row[7] = float(int(row[7]) & ALLOW_PRUNE)
        action, offset, counts = decide(params, stats, row)
        capped = True
    p, m, v, row_source, row_child, five = apply(params, exp_avg, exp_avg_sq, action, offset, counts, row, noise=noise, seed=seed)
    return p, m, v, dict(five, counts=counts, row_source=row_source, row_child=row_child, capped=capped)


@torch.no_grad()
def reset_opacity(params, exp_avg, exp_avg_sq, ceiling=0.01):
    """3DGS's opacity reset [RECALLED]: every opacity logit above ``logit(ceiling)`` is set to it, and the opacity's two moments are
    zeroed, in place.  torch operators on the one [P,1] tensor, no kernel; the version counter advances."""
    c = float(ceiling)
    if not 0.0 < c < 1.0:
        raise ValueError(f"{_WHO}: the opacity ceiling lies in (0, 1), got {ceiling!r}")
    opacity = params[2].detach()
    opacity.clamp_(max=math.log(c / (1.0 - c)))
    exp_avg[2].zero_()
    exp_avg_sq[2].zero_()
    splatrefine.bump_version([params[2]])


# ---------------------------------------------------------------------------------------------------------- the schedule

@dataclasses.dataclass
class DensifySchedule:
    """When and how ``splatrefine.refine`` densifies.  Steps count from 1, after the step's update: a round runs at step t when
    ``from_step <= t <= until_step`` and ``(t - from_step) % interval == 0``; the opacity is reset at the steps of that range that
    are multiples of ``opacity_reset_interval`` (0: never).  ``extent`` is the scene's radius; ``max_screen_radius`` 0 leaves the
    screen and world limits off.  The defaults are 3DGS's training arguments as recalled [RECALLED], scaled to a refinement of a few
    hundred steps, not of 30 000."""
    from_step: int = 50
    until_step: int = 10 ** 9
    interval: int = 100
    grad_threshold: float = 2e-4
    percent_dense: float = 0.01
    extent: float = 1.0
    min_opacity: float = 0.005
    max_screen_radius: float = 0.0
    opacity_reset_interval: int = 0
    n_split: int = 2
    max_surfels: int | None = None
    seed: int = 0

    def __post_init__(self):
        if int(self.interval) < 1 or int(self.from_step) < 1 or int(self.opacity_reset_interval) < 0:
            raise ValueError(f"{_WHO}: a schedule needs from_step >= 1, interval >= 1 and opacity_reset_interval >= 0")
        self.plan()

    def plan(self):
        return plan(self.grad_threshold, self.percent_dense, self.extent, self.min_opacity, self.max_screen_radius, self.n_split)

    def fires(self, t):
        return self.from_step <= t <= self.until_step and (t - self.from_step) % self.interval == 0

    def resets(self, t):
        return self.opacity_reset_interval > 0 and self.from_step <= t <= self.until_step and t % self.opacity_reset_interval == 0
